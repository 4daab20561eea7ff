// optim.hip -- the fused Adam + EMA update over flat parameter buffers, with the step count on the host or in device memory.
#include "elementwise.hpp"

namespace srganfd {

// ---- fused Adam (torch.optim.Adam maths, train_bsrgan.py:311-323) + EMA (train_bsrgan.py:290-291,470) ----
__global__ __launch_bounds__(256) void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                       float* __restrict__ ema, size_t n, float lr, float b1, float b2, float eps, float wd,
                                                       float bc1, float bc2_sqrt, float gscale, float ema_decay, int ema_mode,
                                                       const float* __restrict__ skip, const float* __restrict__ gscale_dev) {
  if (gscale_dev) gscale *= *gscale_dev;      // 1 / loss scale, from the device-resident scaler state
  // loss-scaled (f16) training: a non-finite gradient skips the parameter update (GradScaler.step, train_bsrgan.py:436,466); the
  // EMA still advances -- the reference calls update_parameters() after every iteration (:470)
  const bool skipped = skip && *skip != 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    if (skipped) {
      if (ema_mode == 1) ema[i] = p[i];
      else if (ema_mode == 2) ema[i] = (1.f - ema_decay) * ema[i] + ema_decay * p[i];
      continue;
    }
    float gi = g[i] * gscale;
    float pi = p[i];
    if (wd != 0.f) gi += wd * pi;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi -= (lr / bc1) * (mi / denom);
    p[i] = pi;
    if (ema_mode == 1) ema[i] = pi;                                               // first update: copy
    else if (ema_mode == 2) ema[i] = (1.f - ema_decay) * ema[i] + ema_decay * pi; // reference avg_fn
  }
}

// Step counter and bias corrections in device memory (hipGraph replays cannot change kernel arguments): one thread
// advances *step and writes bc = {1 - b1^t, sqrt(1 - b2^t)}; the Adam kernel then reads them.
__global__ void adam_step_kernel(int* __restrict__ step, float b1, float b2, float* __restrict__ bc, const float* __restrict__ skip) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && !(skip && *skip != 0.f)) {      // a skipped step does not count (torch: state["step"] unchanged)
    const int t = *step + 1;
    *step = t;
    bc[0] = (float)(1.0 - pow((double)b1, (double)t));
    bc[1] = (float)sqrt(1.0 - pow((double)b2, (double)t));
  }
}
__global__ __launch_bounds__(256) void adam_ema_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                           float* __restrict__ ema, size_t n, float lr, float b1, float b2, float eps, float wd,
                                                           const float* __restrict__ bc, float gscale, float ema_decay, int ema_mode,
                                                           const float* __restrict__ skip, const float* __restrict__ gscale_dev) {
  const float bc1 = bc[0], bc2_sqrt = bc[1];
  if (gscale_dev) gscale *= *gscale_dev;
  const bool skipped = skip && *skip != 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    if (skipped) {
      if (ema_mode == 1) ema[i] = p[i];
      else if (ema_mode == 2) ema[i] = (1.f - ema_decay) * ema[i] + ema_decay * p[i];
      continue;
    }
    float gi = g[i] * gscale;
    float pi = p[i];
    if (wd != 0.f) gi += wd * pi;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi -= (lr / bc1) * (mi / denom);
    p[i] = pi;
    if (ema_mode == 1) ema[i] = pi;
    else if (ema_mode == 2) ema[i] = (1.f - ema_decay) * ema[i] + ema_decay * pi;
  }
}

// ------------------------------------------------------------------------------------------------
extern "C" int srganfd_adam_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t numel, float lr, float b1, float b2, float eps, float wd,
                                int32_t step, float grad_scale, float ema_decay, int32_t ema_mode, const float* skip_flag, const float* grad_scale_dev,
                                void* stream) {
  const size_t n = (size_t)numel;
  const hipStream_t s = (hipStream_t)stream;
  if (!p || !g || !m || !v || step < 1 || (ema_mode && !ema)) return set_err(SRGANFD_EINVAL, "adam: bad args");
  if (numel <= 0) return set_err(SRGANFD_EINVAL, "adam: numel <= 0");
  if (ema_mode < 0 || ema_mode > 2) return set_err(SRGANFD_EINVAL, "adam: ema_mode %d is none of 0, 1, 2", (int)ema_mode);
  const double bc1 = 1.0 - pow((double)b1, step), bc2 = 1.0 - pow((double)b2, step);
  SRGANFD_LAUNCH(adam_ema_kernel, dim3(grid_for(n)), dim3(256), 0, s, p, g, m, v, ema, n, lr, b1, b2, eps, wd, (float)bc1, (float)sqrt(bc2),
                     grad_scale, ema_decay, ema_mode, skip_flag, grad_scale_dev);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_adam_ema_dev(float* p, const float* g, float* m, float* v, float* ema, int64_t numel, float lr, float b1, float b2, float eps, float wd,
                                    int32_t* step_dev, float* bc_dev, float grad_scale, float ema_decay, int32_t ema_mode, const float* skip_flag,
                                    const float* grad_scale_dev, void* stream) {
  const size_t n = (size_t)numel;
  const hipStream_t s = (hipStream_t)stream;
  if (!p || !g || !m || !v || !step_dev || !bc_dev || (ema_mode && !ema)) return set_err(SRGANFD_EINVAL, "adam(dev): bad args");
  if (numel <= 0) return set_err(SRGANFD_EINVAL, "adam(dev): numel <= 0");
  if (ema_mode < 0 || ema_mode > 2) return set_err(SRGANFD_EINVAL, "adam(dev): ema_mode %d is none of 0, 1, 2", (int)ema_mode);
  SRGANFD_LAUNCH(adam_step_kernel, dim3(1), dim3(64), 0, s, step_dev, b1, b2, bc_dev, skip_flag);
  SRGANFD_LAUNCH(adam_ema_dev_kernel, dim3(grid_for(n)), dim3(256), 0, s, p, g, m, v, ema, n, lr, b1, b2, eps, wd, (const float*)bc_dev, grad_scale,
                 ema_decay, ema_mode, skip_flag, grad_scale_dev);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

}  // namespace srganfd
