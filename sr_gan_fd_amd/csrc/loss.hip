// loss.hip -- the scalar losses and what scales them: L1 (flat, on views, its gradient on views), BCE-with-logits and its
// relativistic-average form, sigmoid(mean), the non-finite flag and the device-resident loss scaler.
#include "elementwise.hpp"

namespace srganfd {

// ---- losses.  out[slot] (+)= weight * mean(...) ; two-stage deterministic reduction (store_block_sum, finish_kernel: elementwise.hpp) ----
// The four partial kernels on flat arrays share the tail and spell their loops out: through grid_stride's lambda l1_partial_kernel and
// bce_rel_partial_kernel compiled to other code (profiles/view_kernels_refactor_isa.txt).
// L1 (nn.L1Loss, train_bsrgan.py:297,450) on flat fp32 arrays, optional gradient wrt a.
__global__ __launch_bounds__(256) void l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n, float gscale,
                                                         const float* __restrict__ gscale_dev, float* __restrict__ grad, float* __restrict__ partial) {
  __shared__ float sh[4];
  float s = 0.f;
  if (gscale_dev) gscale *= *gscale_dev;      // the loss scale lives in device memory (srganfd_loss_scale_update), as torch's GradScaler keeps it
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float d = a[i] - b[i];
    s += fabsf(d);
    if (grad) grad[i] = d > 0.f ? gscale : (d < 0.f ? -gscale : 0.f);      // torch.sign: 0 at 0 and at a NaN
  }
  store_block_sum(s, sh, partial);
}
// L1 between two NHWC T views (VGG feature taps, model.py:548-550), no gradient (detached in the reference): vector form N = VecN<T>::N,
// scalar form N = 1.  l1_grad_views_kernel below is the differentiable tap's gradient (ESRGAN/model.py:281-292): that of mean |a - b|
// w.r.t. a, into out; it has the scalar form only.
struct L1K { View a, b, out; size_t npix; int c, relu; float* partial; const float* upstream; float scale; };
template <typename T, int N>
__global__ __launch_bounds__(256) void l1_views_partial_kernel(const L1K k) {
  __shared__ float sh[4];
  float s = 0.f;
  for_each_group<N>(k.npix, k.c, [&](size_t p, int ch) {
    float va[N], vb[N];
    ldn<T, N>(k.a.p, k.a.at(p, ch), va);
    ldn<T, N>(k.b.p, k.b.at(p, ch), vb);
    each<N>([&](int q) {
      float x = va[q], y = vb[q];
      if (k.relu) { x = x < 0.f ? 0.f : x; y = y < 0.f ? 0.f : y; }      // torch's relu: a NaN stays one (fmaxf would turn it into 0)
      s += fabsf(x - y);
    });
  });
  store_block_sum(s, sh, k.partial);
}
template <typename T>
__global__ __launch_bounds__(256) void l1_grad_views_kernel(const L1K k) {
  const float sc = k.scale * (k.upstream ? *k.upstream : 1.f);
  for_each_group<1>(k.npix, k.c, [&](size_t p, int ch) {
    const float d = ld<T>(k.a.p, k.a.at(p, ch)) - ld<T>(k.b.p, k.b.at(p, ch));
    st<T>(k.out.p, k.out.at(p, ch), d > 0.f ? sc : (d < 0.f ? -sc : 0.f));     // torch.sign: 0 at 0 and at a NaN
  });
}
// BCE-with-logits against a constant label map (train_bsrgan.py:301,403-404): loss and sigmoid mean
__global__ __launch_bounds__(256) void bce_partial_kernel(const float* __restrict__ x, size_t n, float target, float gscale,
                                                          const float* __restrict__ gscale_dev, float* __restrict__ grad, float* __restrict__ partial,
                                                          float* __restrict__ partial_sig) {
  __shared__ float sh[4];
  float s = 0.f, sg = 0.f;
  if (gscale_dev) gscale *= *gscale_dev;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float v = x[i];
    s += fmaxf(v, 0.f) - v * target + log1pf(expf(-fabsf(v)));
    const float sig = 1.f / (1.f + expf(-v));
    sg += sig;
    if (grad) grad[i] = (sig - target) * gscale;
  }
  store_block_sum(s, sh, partial);
  store_block_sum(sg, sh, partial_sig);
}
// the plain sum: stage one of sigmoid(mean(logits)) and of the relativistic form's mean(other)
__global__ __launch_bounds__(256) void sum_partial_kernel(const float* __restrict__ x, size_t n, float* __restrict__ partial) {
  __shared__ float sh[4];
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) s += x[i];
  store_block_sum(s, sh, partial);
}
// The epilogues of finish_kernel.  FinAxpy: out (+)= sum * scale, every loss.  FinMean: out = sum / n, the relativistic form's mean(other).
// FinSigmoidMean: out = sigmoid(sum / n), the D(x) probability as ESRGAN / Real-ESRGAN log it (train_esrgan.py:430-431,
// train_realesrgan.py:475-476; BSRGAN / A-ESRGAN log mean(sigmoid(logits)) instead -- bce_partial_kernel's second output).
struct FinBase {
  const float* table; int n; float scale; float* out;
  __device__ const float* partial() const { return table; }
  __device__ int nblk() const { return n; }
};
struct FinAxpy : FinBase { int accumulate; __device__ void store(float r) const { *out = (accumulate ? *out : 0.f) + r * scale; } };
struct FinMean : FinBase { __device__ void store(float r) const { *out = r * scale; } };
struct FinSigmoidMean : FinBase { __device__ void store(float r) const { *out = 1.f / (1.f + expf(-r * scale)); } };
// ---- relativistic-average BCE (ESRGAN/train_esrgan.py:378-380,404,412): mean_i BCE(x_i - mean(other), target) ----
// stage 0: mean(other) -> ws[2 * kRedBlocks] (sum_partial_kernel + FinMean); stage 1: per-element loss, d/dx_i, partial sums of the loss
// and of (sigmoid - target); stage 2: finishes -- loss, and d/d(other_j) = -(1/n_other) * mean_i(sigmoid_i - target), the same for every j.
__global__ __launch_bounds__(256) void bce_rel_partial_kernel(const float* __restrict__ x, size_t n, const float* __restrict__ other_mean, float target,
                                                              float gscale, const float* __restrict__ gscale_dev, float* __restrict__ grad_x,
                                                              int accumulate_x, float* __restrict__ partial, float* __restrict__ partial_d) {
  __shared__ float sh[4];
  float s = 0.f, sd = 0.f;
  const float m = *other_mean;
  if (gscale_dev) gscale *= *gscale_dev;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float v = x[i] - m;
    s += fmaxf(v, 0.f) - v * target + log1pf(expf(-fabsf(v)));
    const float d = 1.f / (1.f + expf(-v)) - target;
    sd += d;
    if (grad_x) grad_x[i] = (accumulate_x ? grad_x[i] : 0.f) + d * gscale;
  }
  store_block_sum(s, sh, partial);
  store_block_sum(sd, sh, partial_d);
}
// grad_other[j] (+)= -gscale * sum_d / n_other for every j (gscale already carries weight / n_x)
__global__ __launch_bounds__(256) void bce_rel_other_kernel(const float* __restrict__ partial_d, int nblk, float gscale, const float* __restrict__ gscale_dev,
                                                            float* __restrict__ grad_other, size_t n_other, int accumulate) {
  __shared__ float sh[4];
  __shared__ float tot;
  const float r = sum_partials(partial_d, nblk, sh);      // every block re-reduces the (<= 1024) partials: same order, same value
  if (threadIdx.x == 0) tot = r;
  __syncthreads();
  if (gscale_dev) gscale *= *gscale_dev;
  const float g = -gscale * tot / (float)n_other;
  grid_stride(n_other, [&](size_t j) { grad_other[j] = (accumulate ? grad_other[j] : 0.f) + g; });
}

// flag = 1 if any element of x is inf or NaN (the found_inf of torch.cuda.amp.GradScaler.unscale_, train_bsrgan.py:436,466)
__global__ __launch_bounds__(256) void nonfinite_flag_kernel(const float* __restrict__ x, size_t n, float* __restrict__ flag) {
  bool bad = false;
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const f32x4 v = ((const f32x4*)x)[i];
    bad |= !(fabsf(v[0]) <= 3.402823466e38f) | !(fabsf(v[1]) <= 3.402823466e38f) | !(fabsf(v[2]) <= 3.402823466e38f) | !(fabsf(v[3]) <= 3.402823466e38f);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) bad |= !(fabsf(x[n4 * 4 + threadIdx.x]) <= 3.402823466e38f);
  if (__any(bad) && (threadIdx.x & 63) == 0) *flag = 1.f;      // every writer stores the same value
}

// torch.amp.GradScaler.update() (torch/amp/grad_scaler.py, _amp_update_scale_) on a device-resident state, so that neither the host nor a
// captured graph ever carries a stale scale: state = {scale, 1 / scale, growth tracker, optimizer steps, skipped steps}.  The three
// counters are int32 words of the same 8-word state (a float stops counting at 2^24 steps; torch's tracker is an int32 tensor too).
__global__ void loss_scale_update_kernel(float* __restrict__ st, const float* __restrict__ found_inf, float growth, float backoff, int interval) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int* sti = reinterpret_cast<int*>(st);
  float scale = st[0];
  int tracker = sti[2];
  sti[3] += 1;
  if (*found_inf != 0.f) {
    scale *= backoff; tracker = 0; sti[4] += 1;
  } else {
    tracker += 1;
    if (tracker >= interval) {
      const float grown = scale * growth;
      if (fabsf(grown) <= 3.402823466e38f) scale = grown;       // torch keeps the scale when growing it would overflow
      tracker = 0;
    }
  }
  st[0] = scale; st[1] = 1.f / scale; sti[2] = tracker;
}

// ------------------------------------------------------------------------------------------------
extern "C" int srganfd_l1_loss(const float* a, const float* b, int64_t numel, float weight, float* out, int32_t accumulate, float* grad, float grad_scale,
                               const float* grad_scale_dev, float* ws, void* stream) {
  const size_t n = (size_t)numel;
  const hipStream_t s = (hipStream_t)stream;
  if (!a || !b || !out || !ws) return set_err(SRGANFD_EINVAL, "l1_loss: bad args");
  if (numel <= 0) return set_err(SRGANFD_EINVAL, "l1_loss: numel <= 0");
  const unsigned g = grid_for(n, 256, kRedBlocks);
  SRGANFD_LAUNCH(l1_partial_kernel, dim3(g), dim3(256), 0, s, a, b, n, grad_scale / (float)n, grad_scale_dev, grad, ws);
  SRGANFD_LAUNCH(finish_kernel<FinAxpy>, dim3(1), dim3(256), 0, s, FinAxpy{{ws, (int)g, weight / (float)n, out}, accumulate});
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_l1_loss_views(srganfd_view a, srganfd_view b, int32_t dtype, int64_t npix64, int32_t c, int32_t relu, float weight, float* out,
                                     int32_t accumulate, float* ws, void* stream) {
  const size_t npix = (size_t)npix64;
  const hipStream_t s = (hipStream_t)stream;
  if (!a.ptr || !b.ptr || !out || !ws) return set_err(SRGANFD_EINVAL, "l1_views: bad args");
  if (const char* why = views_bad(npix64, c, {a, b})) return set_err(SRGANFD_EINVAL, "l1_views: %s", why);      // npix * c == 0 would store weight / 0 * 0 = NaN
  const size_t n = npix * c;
  const unsigned g = grid_for(n, 256, kRedBlocks);
  const L1K k = {dev_view(a), dev_view(b), {}, npix, c, relu, ws, nullptr, 0.f};
  DISPATCH_TN(dtype, vec_ok(dtype, c, {a, b}), SRGANFD_LAUNCH((l1_views_partial_kernel<TT, NN>), dim3(g), dim3(256), 0, s, k));
  SRGANFD_LAUNCH(finish_kernel<FinAxpy>, dim3(1), dim3(256), 0, s, FinAxpy{{ws, (int)g, weight / (float)n, out}, accumulate});
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_l1_grad_views(srganfd_view a, srganfd_view b, srganfd_view out, int32_t dtype, int64_t npix64, int32_t c, const float* upstream,
                                     float scale, void* stream) {
  const size_t npix = (size_t)npix64;
  const hipStream_t s = (hipStream_t)stream;
  if (!a.ptr || !b.ptr || !out.ptr) return set_err(SRGANFD_EINVAL, "l1_grad_views: bad args");
  if (const char* why = views_bad(npix64, c, {a, b, out})) return set_err(SRGANFD_EINVAL, "l1_grad_views: %s", why);
  const L1K k = {dev_view(a), dev_view(b), dev_view(out), npix, c, 0, nullptr, upstream, scale};
  DISPATCH_T(dtype, SRGANFD_LAUNCH(l1_grad_views_kernel<TT>, dim3(grid_for(npix * c)), dim3(256), 0, s, k));
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_bce_logits(const float* x, int64_t numel, float target, float weight, float* loss_out, int32_t accumulate, float* sig_mean_out,
                                  float* grad, float grad_scale, const float* grad_scale_dev, float* ws, void* stream) {
  const size_t n = (size_t)numel;
  const hipStream_t s = (hipStream_t)stream;
  if (!x || !loss_out || !ws) return set_err(SRGANFD_EINVAL, "bce: bad args");
  if (numel <= 0) return set_err(SRGANFD_EINVAL, "bce: numel <= 0");
  const unsigned g = grid_for(n, 256, kRedBlocks);
  SRGANFD_LAUNCH(bce_partial_kernel, dim3(g), dim3(256), 0, s, x, n, target, grad_scale / (float)n, grad_scale_dev, grad, ws, ws + kRedBlocks);
  SRGANFD_LAUNCH(finish_kernel<FinAxpy>, dim3(1), dim3(256), 0, s, FinAxpy{{ws, (int)g, weight / (float)n, loss_out}, accumulate});
  if (sig_mean_out) SRGANFD_LAUNCH(finish_kernel<FinAxpy>, dim3(1), dim3(256), 0, s, FinAxpy{{ws + kRedBlocks, (int)g, 1.f / (float)n, sig_mean_out}, 0});
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_sigmoid_of_mean(const float* x, int64_t numel, float* out, float* ws, void* stream) {
  const size_t n = numel > 0 ? (size_t)numel : 0;
  const hipStream_t s = (hipStream_t)stream;
  if (!x || !out || !ws || n == 0) return set_err(SRGANFD_EINVAL, "sigmoid_of_mean: bad args");
  const unsigned g = grid_for(n, 256, kRedBlocks);
  SRGANFD_LAUNCH(sum_partial_kernel, dim3(g), dim3(256), 0, s, x, n, ws);
  SRGANFD_LAUNCH(finish_kernel<FinSigmoidMean>, dim3(1), dim3(256), 0, s, FinSigmoidMean{{ws, (int)g, 1.f / (float)n, out}});
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
// workspace: 2 * kRedBlocks + 1 floats (SRGANFD_LOSS_WS_FLOATS)
extern "C" int srganfd_bce_logits_relativistic(const float* x, int64_t numel, const float* other, int64_t numel_other, float target, float weight,
                                               float* loss_out, int32_t accumulate, float* grad_x, int32_t accumulate_x, float* grad_other,
                                               int32_t accumulate_other, float grad_scale, const float* grad_scale_dev, float* ws, void* stream) {
  const size_t n = numel > 0 ? (size_t)numel : 0, n_other = numel_other > 0 ? (size_t)numel_other : 0;
  const hipStream_t s = (hipStream_t)stream;
  if (!x || !other || !loss_out || !ws || n == 0 || n_other == 0) return set_err(SRGANFD_EINVAL, "bce_relativistic: bad args");
  float* mean = ws + 2 * kRedBlocks;
  const unsigned go = grid_for(n_other, 256, kRedBlocks), g = grid_for(n, 256, kRedBlocks);
  SRGANFD_LAUNCH(sum_partial_kernel, dim3(go), dim3(256), 0, s, other, n_other, ws);
  SRGANFD_LAUNCH(finish_kernel<FinMean>, dim3(1), dim3(256), 0, s, FinMean{{ws, (int)go, 1.f / (float)n_other, mean}});
  SRGANFD_LAUNCH(bce_rel_partial_kernel, dim3(g), dim3(256), 0, s, x, n, (const float*)mean, target, grad_scale / (float)n, grad_scale_dev, grad_x,
                 accumulate_x, ws, ws + kRedBlocks);
  SRGANFD_LAUNCH(finish_kernel<FinAxpy>, dim3(1), dim3(256), 0, s, FinAxpy{{ws, (int)g, weight / (float)n, loss_out}, accumulate});
  if (grad_other)
    SRGANFD_LAUNCH(bce_rel_other_kernel, dim3(grid_for(n_other, 256, 256)), dim3(256), 0, s, (const float*)(ws + kRedBlocks), (int)g, grad_scale / (float)n,
                   grad_scale_dev, grad_other, n_other, accumulate_other);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_nonfinite_flag(const float* x, int64_t numel, float* flag, int32_t accumulate, void* stream) {
  const size_t n = (size_t)numel;
  const hipStream_t s = (hipStream_t)stream;
  if (!x || !flag || ((uintptr_t)x & 15)) return set_err(SRGANFD_EINVAL, "nonfinite_flag: bad args");
  if (numel <= 0) return set_err(SRGANFD_EINVAL, "nonfinite_flag: numel <= 0");
  if (!accumulate) SRGANFD_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(float), s));
  SRGANFD_LAUNCH(nonfinite_flag_kernel, dim3(grid_for(n / 4 + 1, 256, 2048)), dim3(256), 0, s, x, n, flag);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_loss_scale_update(float* state, const float* found_inf, float growth, float backoff, int32_t interval, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!state || !found_inf || interval < 1 || !(growth >= 1.f) || !(backoff > 0.f && backoff <= 1.f)) return set_err(SRGANFD_EINVAL, "loss_scale_update: bad args");
  SRGANFD_LAUNCH(loss_scale_update_kernel, dim3(1), dim3(64), 0, s, state, found_inf, growth, backoff, interval);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

}  // namespace srganfd
