// norm.hip -- the normalisations: spectral norm (power iteration, sigma) and its gradient, single and batched over layers;
// BatchNorm2d forward / backward with the fused LeakyReLU and the two-phase data-parallel (SyncBN) forms; the per-channel affine map.
#include "elementwise.hpp"

namespace srganfd {

// ---- spectral norm (torch/nn/utils/spectral_norm.py:62-114 as applied at model.py:104-132) ----
// W is (rows=Cout, cols=Cin*k*k) row-major fp32.
// W^T u in row chunks of kSnRows: block (x, y) sums rows [y*kSnRows, ...) of 256 columns into part[y][k]; the normalise kernel adds the
// chunks in order (deterministic).  One thread per column over ALL rows left the chip with <= 18 workgroups for 71 us per layer.
static constexpr int kSnRows = 32;
// Up to kSnBatch layers per launch (blockIdx.z / .y picks the layer): eight layers x four dependent 5-14 us kernels are launch latency,
// not work.  Every layer is summed exactly as in a launch of its own, so batching does not change a bit.
static constexpr int kSnBatch = SRGANFD_SN_BATCH;
struct SnJobs { srganfd_sn_job j[kSnBatch]; };
__global__ __launch_bounds__(256) void sn_wt_u_kernel(const SnJobs jobs) {
  const srganfd_sn_job& J = jobs.j[blockIdx.z];
  const int rows = J.rows, cols = J.cols;
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int r0 = blockIdx.y * kSnRows, r1 = min(rows, r0 + kSnRows);
  if (k >= cols || r0 >= rows) return;
  const float* __restrict__ W = J.w_orig; const float* __restrict__ u = J.u;
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += W[(size_t)r * cols + k] * u[r];
  J.workspace[(size_t)blockIdx.y * cols + k] = s;
}
__global__ __launch_bounds__(1024) void sn_normalize_kernel(const SnJobs jobs, float eps) {
  __shared__ float sh[16];
  __shared__ float inv;
  const srganfd_sn_job& J = jobs.j[blockIdx.x];
  const int n = J.cols, nparts = (J.rows + kSnRows - 1) / kSnRows;
  const float* __restrict__ part = J.workspace; float* __restrict__ out = J.v;
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 1024) {
    float v = 0.f;
    for (int p = 0; p < nparts; ++p) v += part[(size_t)p * n + i];
    out[i] = v;                      // raw W^T u, scaled in place below
    s += v * v;
  }
  const float r = block_reduce_sum(s, sh);
  if (threadIdx.x == 0) inv = 1.f / fmaxf(sqrtf(r), eps);
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 1024) out[i] *= inv;
}
__device__ __forceinline__ float* sn_t(const srganfd_sn_job& J) { return J.workspace + (size_t)((J.rows + kSnRows - 1) / kSnRows) * J.cols; }
__global__ __launch_bounds__(256) void sn_w_v_kernel(const SnJobs jobs) {
  __shared__ float sh[4];
  const srganfd_sn_job& J = jobs.j[blockIdx.y];
  const int r = blockIdx.x, cols = J.cols;
  if (r >= J.rows) return;
  const float* __restrict__ W = J.w_orig; const float* __restrict__ v = J.v;
  float s = 0.f;
  for (int k = threadIdx.x; k < cols; k += 256) s += W[(size_t)r * cols + k] * v[k];
  const float tot = block_reduce_sum(s, sh);
  if (threadIdx.x == 0) sn_t(J)[r] = tot;
}
// u = normalize(t) (only if update_u), sigma = u . t, inv_sigma = 1/sigma
__global__ __launch_bounds__(256) void sn_finish_kernel(const SnJobs jobs, float eps, int update_u) {
  __shared__ float sh[4];
  __shared__ float inv;
  const srganfd_sn_job& J = jobs.j[blockIdx.x];
  const int rows = J.rows;
  const float* __restrict__ t = sn_t(J); float* __restrict__ u = J.u;
  float s = 0.f;
  if (update_u) {
    for (int i = threadIdx.x; i < rows; i += 256) s += t[i] * t[i];
    const float r = block_reduce_sum(s, sh);
    if (threadIdx.x == 0) inv = 1.f / fmaxf(sqrtf(r), eps);
    __syncthreads();
    for (int i = threadIdx.x; i < rows; i += 256) u[i] = t[i] * inv;
    __syncthreads();
  }
  s = 0.f;
  for (int i = threadIdx.x; i < rows; i += 256) s += u[i] * t[i];
  const float sig = block_reduce_sum(s, sh);
  if (threadIdx.x == 0) { *J.sigma_out = sig; *J.inv_sigma_out = 1.f / sig; }
}
// gradient through weight = W_orig / sigma, sigma = u^T W_orig v (u, v constants):
//   dW_orig = (G - <G, W_orig>/sigma * u v^T) / sigma        with G = dL/d(weight)
// Batched like the forward kernels: blockIdx.y picks the layer; every layer keeps the grid (number of partial sums, element stride) a
// launch of its own would have, so the sums are bit-identical.  kSnGradBlocks = the loss entry points' kRedBlocks.
static constexpr int kSnGradBlocks = 1024;
struct SnGradJobs { srganfd_sn_grad_job j[kSnBatch]; };
__device__ __forceinline__ unsigned sn_grad_blocks(size_t n) { const size_t g = (n + 255) / 256; return (unsigned)(g < 1 ? 1 : (g > kSnGradBlocks ? kSnGradBlocks : g)); }
__global__ __launch_bounds__(256) void sn_dot_partial_kernel(const SnGradJobs jobs) {
  __shared__ float sh[4];
  const srganfd_sn_grad_job& J = jobs.j[blockIdx.y];
  const size_t n = (size_t)J.rows * J.cols;
  const unsigned g = sn_grad_blocks(n);
  if (blockIdx.x >= g) return;
  const float* __restrict__ G = J.g_weight; const float* __restrict__ W = J.w_orig;
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)g * 256) s += G[i] * W[i];
  const float r = block_reduce_sum(s, sh);
  if (threadIdx.x == 0) J.workspace[blockIdx.x] = r;
}
__global__ __launch_bounds__(256) void sn_dot_finish_kernel(const SnGradJobs jobs) {
  __shared__ float sh[4];
  const srganfd_sn_grad_job& J = jobs.j[blockIdx.x];
  const int nblk = (int)sn_grad_blocks((size_t)J.rows * J.cols);
  float s = 0.f;
  for (int i = threadIdx.x; i < nblk; i += 256) s += J.workspace[i];
  const float r = block_reduce_sum(s, sh);
  if (threadIdx.x == 0) J.workspace[kSnGradBlocks] = 0.f + r * 1.f;
}
__global__ __launch_bounds__(256) void sn_grad_kernel(const SnGradJobs jobs, float beta) {
  const srganfd_sn_grad_job& J = jobs.j[blockIdx.y];
  const int cols = J.cols;
  const size_t n = (size_t)J.rows * cols;
  const float* __restrict__ G = J.g_weight; const float* __restrict__ u = J.u; const float* __restrict__ v = J.v;
  float* __restrict__ dW = J.dw_orig;
  const float is = *J.inv_sigma, coef = J.workspace[kSnGradBlocks] * is;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int r = (int)(i / cols), k = (int)(i % cols);
    const float g = (G[i] - coef * u[r] * v[k]) * is;
    dW[i] = g + (beta != 0.f ? beta * dW[i] : 0.f);
  }
}

// BatchNorm2d.  Statistics: 16-byte loads, thread = one channel chunk, pixels strided over the grid (coalesced);
// each block writes partial[block][2][C]; the finish kernel (one 1024-thread block) reduces them in a fixed order
// (deterministic), turns them into mean / invstd / (scale, shift) and updates the running statistics.
template <typename T>
__global__ __launch_bounds__(256) void bn_partial_kernel(const void* __restrict__ x, int xC, int x0, const void* __restrict__ g, int gC, int g0,
                                                         const float* __restrict__ save, size_t npix, int c, float* __restrict__ partial,
                                                         const void* __restrict__ act, int actC, int act0, float act_slope) {
  // act (optional, backward only): output of the LeakyReLU that followed the BatchNorm; dy is scaled by its derivative
  // forward statistics (g == nullptr): sum x, sum x^2.  backward (g = dy): sum dy, sum dy * xhat (xhat from save)
  constexpr int N = VecN<T>::N;
  __shared__ float sh[2][256 * N];
  const int cv = c / N;                                 // 16-byte chunks per pixel (host: 256 % cv == 0)
  const int lanes = 256 / cv;                           // pixels per block pass
  const int chunk = threadIdx.x % cv, pl = threadIdx.x / cv, ch = chunk * N;
  float s0[N], s1[N], mean[N], invstd[N];
#pragma unroll
  for (int q = 0; q < N; ++q) {
    s0[q] = 0.f; s1[q] = 0.f;
    mean[q] = (g && save) ? save[ch + q] : 0.f;
    invstd[q] = (g && save) ? save[c + ch + q] : 1.f;
  }
  const size_t step = (size_t)gridDim.x * lanes;
  if (g) {
    for (size_t p = (size_t)blockIdx.x * lanes + pl; p < npix; p += step) {
      float xv[N], dv[N];
      ldv<T>(x, p * xC + x0 + ch, xv);
      ldv<T>(g, p * gC + g0 + ch, dv);
      if (act) {
        float av[N];
        ldv<T>(act, p * actC + act0 + ch, av);
#pragma unroll
        for (int q = 0; q < N; ++q) dv[q] *= av[q] > 0.f ? 1.f : act_slope;
      }
#pragma unroll
      for (int q = 0; q < N; ++q) { s0[q] += dv[q]; s1[q] += dv[q] * (xv[q] - mean[q]) * invstd[q]; }
    }
  } else {
    size_t p = (size_t)blockIdx.x * lanes + pl;
    for (; p + step < npix; p += 2 * step) {            // two loads in flight
      float xa[N], xb[N];
      ldv<T>(x, p * xC + x0 + ch, xa);
      ldv<T>(x, (p + step) * xC + x0 + ch, xb);
#pragma unroll
      for (int q = 0; q < N; ++q) { s0[q] += xa[q] + xb[q]; s1[q] += xa[q] * xa[q] + xb[q] * xb[q]; }
    }
    if (p < npix) {
      float xa[N];
      ldv<T>(x, p * xC + x0 + ch, xa);
#pragma unroll
      for (int q = 0; q < N; ++q) { s0[q] += xa[q]; s1[q] += xa[q] * xa[q]; }
    }
  }
#pragma unroll
  for (int q = 0; q < N; ++q) { sh[0][(pl * cv + chunk) * N + q] = s0[q]; sh[1][(pl * cv + chunk) * N + q] = s1[q]; }
  __syncthreads();
  if ((int)threadIdx.x < c) {
    float a0 = 0.f, a1 = 0.f;
    for (int l = 0; l < lanes; ++l) { a0 += sh[0][l * c + threadIdx.x]; a1 += sh[1][l * c + threadIdx.x]; }
    partial[((size_t)blockIdx.x * 2 + 0) * c + threadIdx.x] = a0;
    partial[((size_t)blockIdx.x * 2 + 1) * c + threadIdx.x] = a1;
  }
}
// sums partial[b][2][c] over b with all 1024 threads (fixed order), result in tot[2][256]
__device__ __forceinline__ void bn_reduce_partials(const float* __restrict__ partial, int nblk, int c, float (*tot)[256]) {
  __shared__ float sh[2][1024];
  const int ch = threadIdx.x % c, l = threadIdx.x / c, lanes = 1024 / c;
  float a0 = 0.f, a1 = 0.f;
  if (l < lanes) {
#pragma unroll 8
    for (int b = l; b < nblk; b += lanes) { a0 += partial[((size_t)b * 2 + 0) * c + ch]; a1 += partial[((size_t)b * 2 + 1) * c + ch]; }
  }
  sh[0][threadIdx.x] = a0; sh[1][threadIdx.x] = a1;
  __syncthreads();
  if ((int)threadIdx.x < c) {
    float t0 = 0.f, t1 = 0.f;
    for (int k = 0; k < lanes; ++k) { t0 += sh[0][k * c + threadIdx.x]; t1 += sh[1][k * c + threadIdx.x]; }
    tot[0][threadIdx.x] = t0; tot[1][threadIdx.x] = t1;
  }
  __syncthreads();
}
__global__ __launch_bounds__(1024) void bn_fwd_finish_kernel(const float* __restrict__ partial, int nblk, int c, float npix, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float* running_mean, float* running_var, float momentum, float eps,
                                                             int training, float* __restrict__ save) {
  __shared__ float tot[2][256];
  if (training) bn_reduce_partials(partial, nblk, c, tot);
  const int ch = threadIdx.x;
  if (ch >= c) return;
  float mean, var;
  if (training) {
    mean = tot[0][ch] / npix;
    var = fmaxf(tot[1][ch] / npix - mean * mean, 0.f);
    running_mean[ch] = (1.f - momentum) * running_mean[ch] + momentum * mean;
    running_var[ch] = (1.f - momentum) * running_var[ch] + momentum * var * (npix / (npix - 1.f));
  } else {
    mean = running_mean[ch]; var = running_var[ch];
  }
  const float invstd = rsqrtf(var + eps);
  const float sc = gamma[ch] * invstd;
  save[ch] = mean; save[c + ch] = invstd; save[2 * c + ch] = sc; save[3 * c + ch] = beta[ch] - mean * sc;
}
// dx = dy*A + x*B + C0 per channel; coefficient triple + parameter gradients from the partial sums
// partial_global (data-parallel SyncBN, else NULL): the same table summed over the ranks.  The parameter gradients are this rank's
// sums (the flat-gradient all-reduce adds the ranks later); the dx coefficients use the sums and the pixel count of the whole batch.
__global__ __launch_bounds__(1024) void bn_bwd_finish_kernel(const float* __restrict__ partial, int nblk, int c, float npix, const float* __restrict__ gamma,
                                                             const float* __restrict__ save, float* dgamma, float* dbeta, float acc, float* __restrict__ coef,
                                                             const float* __restrict__ partial_global) {
  __shared__ float tot[2][256];
  bn_reduce_partials(partial, nblk, c, tot);
  const int ch = threadIdx.x;
  float db = 0.f, dg = 0.f;
  if (ch < c) {
    db = tot[0][ch]; dg = tot[1][ch];
    dgamma[ch] = dg + (acc != 0.f ? acc * dgamma[ch] : 0.f);
    dbeta[ch] = db + (acc != 0.f ? acc * dbeta[ch] : 0.f);
  }
  if (partial_global) {
    __syncthreads();
    bn_reduce_partials(partial_global, nblk, c, tot);
    if (ch < c) { db = tot[0][ch]; dg = tot[1][ch]; }
  }
  if (ch >= c) return;
  const float mean = save[ch], invstd = save[c + ch], gi = gamma[ch] * invstd;
  coef[ch] = gi;                                              // A
  coef[c + ch] = -gi * invstd * dg / npix;                    // B
  coef[2 * c + ch] = gi * (-db / npix + mean * invstd * dg / npix);  // C0
}
// out = a*ca[c] + b*cb[c] + c0[c]  (b, cb optional): BatchNorm apply (forward: a=x, ca=scale, c0=shift) and backward.
// Thread = one fixed channel chunk (coefficients live in registers), pixels strided over the grid.
template <typename T>
__global__ __launch_bounds__(256) void chan_affine_kernel(const void* __restrict__ a, int aC, int a0, const void* __restrict__ b, int bC, int b0,
                                                          void* out, int oC, int o0, const float* __restrict__ ca, const float* __restrict__ cb,
                                                          const float* __restrict__ c0, size_t npix, int c, float post_slope,
                                                          const void* __restrict__ act, int actC, int act0, float act_slope) {
  // post_slope: LeakyReLU applied to the result (1 = none).  act (optional): `a` is scaled by LeakyReLU'(act) first.
  constexpr int N = VecN<T>::N;
  const int cv = c / N, lanes = 256 / cv;               // host: 256 % cv == 0
  const int ch = (threadIdx.x % cv) * N, pl = threadIdx.x / cv;
  float fa[N], fb[N], f0[N];
#pragma unroll
  for (int q = 0; q < N; ++q) { fa[q] = ca[ch + q]; fb[q] = b ? cb[ch + q] : 0.f; f0[q] = c0[ch + q]; }
  const size_t step = (size_t)gridDim.x * lanes;
  for (size_t p = (size_t)blockIdx.x * lanes + pl; p < npix; p += step) {
    float va[N], vb[N];
    ldv<T>(a, p * aC + a0 + ch, va);
    if (act) {
      ldv<T>(act, p * actC + act0 + ch, vb);
#pragma unroll
      for (int q = 0; q < N; ++q) va[q] *= vb[q] > 0.f ? 1.f : act_slope;
    }
    if (b) {
      ldv<T>(b, p * bC + b0 + ch, vb);
#pragma unroll
      for (int q = 0; q < N; ++q) va[q] = va[q] * fa[q] + vb[q] * fb[q] + f0[q];
    } else {
#pragma unroll
      for (int q = 0; q < N; ++q) va[q] = va[q] * fa[q] + f0[q];
    }
    if (post_slope != 1.f) {
#pragma unroll
      for (int q = 0; q < N; ++q) va[q] = va[q] > 0.f ? va[q] : va[q] * post_slope;
    }
    stv<T>(out, p * oC + o0 + ch, va);
  }
}

// ------------------------------------------------------------------------------------------------
// each job's workspace: ceil(rows / 32) * cols + rows floats
extern "C" int srganfd_spectral_norm_batch(const srganfd_sn_job* jobs, int32_t njobs, int32_t training, float eps, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!jobs || njobs <= 0) return set_err(SRGANFD_EINVAL, "spectral_norm: no jobs");
  for (int b = 0; b < njobs; b += kSnBatch) {
    const int nb = std::min(kSnBatch, njobs - b);
    SnJobs J;
    int max_rows = 0, max_cols = 0;
    for (int i = 0; i < nb; ++i) {
      const srganfd_sn_job& q = jobs[b + i];
      if (!q.w_orig || !q.u || !q.v || !q.sigma_out || !q.inv_sigma_out || !q.workspace || q.rows <= 0 || q.cols <= 0)
        return set_err(SRGANFD_EINVAL, "spectral_norm: bad args");
      J.j[i] = q; max_rows = std::max(max_rows, q.rows); max_cols = std::max(max_cols, q.cols);
    }
    for (int i = nb; i < kSnBatch; ++i) J.j[i] = J.j[0];            // never indexed: the grids stop at nb
    if (training) {
      SRGANFD_LAUNCH(sn_wt_u_kernel, dim3((max_cols + 255) / 256, (max_rows + kSnRows - 1) / kSnRows, nb), dim3(256), 0, s, J);
      SRGANFD_LAUNCH(sn_normalize_kernel, dim3(nb), dim3(1024), 0, s, J, eps);
    }
    SRGANFD_LAUNCH(sn_w_v_kernel, dim3(max_rows, nb), dim3(256), 0, s, J);
    SRGANFD_LAUNCH(sn_finish_kernel, dim3(nb), dim3(256), 0, s, J, eps, training);
  }
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_spectral_norm(const float* W, float* u, float* v, int32_t rows, int32_t cols, int32_t training, float eps, float* sigma, float* inv_sigma,
                                     float* ws, void* stream) {
  srganfd_sn_job q;
  q.w_orig = W; q.u = u; q.v = v; q.sigma_out = sigma; q.inv_sigma_out = inv_sigma; q.workspace = ws; q.rows = rows; q.cols = cols;
  return srganfd_spectral_norm_batch(&q, 1, training, eps, stream);
}
// each job's workspace: kRedBlocks + 1 floats
extern "C" int srganfd_spectral_norm_grad_batch(const srganfd_sn_grad_job* jobs, int32_t njobs, float beta, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  static_assert(kSnGradBlocks == kRedBlocks, "workspace contract of srganfd_spectral_norm_grad");
  if (!jobs || njobs <= 0) return set_err(SRGANFD_EINVAL, "spectral_norm_grad: no jobs");
  for (int b = 0; b < njobs; b += kSnBatch) {
    const int nb = std::min(kSnBatch, njobs - b);
    SnGradJobs J;
    size_t max_n = 0;
    for (int i = 0; i < nb; ++i) {
      const srganfd_sn_grad_job& q = jobs[b + i];
      if (!q.g_weight || !q.w_orig || !q.u || !q.v || !q.inv_sigma || !q.dw_orig || !q.workspace || q.rows <= 0 || q.cols <= 0)
        return set_err(SRGANFD_EINVAL, "spectral_norm_grad: bad args");
      J.j[i] = q; max_n = std::max(max_n, (size_t)q.rows * q.cols);
    }
    for (int i = nb; i < kSnBatch; ++i) J.j[i] = J.j[0];
    SRGANFD_LAUNCH(sn_dot_partial_kernel, dim3(grid_for(max_n, 256, kRedBlocks), nb), dim3(256), 0, s, J);
    SRGANFD_LAUNCH(sn_dot_finish_kernel, dim3(nb), dim3(256), 0, s, J);
    SRGANFD_LAUNCH(sn_grad_kernel, dim3(grid_for(max_n), nb), dim3(256), 0, s, J, beta);
  }
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_spectral_norm_grad(const float* G, const float* W, const float* u, const float* v, const float* inv_sigma, float* dW, int32_t rows,
                                          int32_t cols, float beta, float* ws, void* stream) {
  srganfd_sn_grad_job q;
  q.g_weight = G; q.w_orig = W; q.u = u; q.v = v; q.inv_sigma = inv_sigma; q.dw_orig = dW; q.workspace = ws; q.rows = rows; q.cols = cols;
  return srganfd_spectral_norm_grad_batch(&q, 1, beta, stream);
}

static constexpr int kBnBlocks = 1024;  // workspace: kBnBlocks * 2 * c floats (+ 3c for the backward coefficients)
extern "C" int64_t srganfd_batchnorm_partial_floats(int32_t c) { return (long long)kBnBlocks * 2 * c; }
static inline bool bn_chunks_ok(int dtype, int c) { const int cv = c / (dtype == SRGANFD_F32 ? 4 : 8); return cv > 0 && 256 % cv == 0; }
// every channel block of <= 256, checked before the first launch: a refused call has written nothing.  Returns the bad block's size or 0.
static inline int bn_bad_block(int dtype, int c) {
  for (int cb = 0; cb < c; cb += 256) {
    const int cc = c - cb < 256 ? c - cb : 256;
    if (!bn_chunks_ok(dtype, cc)) return cc;
  }
  return 0;
}
static inline unsigned bn_grid(size_t npix, int dtype, int c) { const int lanes = 256 / (c / (dtype == SRGANFD_F32 ? 4 : 8)); return grid_for((npix + lanes - 1) / lanes, 1, 16384); }
// Channels are processed in blocks of <= 256 (the statistics kernels map one thread to one channel); `save` is
// [block][mean | invstd | scale | shift] and is only read back by batchnorm_bwd_impl with the same blocking.
// phase (data-parallel SyncBN): 0 = statistics, finish and apply in one call; 1 = this rank's partial sums into ws only (the caller
// all-reduces the first batchnorm_partial_floats(c) floats of ws over the ranks); 2 = finish + apply from ws with total_npix pixels.
// Shared by the three forward entry points (plain, fused activation, two-phase).
static int batchnorm_fwd_impl(srganfd_view x, srganfd_view y, int dtype, size_t npix, int c, const float* gamma, const float* beta, float* rm, float* rv,
                              float momentum, float eps, int training, float* save, float* ws, float act_slope, hipStream_t s, int phase,
                              size_t total_npix) {
  if (!x.ptr || !y.ptr || !gamma || !beta || !rm || !rv || !save || !ws || c <= 0 || !vec_ok(dtype, c, {x, y}))
    return set_err(SRGANFD_EINVAL, "batchnorm_fwd: bad args (16-byte aligned views)");
  if (const char* why = views_bad(c, {x, y})) return set_err(SRGANFD_EINVAL, "batchnorm_fwd: %s", why);
  if (phase && (c > 256 || !training)) return set_err(SRGANFD_EINVAL, "batchnorm_fwd: the two-phase form takes training mode and at most 256 channels");
  if (const int bad = bn_bad_block(dtype, c)) return set_err(SRGANFD_EINVAL, "batchnorm_fwd: channel block of %d is not a power-of-two number of 16-byte chunks", bad);
  // the unbiased running variance is var * n / (n - 1): one value per channel has none (torch refuses it as well)
  if (training && phase != 1 && (phase == 2 ? total_npix : npix) < 2)
    return set_err(SRGANFD_EINVAL, "batchnorm_fwd: training mode needs more than one value per channel (npix = %lld)", (long long)(phase == 2 ? total_npix : npix));
  const float count = (float)(phase == 2 ? total_npix : npix);
  for (int cb = 0; cb < c; cb += 256) {
    const int cc = c - cb < 256 ? c - cb : 256;
    const srganfd_view xs = sub_view(x, cb), ys = sub_view(y, cb);
    float* sv = save + 4 * cb;
    if (training && phase != 2) {
      DISPATCH_T(dtype,
                 SRGANFD_LAUNCH(bn_partial_kernel<TT>, dim3(kBnBlocks), dim3(256), 0, s, xs.ptr, xs.cstride, xs.c0, (const void*)nullptr, 0, 0, (const float*)nullptr, npix, cc, ws, (const void*)nullptr, 0, 0, 1.f));
    }
    if (phase == 1) continue;
    SRGANFD_LAUNCH(bn_fwd_finish_kernel, dim3(1), dim3(1024), 0, s, (const float*)ws, kBnBlocks, cc, count, gamma + cb, beta + cb, rm + cb, rv + cb, momentum, eps, training, sv);
    DISPATCH_T(dtype,
               SRGANFD_LAUNCH(chan_affine_kernel<TT>, dim3(bn_grid(npix, dtype, cc)), dim3(256), 0, s, xs.ptr, xs.cstride, xs.c0, (const void*)nullptr, 0, 0,
                              ys.ptr, ys.cstride, ys.c0, (const float*)(sv + 2 * cc), (const float*)nullptr, (const float*)(sv + 3 * cc), npix, cc, act_slope, (const void*)nullptr, 0, 0, 1.f));
  }
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
// phase as in batchnorm_fwd_impl; phase 2 takes ws_global = the partial table summed over the ranks (ws keeps this rank's own)
static int batchnorm_bwd_impl(srganfd_view x, srganfd_view dy, srganfd_view dx, int dtype, size_t npix, int c, const float* gamma, const float* save,
                              float* dgamma, float* dbeta, float acc, float* ws, srganfd_view act, float act_slope, hipStream_t s, int phase,
                              const float* ws_global, size_t total_npix) {
  if (!x.ptr || !dy.ptr || !dx.ptr || !gamma || !save || !dgamma || !dbeta || !ws || c <= 0 || !vec_ok(dtype, c, {x, dy, dx, act}))
    return set_err(SRGANFD_EINVAL, "batchnorm_bwd: bad args");
  if (const char* why = views_bad(c, {x, dy, dx, act})) return set_err(SRGANFD_EINVAL, "batchnorm_bwd: %s", why);
  if (phase && c > 256) return set_err(SRGANFD_EINVAL, "batchnorm_bwd: the two-phase form takes at most 256 channels");
  if (phase == 2 && !ws_global) return set_err(SRGANFD_EINVAL, "batchnorm_bwd: phase 2 needs the all-reduced table");
  if (const int bad = bn_bad_block(dtype, c)) return set_err(SRGANFD_EINVAL, "batchnorm_bwd: channel block of %d is not a power-of-two number of 16-byte chunks", bad);
  const float count = (float)(phase == 2 ? total_npix : npix);
  for (int cb = 0; cb < c; cb += 256) {
    const int cc = c - cb < 256 ? c - cb : 256;
    const srganfd_view xs = sub_view(x, cb), dys = sub_view(dy, cb), dxs = sub_view(dx, cb), as = sub_view(act, cb);
    const float* sv = save + 4 * cb;
    float* coef = ws + (size_t)kBnBlocks * 2 * cc;
    if (phase != 2) {
      DISPATCH_T(dtype,
                 SRGANFD_LAUNCH(bn_partial_kernel<TT>, dim3(kBnBlocks), dim3(256), 0, s, xs.ptr, xs.cstride, xs.c0, (const void*)dys.ptr, dys.cstride, dys.c0, sv, npix, cc, ws, (const void*)as.ptr, as.cstride, as.c0, act_slope));
    }
    if (phase == 1) continue;
    SRGANFD_LAUNCH(bn_bwd_finish_kernel, dim3(1), dim3(1024), 0, s, (const float*)ws, kBnBlocks, cc, count, gamma + cb, sv, dgamma + cb, dbeta + cb, acc, coef,
                   phase == 2 ? ws_global : (const float*)nullptr);
    DISPATCH_T(dtype,
               SRGANFD_LAUNCH(chan_affine_kernel<TT>, dim3(bn_grid(npix, dtype, cc)), dim3(256), 0, s, dys.ptr, dys.cstride, dys.c0, (const void*)xs.ptr, xs.cstride, xs.c0,
                              dxs.ptr, dxs.cstride, dxs.c0, (const float*)coef, (const float*)(coef + cc), (const float*)(coef + 2 * cc), npix, cc, 1.f, (const void*)as.ptr, as.cstride, as.c0, act_slope));
  }
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_batchnorm_fwd(srganfd_view x, srganfd_view y, int32_t dtype, int64_t npix, int32_t c, const float* gamma, const float* beta,
                                     float* running_mean, float* running_var, float momentum, float eps, int32_t training, float* save, float* workspace,
                                     void* stream) {
  return batchnorm_fwd_impl(x, y, dtype, (size_t)npix, c, gamma, beta, running_mean, running_var, momentum, eps, training, save, workspace,
                            1.f, (hipStream_t)stream, 0, 0);
}
extern "C" int srganfd_batchnorm_act_fwd(srganfd_view x, srganfd_view y, int32_t dtype, int64_t npix, int32_t c, const float* gamma, const float* beta,
                                         float* running_mean, float* running_var, float momentum, float eps, int32_t training, float* save,
                                         float* workspace, float act_slope, void* stream) {
  return batchnorm_fwd_impl(x, y, dtype, (size_t)npix, c, gamma, beta, running_mean, running_var, momentum, eps, training, save, workspace,
                            act_slope, (hipStream_t)stream, 0, 0);
}
extern "C" int srganfd_batchnorm_fwd_sync(srganfd_view x, srganfd_view y, int32_t dtype, int64_t npix, int32_t c, const float* gamma, const float* beta,
                                          float* running_mean, float* running_var, float momentum, float eps, float* save, float* workspace,
                                          float act_slope, int32_t phase, int64_t total_npix, void* stream) {
  return batchnorm_fwd_impl(x, y, dtype, (size_t)npix, c, gamma, beta, running_mean, running_var, momentum, eps, 1, save, workspace, act_slope,
                            (hipStream_t)stream, phase, (size_t)total_npix);
}
extern "C" int srganfd_batchnorm_bwd_sync(srganfd_view x, srganfd_view dy, srganfd_view dx, int32_t dtype, int64_t npix, int32_t c, const float* gamma,
                                          const float* save, float* dgamma, float* dbeta, float acc, float* workspace, const float* workspace_global,
                                          srganfd_view act, float act_slope, int32_t phase, int64_t total_npix, void* stream) {
  return batchnorm_bwd_impl(x, dy, dx, dtype, (size_t)npix, c, gamma, save, dgamma, dbeta, acc, workspace, act, act_slope, (hipStream_t)stream, phase,
                            workspace_global, (size_t)total_npix);
}
extern "C" int srganfd_batchnorm_bwd(srganfd_view x, srganfd_view dy, srganfd_view dx, int32_t dtype, int64_t npix, int32_t c, const float* gamma,
                                     const float* save, float* dgamma, float* dbeta, float acc, float* workspace, void* stream) {
  srganfd_view none = {nullptr, 0, 0};
  return batchnorm_bwd_impl(x, dy, dx, dtype, (size_t)npix, c, gamma, save, dgamma, dbeta, acc, workspace, none, 1.f, (hipStream_t)stream, 0, nullptr, 0);
}
extern "C" int srganfd_batchnorm_act_bwd(srganfd_view x, srganfd_view dy, srganfd_view dx, int32_t dtype, int64_t npix, int32_t c, const float* gamma,
                                         const float* save, float* dgamma, float* dbeta, float acc, float* workspace, srganfd_view act,
                                         float act_slope, void* stream) {
  return batchnorm_bwd_impl(x, dy, dx, dtype, (size_t)npix, c, gamma, save, dgamma, dbeta, acc, workspace, act, act_slope, (hipStream_t)stream, 0, nullptr,
                            0);
}

}  // namespace srganfd
