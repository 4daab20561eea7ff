// norm.hip -- the normalisations: spectral norm (power iteration, sigma) and its gradient, single and batched over layers;
// BatchNorm2d forward / backward with the fused LeakyReLU and the two-phase data-parallel (SyncBN) forms; the per-channel affine map.
// The BatchNorm kernels take one struct of views and scalars each; the two directions share their refusals (bn_refuse) and the loop over
// channel blocks and phases (bn_blocks).
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
// finish_kernel's epilogue for <G, W_orig>: block b sums layer b's partials into workspace[kSnGradBlocks]  (0.f + r: a sum of -0 is stored as +0)
struct SnDotFin {
  SnGradJobs jobs;
  __device__ const srganfd_sn_grad_job& job() const { return jobs.j[blockIdx.x]; }
  __device__ const float* partial() const { return job().workspace; }
  __device__ int nblk() const { return (int)sn_grad_blocks((size_t)job().rows * job().cols); }
  __device__ void store(float r) const { job().workspace[kSnGradBlocks] = 0.f + r; }
};
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
struct BnPartialK { View x, g, act; const float* save; size_t npix; int c; float* partial; float act_slope; };
template <typename T>
__global__ __launch_bounds__(256) void bn_partial_kernel(const BnPartialK k) {
  // act (optional, backward only): output of the LeakyReLU that followed the BatchNorm; dy is scaled by its derivative
  // forward statistics (g absent): sum x, sum x^2.  backward (g = dy): sum dy, sum dy * xhat (xhat from save)
  const View &x = k.x, &g = k.g, &act = k.act;
  const float* __restrict__ save = k.save; float* __restrict__ partial = k.partial;
  const size_t npix = k.npix; const int c = k.c; const float act_slope = k.act_slope;
  constexpr int N = VecN<T>::N;
  __shared__ float sh[2][256 * N];
  const int cv = c / N;                                 // 16-byte chunks per pixel (host: 256 % cv == 0)
  const int lanes = 256 / cv;                           // pixels per block pass
  const int chunk = threadIdx.x % cv, pl = threadIdx.x / cv, ch = chunk * N;
  float s0[N], s1[N];
  each<N>([&](int q) { s0[q] = 0.f; s1[q] = 0.f; });
  const size_t step = (size_t)gridDim.x * lanes;
  if (g.p) {
    // the saved statistics, read under one guard: guarded per channel they cost a load and a wait each, or two more VGPRs than a wave step
    // allows (profiles/view_kernels_refactor_isa.txt)
    float mean[N], invstd[N];
    each<N>([&](int q) { mean[q] = 0.f; invstd[q] = 1.f; });
    if (save) each<N>([&](int q) { mean[q] = save[ch + q]; invstd[q] = save[c + ch + q]; });
    for (size_t p = (size_t)blockIdx.x * lanes + pl; p < npix; p += step) {
      float xv[N], dv[N];
      ldv<T>(x.p, x.at(p, ch), xv);
      ldv<T>(g.p, g.at(p, ch), dv);
      if (act.p) {
        float av[N];
        ldv<T>(act.p, act.at(p, ch), av);
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
      ldv<T>(x.p, x.at(p, ch), xa);
      ldv<T>(x.p, x.at(p + step, ch), xb);
#pragma unroll
      for (int q = 0; q < N; ++q) { s0[q] += xa[q] + xb[q]; s1[q] += xa[q] * xa[q] + xb[q] * xb[q]; }
    }
    if (p < npix) {
      float xa[N];
      ldv<T>(x.p, x.at(p, ch), xa);
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
struct AffineK { View a, b, out, act; const float *ca, *cb, *c0; size_t npix; int c; float post_slope, act_slope; };
template <typename T>
__global__ __launch_bounds__(256) void chan_affine_kernel(const AffineK k) {
  // post_slope: LeakyReLU applied to the result (1 = none).  act (optional): `a` is scaled by LeakyReLU'(act) first.
  const View &a = k.a, &b = k.b, &out = k.out, &act = k.act;
  const float* __restrict__ ca = k.ca; const float* __restrict__ cb = k.cb; const float* __restrict__ c0 = k.c0;
  const size_t npix = k.npix; const int c = k.c; const float post_slope = k.post_slope, act_slope = k.act_slope;
  constexpr int N = VecN<T>::N;
  const int cv = c / N, lanes = 256 / cv;               // host: 256 % cv == 0
  const int ch = (threadIdx.x % cv) * N, pl = threadIdx.x / cv;
  float fa[N], fb[N], f0[N];
#pragma unroll
  for (int q = 0; q < N; ++q) { fa[q] = ca[ch + q]; fb[q] = b.p ? cb[ch + q] : 0.f; f0[q] = c0[ch + q]; }
  const size_t step = (size_t)gridDim.x * lanes;
  for (size_t p = (size_t)blockIdx.x * lanes + pl; p < npix; p += step) {
    float va[N], vb[N];
    ldv<T>(a.p, a.at(p, ch), va);
    if (act.p) {
      ldv<T>(act.p, act.at(p, ch), vb);
#pragma unroll
      for (int q = 0; q < N; ++q) va[q] *= vb[q] > 0.f ? 1.f : act_slope;
    }
    if (b.p) {
      ldv<T>(b.p, b.at(p, ch), vb);
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
    stv<T>(out.p, out.at(p, ch), va);
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
    SRGANFD_LAUNCH(finish_kernel<SnDotFin>, dim3(nb), dim3(256), 0, s, SnDotFin{J});
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
static inline bool bn_chunks_ok(int dtype, int c) { const int cv = c / vec_width(dtype); return cv > 0 && 256 % cv == 0; }
// every channel block of <= 256, checked before the first launch: a refused call has written nothing.  Returns the bad block's size or 0.
static inline int bn_bad_block(int dtype, int c) {
  for (int cb = 0; cb < c; cb += 256) {
    const int cc = c - cb < 256 ? c - cb : 256;
    if (!bn_chunks_ok(dtype, cc)) return cc;
  }
  return 0;
}
static inline unsigned bn_grid(size_t npix, int dtype, int c) { const int lanes = 256 / (c / vec_width(dtype)); return grid_for((npix + lanes - 1) / lanes, 1, 16384); }
// Channels are processed in blocks of <= 256 (the statistics kernels map one thread to one channel); `save` is
// [block][mean | invstd | scale | shift], written by the forward pass and read back by the backward pass with the same blocking.
// phase (data-parallel SyncBN): 0 = statistics, finish and apply in one call; 1 = this rank's partial sums into ws only (the caller
// all-reduces the first batchnorm_partial_floats(c) floats of ws over the ranks); 2 = finish + apply from the summed table with total_npix
// pixels (backward: ws_global is that table, ws keeps this rank's own).
// What both directions refuse after their own null / alignment check (phase_why: the direction's own rule for the two-phase form, or NULL)
static int bn_refuse(const char* who, int dtype, int c, std::initializer_list<srganfd_view> views, const char* phase_why) {
  if (const char* why = views_bad(c, views)) return set_err(SRGANFD_EINVAL, "%s: %s", who, why);
  if (phase_why) return set_err(SRGANFD_EINVAL, "%s: %s", who, phase_why);
  if (const int bad = bn_bad_block(dtype, c)) return set_err(SRGANFD_EINVAL, "%s: channel block of %d is not a power-of-two number of 16-byte chunks", who, bad);
  return SRGANFD_OK;
}
// The block loop and the phases, once: stats(cb, cc) launches the partial sums of channels [cb, cb + cc) (not in phase 2, and not where
// the running statistics are used), apply(cb, cc) the finish kernel and the affine map (not in phase 1).  Both return an error code.
template <typename S, typename A>
static int bn_blocks(int c, int phase, bool want_stats, S stats, A apply) {
  for (int cb = 0; cb < c; cb += 256) {
    const int cc = c - cb < 256 ? c - cb : 256;
    if (want_stats && phase != 2)
      if (const int rc = stats(cb, cc)) return rc;
    if (phase == 1) continue;
    if (const int rc = apply(cb, cc)) return rc;
  }
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
// Shared by the three forward entry points (plain, fused activation, two-phase).
static int batchnorm_fwd_impl(srganfd_view x, srganfd_view y, int dtype, size_t npix, int c, const float* gamma, const float* beta, float* rm, float* rv,
                              float momentum, float eps, int training, float* save, float* ws, float act_slope, hipStream_t s, int phase,
                              size_t total_npix) {
  if (!x.ptr || !y.ptr || !gamma || !beta || !rm || !rv || !save || !ws || c <= 0 || !vec_ok(dtype, c, {x, y}))
    return set_err(SRGANFD_EINVAL, "batchnorm_fwd: bad args (16-byte aligned views)");
  if (const int rc = bn_refuse("batchnorm_fwd", dtype, c, {x, y},
                               phase && (c > 256 || !training) ? "the two-phase form takes training mode and at most 256 channels" : nullptr))
    return rc;
  // the unbiased running variance is var * n / (n - 1): one value per channel has none (torch refuses it as well)
  const size_t count = phase == 2 ? total_npix : npix;
  if (training && phase != 1 && count < 2)
    return set_err(SRGANFD_EINVAL, "batchnorm_fwd: training mode needs more than one value per channel (npix = %lld)", (long long)count);
  return bn_blocks(
      c, phase, training != 0,
      [&](int cb, int cc) {
        const BnPartialK k = {dev_view(sub_view(x, cb)), {}, {}, nullptr, npix, cc, ws, 1.f};
        DISPATCH_T(dtype, SRGANFD_LAUNCH(bn_partial_kernel<TT>, dim3(kBnBlocks), dim3(256), 0, s, k));
        return (int)SRGANFD_OK;
      },
      [&](int cb, int cc) {
        float* sv = save + 4 * cb;
        SRGANFD_LAUNCH(bn_fwd_finish_kernel, dim3(1), dim3(1024), 0, s, (const float*)ws, kBnBlocks, cc, (float)count, gamma + cb, beta + cb, rm + cb, rv + cb, momentum, eps, training, sv);
        const AffineK k = {dev_view(sub_view(x, cb)), {}, dev_view(sub_view(y, cb)), {}, sv + 2 * cc, nullptr, sv + 3 * cc, npix, cc, act_slope, 1.f};
        DISPATCH_T(dtype, SRGANFD_LAUNCH(chan_affine_kernel<TT>, dim3(bn_grid(npix, dtype, cc)), dim3(256), 0, s, k));
        return (int)SRGANFD_OK;
      });
}
// Shared by the three backward entry points.  act (optional): the output of the LeakyReLU fused into the forward pass.
static int batchnorm_bwd_impl(srganfd_view x, srganfd_view dy, srganfd_view dx, int dtype, size_t npix, int c, const float* gamma, const float* save,
                              float* dgamma, float* dbeta, float acc, float* ws, srganfd_view act, float act_slope, hipStream_t s, int phase,
                              const float* ws_global, size_t total_npix) {
  if (!x.ptr || !dy.ptr || !dx.ptr || !gamma || !save || !dgamma || !dbeta || !ws || c <= 0 || !vec_ok(dtype, c, {x, dy, dx, act}))
    return set_err(SRGANFD_EINVAL, "batchnorm_bwd: bad args");
  if (const int rc = bn_refuse("batchnorm_bwd", dtype, c, {x, dy, dx, act},
                               phase && c > 256 ? "the two-phase form takes at most 256 channels"
                                                : phase == 2 && !ws_global ? "phase 2 needs the all-reduced table" : nullptr))
    return rc;
  const float count = (float)(phase == 2 ? total_npix : npix);
  return bn_blocks(
      c, phase, true,
      [&](int cb, int cc) {
        const BnPartialK k = {dev_view(sub_view(x, cb)), dev_view(sub_view(dy, cb)), dev_view(sub_view(act, cb)), save + 4 * cb, npix, cc, ws, act_slope};
        DISPATCH_T(dtype, SRGANFD_LAUNCH(bn_partial_kernel<TT>, dim3(kBnBlocks), dim3(256), 0, s, k));
        return (int)SRGANFD_OK;
      },
      [&](int cb, int cc) {
        float* coef = ws + (size_t)kBnBlocks * 2 * cc;
        SRGANFD_LAUNCH(bn_bwd_finish_kernel, dim3(1), dim3(1024), 0, s, (const float*)ws, kBnBlocks, cc, count, gamma + cb, save + 4 * cb, dgamma + cb, dbeta + cb, acc, coef,
                       phase == 2 ? ws_global : (const float*)nullptr);
        const AffineK k = {dev_view(sub_view(dy, cb)), dev_view(sub_view(x, cb)), dev_view(sub_view(dx, cb)), dev_view(sub_view(act, cb)),
                           coef, coef + cc, coef + 2 * cc, npix, cc, 1.f, act_slope};
        DISPATCH_T(dtype, SRGANFD_LAUNCH(chan_affine_kernel<TT>, dim3(bn_grid(npix, dtype, cc)), dim3(256), 0, s, k));
        return (int)SRGANFD_OK;
      });
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
