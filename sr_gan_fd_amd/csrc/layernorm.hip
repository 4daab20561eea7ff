// layernorm.hip -- the two element-wise pieces of a post-norm transformer encoder layer (nn.TransformerEncoderLayer, norm_first=False):
// the residual add with its dropout fused into LayerNorm, forward and backward, and a stand-alone dropout for the feed-forward site.
// Tensors are contiguous (ntok, e) token-major rows in the compute type T; keep-masks are uint8 (1 = keep) of the same shape, drawn
// by the host; statistics and every accumulation are fp32 whatever T is.
//
//   add_ln_fwd_kernel   z = x + r * keep * scale (keep NULL: x + r), rounded to T and stored; then over the STORED z of a token
//       mean, rstd = 1 / sqrt(biased variance + eps) (two passes: the mean first, then the squared deviations) and
//       y = (z - mean) * rstd * gamma + beta.  The statistics of the stored z are what the backward pass re-derives x^ from, so
//       forward and backward see the same normalised values.
//   add_ln_bwd_kernel   g = dy * gamma, x^ = (z - mean) * rstd, dz = rstd * (g - mean(g) - x^ * mean(g x^)); dx = dz,
//       dr = dz * keep * scale, each rounded once at its store.
//   ln_param_partial_kernel / ln_param_reduce_kernel   dgamma = sum_t dy x^, dbeta = sum_t dy in two phases: every workgroup sums a
//       contiguous range of tokens (a thread owns 8 channels and every rows-th token, the rows are added in order through LDS), then
//       one wave per channel adds the workgroups' partial sums in a fixed order.  No atomics: two runs give the same bits.
//   dropout_apply_kernel   y = x * keep * scale, in place allowed (a lane reads its 16 bytes before it writes them).
//
// A token is handled by a group of 8 .. 64 lanes of one wave (the largest power of two <= e / 8): each lane moves 8 channels at a
// time as 16-byte vectors and the group's sums are butterfly shuffles inside the group -- every lane ends with the same bits.  The
// passes over a token re-read what the same lane wrote or read before (L1 / L2 hits); e is 64 .. 512 in this project, so a token is
// 128 bytes .. 2 KB and nothing is staged in LDS.
#include "elementwise.hpp"

namespace srganfd {
namespace {

constexpr int kChunk = 8;          // channels a lane moves at a time: one 16-byte vector of a 16-bit type, two of fp32
constexpr int kLnThreads = 256;
constexpr int kMaxE = 2048;        // the parameter-gradient kernel gives every 8 channels a thread of a 256-thread workgroup

template <typename T> __device__ __forceinline__ void ld8(const void* p, size_t i, float* o) {
  if constexpr (sizeof(T) == 2) {
    ldv<T>(p, i, o);
  } else {
    ldv<T>(p, i, o);
    ldv<T>(p, i + 4, o + 4);
  }
}
template <typename T> __device__ __forceinline__ void st8(void* p, size_t i, const float* v) {
  if constexpr (sizeof(T) == 2) {
    stv<T>(p, i, v);
  } else {
    stv<T>(p, i, v);
    stv<T>(p, i + 4, v + 4);
  }
}
// what a value becomes when it is stored in T and read back
template <typename T> __device__ __forceinline__ float round_to(float v) { return Elem<T>::to_f(Elem<T>::from_f(v)); }

// keep-mask factors of 8 consecutive elements: scale where the byte is non-zero, else 0 (keep NULL: all 1)
__device__ __forceinline__ void keep8(const uint8_t* keep, size_t i, float scale, float* f) {
  if (!keep) {
#pragma unroll
    for (int q = 0; q < kChunk; ++q) f[q] = 1.f;
    return;
  }
  const unsigned long long bits = *(const unsigned long long*)(keep + i);
#pragma unroll
  for (int q = 0; q < kChunk; ++q) f[q] = ((bits >> (8 * q)) & 0xffull) ? scale : 0.f;
}

// sum over the `lpt` lanes of a token's group (a power of two, groups aligned): every lane gets the same bits
__device__ __forceinline__ float group_sum(float v, int lpt) {
  for (int m = 1; m < lpt; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// lanes per token: the largest power of two <= e / 8, at most 64
inline int lanes_per_token(int e) {
  int l = 1;
  while (2 * l <= e / kChunk && 2 * l <= 64) l *= 2;
  return l;
}

template <typename T>
__global__ __launch_bounds__(kLnThreads) void add_ln_fwd_kernel(const void* __restrict__ x, const void* __restrict__ r, const uint8_t* __restrict__ keep,
                                                                float scale, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                void* z, void* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd,
                                                                size_t ntok, int e, int lpt) {
  const int tpb = kLnThreads / lpt;                       // tokens per workgroup
  const int sub = threadIdx.x % lpt;
  const size_t tok = (size_t)blockIdx.x * tpb + threadIdx.x / lpt;
  const bool live = tok < ntok;                           // (no early return: the group's shuffles need every lane of the wave)
  const size_t base = tok * (size_t)e;
  float sum = 0.f;
  if (live)
    for (int c = sub * kChunk; c < e; c += lpt * kChunk) {
      float vx[kChunk], vr[kChunk], f[kChunk];
      ld8<T>(x, base + c, vx);
      ld8<T>(r, base + c, vr);
      keep8(keep, base + c, scale, f);
#pragma unroll
      for (int q = 0; q < kChunk; ++q) {
        vx[q] = round_to<T>(vx[q] + vr[q] * f[q]);
        sum += vx[q];
      }
      st8<T>(z, base + c, vx);
    }
  const float mu = group_sum(sum, lpt) / (float)e;
  float sq = 0.f;
  if (live)
    for (int c = sub * kChunk; c < e; c += lpt * kChunk) {
      float vz[kChunk];
      ld8<T>(z, base + c, vz);                            // the lane's own stores
#pragma unroll
      for (int q = 0; q < kChunk; ++q) sq += (vz[q] - mu) * (vz[q] - mu);
    }
  const float rs = 1.f / sqrtf(group_sum(sq, lpt) / (float)e + eps);
  if (!live) return;
  for (int c = sub * kChunk; c < e; c += lpt * kChunk) {
    float vz[kChunk];
    ld8<T>(z, base + c, vz);
#pragma unroll
    for (int q = 0; q < kChunk; ++q) vz[q] = (vz[q] - mu) * rs * gamma[c + q] + beta[c + q];
    st8<T>(y, base + c, vz);
  }
  if (sub == 0) { mean[tok] = mu; rstd[tok] = rs; }
}

template <typename T>
__global__ __launch_bounds__(kLnThreads) void add_ln_bwd_kernel(const void* __restrict__ dy, const void* __restrict__ z, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                const uint8_t* __restrict__ keep, float scale, void* __restrict__ dx, void* __restrict__ dr,
                                                                size_t ntok, int e, int lpt) {
  const int tpb = kLnThreads / lpt;
  const int sub = threadIdx.x % lpt;
  const size_t tok = (size_t)blockIdx.x * tpb + threadIdx.x / lpt;
  const bool live = tok < ntok;
  const size_t base = tok * (size_t)e;
  const float mu = live ? mean[tok] : 0.f, rs = live ? rstd[tok] : 0.f;
  float sg = 0.f, sgx = 0.f;
  if (live)
    for (int c = sub * kChunk; c < e; c += lpt * kChunk) {
      float vg[kChunk], vz[kChunk];
      ld8<T>(dy, base + c, vg);
      ld8<T>(z, base + c, vz);
#pragma unroll
      for (int q = 0; q < kChunk; ++q) {
        const float g = vg[q] * gamma[c + q];
        sg += g;
        sgx += g * ((vz[q] - mu) * rs);
      }
    }
  const float c1 = group_sum(sg, lpt) / (float)e, c2 = group_sum(sgx, lpt) / (float)e;
  if (!live) return;
  for (int c = sub * kChunk; c < e; c += lpt * kChunk) {
    float vg[kChunk], vz[kChunk], f[kChunk];
    ld8<T>(dy, base + c, vg);
    ld8<T>(z, base + c, vz);
    keep8(keep, base + c, scale, f);
#pragma unroll
    for (int q = 0; q < kChunk; ++q) {
      const float xh = (vz[q] - mu) * rs;
      vg[q] = rs * (vg[q] * gamma[c + q] - c1 - xh * c2);
      vz[q] = vg[q] * f[q];
    }
    st8<T>(dx, base + c, vg);
    st8<T>(dr, base + c, vz);
  }
}

// phase 1 of dgamma / dbeta: workgroup b sums tokens [b * per, (b + 1) * per); part[(b * 2 + which) * e + c], which 0: dgamma, 1: dbeta
template <typename T>
__global__ __launch_bounds__(kLnThreads) void ln_param_partial_kernel(const void* __restrict__ dy, const void* __restrict__ z, const float* __restrict__ mean,
                                                                      const float* __restrict__ rstd, float* __restrict__ part, size_t ntok, size_t per, int e) {
  __shared__ float sh[kLnThreads * 2 * kChunk];
  const int nch = e / kChunk, rows = kLnThreads / nch;
  const int tid = threadIdx.x, row = tid / nch, c = (tid % nch) * kChunk;
  const size_t t0 = (size_t)blockIdx.x * per, t1 = t0 + per < ntok ? t0 + per : ntok;
  float ag[kChunk], ab[kChunk];
#pragma unroll
  for (int q = 0; q < kChunk; ++q) ag[q] = ab[q] = 0.f;
  if (row < rows)
    for (size_t t = t0 + row; t < t1; t += rows) {
      float vg[kChunk], vz[kChunk];
      ld8<T>(dy, t * e + c, vg);
      ld8<T>(z, t * e + c, vz);
      const float mu = mean[t], rs = rstd[t];
#pragma unroll
      for (int q = 0; q < kChunk; ++q) {
        ag[q] += vg[q] * ((vz[q] - mu) * rs);
        ab[q] += vg[q];
      }
    }
#pragma unroll
  for (int q = 0; q < kChunk; ++q) { sh[tid * 2 * kChunk + q] = ag[q]; sh[tid * 2 * kChunk + kChunk + q] = ab[q]; }
  __syncthreads();
  if (row != 0) return;
  for (int rr = 1; rr < rows; ++rr) {
    const float* o = sh + (rr * nch + tid) * 2 * kChunk;
#pragma unroll
    for (int q = 0; q < kChunk; ++q) { ag[q] += o[q]; ab[q] += o[kChunk + q]; }
  }
  float* pg = part + (size_t)blockIdx.x * 2 * e + c;
#pragma unroll
  for (int q = 0; q < kChunk; ++q) { pg[q] = ag[q]; pg[e + q] = ab[q]; }
}

// phase 2: one wave per (which, channel): lane l adds the partial sums of workgroups l, l + 64, ... in order, then the lanes are added
// by a butterfly -- a fixed order, and no chain of dependent loads as long as the workgroup count
__global__ __launch_bounds__(64) void ln_param_reduce_kernel(const float* __restrict__ part, int nblk, int e, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta) {
  const int i = blockIdx.x, lane = threadIdx.x;                  // grid: 2 e workgroups of one wave
  float s = 0.f;
  for (int b = lane; b < nblk; b += 64) s += part[(size_t)b * 2 * e + i];
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m, 64);
  if (lane == 0) {
    if (i < e) dgamma[i] = s;
    else dbeta[i - e] = s;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void dropout_apply_kernel(const void* x, const uint8_t* __restrict__ keep, float scale, void* y, size_t nvec) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
    float v[kChunk], f[kChunk];
    ld8<T>(x, i * kChunk, v);
    keep8(keep, i * kChunk, scale, f);
#pragma unroll
    for (int q = 0; q < kChunk; ++q) v[q] *= f[q];
    st8<T>(y, i * kChunk, v);
  }
}

bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

// workgroups of phase 1 and the tokens each sums
void param_split(long long ntok, int* nblk, long long* per) {
  long long n = (ntok + 31) / 32;
  if (n > 256) n = 256;
  if (n < 1) n = 1;
  *per = (ntok + n - 1) / n;
  *nblk = (int)((ntok + *per - 1) / *per);
}

int check_shape(const char* what, int dtype, long long ntok, int e) {
  if (dtype != SRGANFD_BF16 && dtype != SRGANFD_F16 && dtype != SRGANFD_F32) return set_err(SRGANFD_EINVAL, "%s: bad dtype %d", what, dtype);
  if (ntok <= 0 || ntok > (1ll << 31)) return set_err(SRGANFD_EINVAL, "%s: ntok %lld outside 1 .. 2^31", what, ntok);
  if (e < 32 || e % 32 || e > kMaxE) return set_err(SRGANFD_EINVAL, "%s: e = %d (need a multiple of 32 in 32 .. %d)", what, e, kMaxE);
  return SRGANFD_OK;
}

}  // namespace
}  // namespace srganfd

using namespace srganfd;

extern "C" int srganfd_add_layernorm_fwd(int32_t dtype, const void* x, const void* r, const uint8_t* keep, float keep_scale, const float* gamma,
                                         const float* beta, float eps, void* z, void* y, float* mean, float* rstd, int64_t ntok, int32_t e, void* stream) {
  const char* const what = "add_layernorm_fwd";
  if (int rc = check_shape(what, dtype, ntok, e)) return rc;
  if (!x || !r || !gamma || !beta || !z || !y || !mean || !rstd)
    return set_err(SRGANFD_EINVAL, "%s: null pointer (x, r, gamma, beta, z, y, mean and rstd are needed)", what);
  if (misaligned(x) || misaligned(r) || misaligned(z) || misaligned(y) || ((uintptr_t)keep & 7))
    return set_err(SRGANFD_EINVAL, "%s: x, r, z and y must be 16-byte aligned, keep 8-byte aligned", what);
  if (z == x || z == r || y == x || y == r || y == z) return set_err(SRGANFD_EINVAL, "%s: z and y alias an input or each other", what);
  if (!(eps > 0.f)) return set_err(SRGANFD_EINVAL, "%s: eps must be positive", what);
  const int lpt = lanes_per_token(e);
  const unsigned grid = (unsigned)((ntok + kLnThreads / lpt - 1) / (kLnThreads / lpt));
  DISPATCH_T(dtype, SRGANFD_LAUNCH(add_ln_fwd_kernel<TT>, dim3(grid), dim3(kLnThreads), 0, (hipStream_t)stream, x, r, keep, keep_scale, gamma, beta, eps, z, y,
                                   mean, rstd, (size_t)ntok, e, lpt));
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

extern "C" size_t srganfd_add_layernorm_workspace_bytes(int64_t ntok, int32_t e) {
  if (check_shape("add_layernorm_workspace_bytes", SRGANFD_F32, ntok, e)) return 0;
  int nblk;
  long long per;
  param_split(ntok, &nblk, &per);
  return (size_t)nblk * 2 * e * sizeof(float);
}

extern "C" int srganfd_add_layernorm_bwd(int32_t dtype, const void* dy, const void* z, const float* mean, const float* rstd, const float* gamma,
                                         const uint8_t* keep, float keep_scale, void* dx, void* dr, float* dgamma, float* dbeta, void* workspace,
                                         size_t workspace_bytes, int64_t ntok, int32_t e, void* stream) {
  const char* const what = "add_layernorm_bwd";
  if (int rc = check_shape(what, dtype, ntok, e)) return rc;
  if (!dy || !z || !mean || !rstd || !gamma || !dx || !dr)
    return set_err(SRGANFD_EINVAL, "%s: null pointer (dy, z, mean, rstd, gamma, dx and dr are needed)", what);
  if ((dgamma == nullptr) != (dbeta == nullptr)) return set_err(SRGANFD_EINVAL, "%s: dgamma and dbeta come together or not at all", what);
  if (misaligned(dy) || misaligned(z) || misaligned(dx) || misaligned(dr) || ((uintptr_t)keep & 7))
    return set_err(SRGANFD_EINVAL, "%s: dy, z, dx and dr must be 16-byte aligned, keep 8-byte aligned", what);
  if (dx == dy || dx == z || dr == dy || dr == z || dr == dx) return set_err(SRGANFD_EINVAL, "%s: dx and dr alias an input or each other", what);
  int nblk = 0;
  long long per = 0;
  if (dgamma) {
    param_split(ntok, &nblk, &per);
    const size_t need = (size_t)nblk * 2 * e * sizeof(float);
    if (!workspace || misaligned(workspace) || workspace_bytes < need)
      return set_err(SRGANFD_EINVAL, "%s: workspace too small or misaligned: %zu bytes, srganfd_add_layernorm_workspace_bytes asks for %zu", what,
                     workspace ? workspace_bytes : (size_t)0, need);
  }
  const hipStream_t s = (hipStream_t)stream;
  const int lpt = lanes_per_token(e);
  const unsigned grid = (unsigned)((ntok + kLnThreads / lpt - 1) / (kLnThreads / lpt));
  DISPATCH_T(dtype, SRGANFD_LAUNCH(add_ln_bwd_kernel<TT>, dim3(grid), dim3(kLnThreads), 0, s, dy, z, mean, rstd, gamma, keep, keep_scale, dx, dr, (size_t)ntok,
                                   e, lpt));
  if (dgamma) {
    DISPATCH_T(dtype, SRGANFD_LAUNCH(ln_param_partial_kernel<TT>, dim3((unsigned)nblk), dim3(kLnThreads), 0, s, dy, z, mean, rstd, (float*)workspace,
                                     (size_t)ntok, (size_t)per, e));
    SRGANFD_LAUNCH(ln_param_reduce_kernel, dim3((unsigned)(2 * e)), dim3(64), 0, s, (const float*)workspace, nblk, e, dgamma, dbeta);
  }
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

extern "C" int srganfd_dropout_apply(int32_t dtype, const void* x, const uint8_t* keep, float scale, void* y, int64_t numel, void* stream) {
  const char* const what = "dropout_apply";
  if (dtype != SRGANFD_BF16 && dtype != SRGANFD_F16 && dtype != SRGANFD_F32) return set_err(SRGANFD_EINVAL, "%s: bad dtype %d", what, (int)dtype);
  if (!x || !keep || !y) return set_err(SRGANFD_EINVAL, "%s: null pointer (x, keep and y are needed)", what);
  if (numel <= 0 || numel % kChunk) return set_err(SRGANFD_EINVAL, "%s: numel %lld is not a positive multiple of 8", what, (long long)numel);
  if (misaligned(x) || misaligned(y) || ((uintptr_t)keep & 7)) return set_err(SRGANFD_EINVAL, "%s: x and y must be 16-byte aligned, keep 8-byte aligned", what);
  const size_t nvec = (size_t)numel / kChunk;
  DISPATCH_T(dtype, SRGANFD_LAUNCH(dropout_apply_kernel<TT>, dim3(grid_for(nvec, 256, 2048)), dim3(256), 0, (hipStream_t)stream, x, keep, scale, y, nvec));
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
