// attention.hip -- fused multi-head self-attention (the reference's SelfAttention, BSRGAN/model.py:388-402: nn.MultiheadAttention
// without masks or dropout), forward and backward, for head sizes 16 / 32 / 64 and any sequence length.
//
// The operand is the packed in-projection output qkv (B, L, 3C), token-major: q | k | v in a token's row, head h in channels
// [h D, (h + 1) D) of each, C = H D.  S = (q k^T) / sqrt(D) with the scale applied to the fp32 product, P = exp(S - lse).
//
//   attn_fwd_kernel      one workgroup per (query block, head, batch), one wave per 16 query rows.  Two sweeps over the key tiles
//       (32 keys each): the first keeps a running row maximum and sum and ends in lse = max + log(sum); the second recomputes S,
//       forms the NORMALISED P = exp(S - lse) in fp32, rounds it once to the compute type and accumulates O += P v.  The same
//       expression gives P in the weights kernel and in both backward kernels, so all four see the same probabilities.
//   attn_weights_kernel  W[b, i, j] = (1 / H) sum_h P_h[i, j] from the fp32 probabilities, heads summed in order.
//   attn_bwd_dq_kernel   per query block, sweeps the keys: delta = rowsum(dO o O) (also written to the workspace for the second
//       launch), dS = P o (dP - delta), dQ = dS k / sqrt(D).
//   attn_bwd_dkv_kernel  per key block, sweeps the queries: dV = P^T dO, dK = dS^T q / sqrt(D).
//
// Every output element has one owner and every sum a fixed order: no atomics, no hand-off between workgroups, no waits -- two runs
// are bit-equal, and a batch entry's result does not depend on the others.  Tiles are staged in LDS (rows past L and, for D = 16,
// columns past D are zero) and every product is v_mfma_f32_16x16x32_{f16,bf16} (fp32 accumulation), or v_mfma_f32_16x16x4_f32 in the
// exact-fp32 mode, fed from LDS through the lane maps of conv_common.hpp.  Keys past L enter the softmax as -inf (P = 0), rows
// past L are never stored.  The arithmetic is tiny (27 GFLOP forward at batch 16, 1296 tokens, 8 heads of 32), so the structure
// is the simplest that is correct; DESIGN.md 4d has the times.
#include "conv_common.hpp"

namespace srganfd {
namespace {

constexpr int kTile = 32;        // keys (forward, dQ) or queries (dK / dV) per swept tile: the K of one 16-bit MFMA

template <typename T> struct Store { typedef unsigned short type; };      // what a tile holds: the 16-bit types as raw bits
template <> struct Store<float> { typedef float type; };

template <typename T> __device__ __forceinline__ float ld_f(typename Store<T>::type v);
template <> __device__ __forceinline__ float ld_f<bf16_t>(unsigned short v) { return bf2f(v); }
template <> __device__ __forceinline__ float ld_f<f16_t>(unsigned short v) { return (float)__builtin_bit_cast(_Float16, v); }
template <> __device__ __forceinline__ float ld_f<float>(float v) { return v; }
template <typename T> __device__ __forceinline__ typename Store<T>::type st_f(float v);
template <> __device__ __forceinline__ unsigned short st_f<bf16_t>(float v) { return f2bf(v); }
template <> __device__ __forceinline__ unsigned short st_f<f16_t>(float v) { return __builtin_bit_cast(unsigned short, (_Float16)v); }
template <> __device__ __forceinline__ float st_f<float>(float v) { return v; }

template <typename T, int D> struct Cfg {
  typedef typename Store<T>::type S;
  static constexpr int kWaves = sizeof(T) == 4 ? 2 : 4;     // fp32 tiles are twice the bytes: half the rows per workgroup
  static constexpr int kThreads = 64 * kWaves;
  static constexpr int kRows = 16 * kWaves;                 // rows a workgroup owns (16 per wave)
  static constexpr int kChunk = 16 / (int)sizeof(S);        // elements per 16-byte access
  static constexpr int DP = D < 32 ? 32 : D;                // tile columns: D = 16 is zero-padded to one MFMA's K
  static constexpr int LD = DP + kChunk;                    // row pitch of a (rows x DP) tile
  static constexpr int LDP = kTile + kChunk;                // row pitch of a (16 x kTile) probability tile
};

struct AttnK {
  const void* qkv; void* out; float* lse; const void* d_out; void* d_qkv; float* weights; float* delta;
  int B, L, H, C;
  float scale;
};

// rows [row0, row0 + nrows) of one head of q, k, v, O or dO -- D elements at `pitch` elements per token, src at token 0 -- into
// tile[nrows][LD]; rows at or past L and columns at or past D are zero
template <typename T, int D>
__device__ __forceinline__ void load_tile(typename Store<T>::type* tile, const typename Store<T>::type* src, long long pitch, int row0, int nrows,
                                          int L, int tid) {
  typedef Cfg<T, D> G;
  constexpr int CPR = G::DP / G::kChunk;
  for (int i = tid; i < nrows * CPR; i += G::kThreads) {
    const int r = i / CPR, c = (i % CPR) * G::kChunk;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row0 + r < L && c < D) v = *(const u32x4*)(src + (long long)(row0 + r) * pitch + c);
    *(u32x4*)(tile + r * G::LD + c) = v;
  }
}

// C (16 x 16, the 16x16 MFMA accumulator layout: column = lane & 15, row = 4 (lane >> 4) + register) += A (16 x 32) B (32 x 16) from LDS.
// AK: A is stored [m][k] (else [k][m]) and `a` points at its (m, k) = (0, 0); BK: B is stored [n][k] (else [k][n]), `b` alike.
template <typename T, bool AK, bool BK>
__device__ __forceinline__ f32x4_t mma32(const typename Store<T>::type* a, int lda, const typename Store<T>::type* b, int ldb, f32x4_t c, int lane) {
  const int r = lane & 15, g = lane >> 4;
  if constexpr (sizeof(T) == 2) {
    // lane holds A[row r][k = 8 g + j] and B[k = 8 g + j][col r], j = 0..7
    u16x8 av, bv;
    if constexpr (AK) {
      av = __builtin_bit_cast(u16x8, *(const u32x4*)(a + r * lda + 8 * g));
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) av[j] = a[(8 * g + j) * lda + r];
    }
    if constexpr (BK) {
      bv = __builtin_bit_cast(u16x8, *(const u32x4*)(b + r * ldb + 8 * g));
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) bv[j] = b[(8 * g + j) * ldb + r];
    }
    typedef typename FragAB<T>::type F;
    return mfma16<T>(__builtin_bit_cast(F, av), __builtin_bit_cast(F, bv), c);
  } else {
    // v_mfma_f32_16x16x4_f32: lane holds A[row r][k = g] and B[k = g][col r]; eight steps cover the 32
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int k = 4 * s + g;
      const float af = AK ? a[r * lda + k] : a[k * lda + r];
      const float bf = BK ? b[r * ldb + k] : b[k * ldb + r];
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf, c, 0, 0, 0);
    }
    return c;
  }
}

// s[nb] = rows (16 of `a`, [row][d]) x columns (16 nb .. 16 nb + 15 of `bt`, [column][d]) summed over d
template <typename T, int D>
__device__ __forceinline__ void dot_tiles(const typename Store<T>::type* a, const typename Store<T>::type* bt, f32x4_t s[2], int lane) {
  typedef Cfg<T, D> G;
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    s[nb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k0 = 0; k0 < G::DP; k0 += 32) s[nb] = mma32<T, true, true>(a + k0, G::LD, bt + nb * 16 * G::LD + k0, G::LD, s[nb], lane);
  }
}

__device__ __forceinline__ float max16(float v) {
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ float sum16(float v) {
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

template <typename T, int D>
__global__ __launch_bounds__((Cfg<T, D>::kThreads)) void attn_fwd_kernel(AttnK k) {
  typedef Cfg<T, D> G;
  typedef typename G::S S;
  __shared__ __attribute__((aligned(16))) S Qs[G::kRows * G::LD], Ks[kTile * G::LD], Vs[kTile * G::LD], Ps[G::kRows * G::LDP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * G::kRows, h = blockIdx.y, b = blockIdx.z, L = k.L;
  const long long pitch = 3LL * k.C;
  const S* qp = (const S*)k.qkv + (long long)b * L * pitch + h * D;
  const S* kp = qp + k.C;
  const S* vp = qp + 2 * k.C;
  const S* qw = Qs + 16 * w * G::LD;
  S* pw = Ps + 16 * w * G::LDP;
  const int ntiles = (L + kTile - 1) / kTile;
  load_tile<T, D>(Qs, qp, pitch, q0, G::kRows, L, tid);

  // sweep 1: running maximum and sum of every row (a tile always holds a key below L, so the maximum is finite after the first)
  float m[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { m[i] = -INFINITY; l[i] = 0.f; }
  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();
    load_tile<T, D>(Ks, kp, pitch, t * kTile, kTile, L, tid);
    __syncthreads();
    f32x4_t s[2];
    dot_tiles<T, D>(qw, Ks, s, lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v[2];
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) v[nb] = (t * kTile + 16 * nb + r < L) ? s[nb][i] * k.scale : -INFINITY;
      const float mn = fmaxf(m[i], max16(fmaxf(v[0], v[1])));
      const float e = sum16(expf(v[0] - mn) + expf(v[1] - mn));
      l[i] = l[i] * expf(m[i] - mn) + e;
      m[i] = mn;
    }
  }
  float lse[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lse[i] = m[i] + logf(l[i]);
    const int q = q0 + 16 * w + 4 * g + i;
    if (r == 0 && q < L) k.lse[((long long)b * k.H + h) * L + q] = lse[i];
  }

  // sweep 2: O += P v with the normalised P
  f32x4_t o[D / 16];
#pragma unroll
  for (int nb = 0; nb < D / 16; ++nb) o[nb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();
    load_tile<T, D>(Ks, kp, pitch, t * kTile, kTile, L, tid);
    load_tile<T, D>(Vs, vp, pitch, t * kTile, kTile, L, tid);
    __syncthreads();
    f32x4_t s[2];
    dot_tiles<T, D>(qw, Ks, s, lane);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = (t * kTile + 16 * nb + r < L) ? expf(s[nb][i] * k.scale - lse[i]) : 0.f;
        pw[(4 * g + i) * G::LDP + 16 * nb + r] = st_f<T>(p);
      }
    __syncthreads();
#pragma unroll
    for (int nb = 0; nb < D / 16; ++nb) o[nb] = mma32<T, true, false>(pw, G::LDP, Vs + 16 * nb, G::LD, o[nb], lane);
  }
  S* op = (S*)k.out + (long long)b * L * k.C + h * D;
#pragma unroll
  for (int nb = 0; nb < D / 16; ++nb)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = q0 + 16 * w + 4 * g + i;
      if (q < L) op[(long long)q * k.C + 16 * nb + r] = st_f<T>(o[nb][i]);
    }
}

template <typename T, int D>
__global__ __launch_bounds__((Cfg<T, D>::kThreads)) void attn_weights_kernel(AttnK k) {
  typedef Cfg<T, D> G;
  typedef typename G::S S;
  __shared__ __attribute__((aligned(16))) S Qs[G::kRows * G::LD], Ks[kTile * G::LD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * G::kRows, j0 = blockIdx.y * kTile, b = blockIdx.z, L = k.L;
  const long long pitch = 3LL * k.C;
  f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
  for (int h = 0; h < k.H; ++h) {
    const S* qp = (const S*)k.qkv + (long long)b * L * pitch + h * D;
    __syncthreads();
    load_tile<T, D>(Qs, qp, pitch, q0, G::kRows, L, tid);
    load_tile<T, D>(Ks, qp + k.C, pitch, j0, kTile, L, tid);
    __syncthreads();
    f32x4_t s[2];
    dot_tiles<T, D>(Qs + 16 * w * G::LD, Ks, s, lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = q0 + 16 * w + 4 * g + i;
      const float lse = q < L ? k.lse[((long long)b * k.H + h) * L + q] : 0.f;
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
        if (j0 + 16 * nb + r < L) acc[nb][i] += expf(s[nb][i] * k.scale - lse);
    }
  }
  const float inv_h = 1.f / (float)k.H;
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = q0 + 16 * w + 4 * g + i, j = j0 + 16 * nb + r;
      if (q < L && j < L) k.weights[((long long)b * L + q) * L + j] = acc[nb][i] * inv_h;
    }
}

template <typename T, int D>
__global__ __launch_bounds__((Cfg<T, D>::kThreads)) void attn_bwd_dq_kernel(AttnK k) {
  typedef Cfg<T, D> G;
  typedef typename G::S S;
  __shared__ __attribute__((aligned(16))) S Qs[G::kRows * G::LD], Gs[G::kRows * G::LD], Ks[kTile * G::LD], Vs[kTile * G::LD], Ds[G::kRows * G::LDP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * G::kRows, h = blockIdx.y, b = blockIdx.z, L = k.L;
  const long long pitch = 3LL * k.C;
  const S* qp = (const S*)k.qkv + (long long)b * L * pitch + h * D;
  const S* kp = qp + k.C;
  const S* vp = qp + 2 * k.C;
  const S* gp = (const S*)k.d_out + (long long)b * L * k.C + h * D;
  const S* op = (const S*)k.out + (long long)b * L * k.C + h * D;
  load_tile<T, D>(Qs, qp, pitch, q0, G::kRows, L, tid);
  load_tile<T, D>(Gs, gp, k.C, q0, G::kRows, L, tid);
  __syncthreads();
  // delta of row 16 w + r: the lane group g sums a quarter of the head's channels, the four quarters are added in a fixed order
  float part = 0.f;
  {
    const int q = q0 + 16 * w + r;
    if (q < L)
      for (int d = g * (D / 4); d < (g + 1) * (D / 4); ++d) part += ld_f<T>(Gs[(16 * w + r) * G::LD + d]) * ld_f<T>(op[(long long)q * k.C + d]);
    part += __shfl_xor(part, 16);
    part += __shfl_xor(part, 32);
    if (g == 0 && q < L) k.delta[((long long)b * k.H + h) * L + q] = part;
  }
  float lse[4], delta[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = q0 + 16 * w + 4 * g + i;
    delta[i] = __shfl(part, 4 * g + i);
    lse[i] = q < L ? k.lse[((long long)b * k.H + h) * L + q] : 0.f;
  }
  const S* qw = Qs + 16 * w * G::LD;
  const S* gw = Gs + 16 * w * G::LD;
  S* dw = Ds + 16 * w * G::LDP;
  f32x4_t dq[D / 16];
#pragma unroll
  for (int nb = 0; nb < D / 16; ++nb) dq[nb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int ntiles = (L + kTile - 1) / kTile;
  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();
    load_tile<T, D>(Ks, kp, pitch, t * kTile, kTile, L, tid);
    load_tile<T, D>(Vs, vp, pitch, t * kTile, kTile, L, tid);
    __syncthreads();
    f32x4_t s[2], dp[2];
    dot_tiles<T, D>(qw, Ks, s, lane);
    dot_tiles<T, D>(gw, Vs, dp, lane);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = (t * kTile + 16 * nb + r < L) ? expf(s[nb][i] * k.scale - lse[i]) : 0.f;
        dw[(4 * g + i) * G::LDP + 16 * nb + r] = st_f<T>(p * (dp[nb][i] - delta[i]));
      }
    __syncthreads();
#pragma unroll
    for (int nb = 0; nb < D / 16; ++nb) dq[nb] = mma32<T, true, false>(dw, G::LDP, Ks + 16 * nb, G::LD, dq[nb], lane);
  }
  S* dqp = (S*)k.d_qkv + (long long)b * L * pitch + h * D;
#pragma unroll
  for (int nb = 0; nb < D / 16; ++nb)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = q0 + 16 * w + 4 * g + i;
      if (q < L) dqp[(long long)q * pitch + 16 * nb + r] = st_f<T>(dq[nb][i] * k.scale);
    }
}

template <typename T, int D>
__global__ __launch_bounds__((Cfg<T, D>::kThreads)) void attn_bwd_dkv_kernel(AttnK k) {
  typedef Cfg<T, D> G;
  typedef typename G::S S;
  __shared__ __attribute__((aligned(16))) S Ks[G::kRows * G::LD], Vs[G::kRows * G::LD], Qs[kTile * G::LD], Gs[kTile * G::LD], Pt[G::kRows * G::LDP],
      Dt[G::kRows * G::LDP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
  const int j0 = blockIdx.x * G::kRows, h = blockIdx.y, b = blockIdx.z, L = k.L;
  const long long pitch = 3LL * k.C;
  const S* qp = (const S*)k.qkv + (long long)b * L * pitch + h * D;
  const S* gp = (const S*)k.d_out + (long long)b * L * k.C + h * D;
  const float* lsep = k.lse + ((long long)b * k.H + h) * L;
  const float* delp = k.delta + ((long long)b * k.H + h) * L;
  load_tile<T, D>(Ks, qp + k.C, pitch, j0, G::kRows, L, tid);
  load_tile<T, D>(Vs, qp + 2 * k.C, pitch, j0, G::kRows, L, tid);
  const S* kw = Ks + 16 * w * G::LD;
  const S* vw = Vs + 16 * w * G::LD;
  S* pw = Pt + 16 * w * G::LDP;
  S* dw = Dt + 16 * w * G::LDP;
  f32x4_t dk[D / 16], dv[D / 16];
#pragma unroll
  for (int nb = 0; nb < D / 16; ++nb) { dk[nb] = f32x4_t{0.f, 0.f, 0.f, 0.f}; dv[nb] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
  const int ntiles = (L + kTile - 1) / kTile;
  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();
    load_tile<T, D>(Qs, qp, pitch, t * kTile, kTile, L, tid);
    load_tile<T, D>(Gs, gp, k.C, t * kTile, kTile, L, tid);
    __syncthreads();
    // transposed: this wave's 16 keys on the rows, the tile's 32 queries on the columns
    f32x4_t s[2], dp[2];
    dot_tiles<T, D>(kw, Qs, s, lane);
    dot_tiles<T, D>(vw, Gs, dp, lane);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int q = t * kTile + 16 * nb + r;
      const float lse = q < L ? lsep[q] : 0.f, delta = q < L ? delp[q] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = (q < L && j0 + 16 * w + 4 * g + i < L) ? expf(s[nb][i] * k.scale - lse) : 0.f;
        pw[(4 * g + i) * G::LDP + 16 * nb + r] = st_f<T>(p);
        dw[(4 * g + i) * G::LDP + 16 * nb + r] = st_f<T>(p * (dp[nb][i] - delta));
      }
    }
    __syncthreads();
#pragma unroll
    for (int nb = 0; nb < D / 16; ++nb) {
      dv[nb] = mma32<T, true, false>(pw, G::LDP, Gs + 16 * nb, G::LD, dv[nb], lane);
      dk[nb] = mma32<T, true, false>(dw, G::LDP, Qs + 16 * nb, G::LD, dk[nb], lane);
    }
  }
  S* dkp = (S*)k.d_qkv + (long long)b * L * pitch + k.C + h * D;
  S* dvp = dkp + k.C;
#pragma unroll
  for (int nb = 0; nb < D / 16; ++nb)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = j0 + 16 * w + 4 * g + i;
      if (j < L) {
        dkp[(long long)j * pitch + 16 * nb + r] = st_f<T>(dk[nb][i] * k.scale);
        dvp[(long long)j * pitch + 16 * nb + r] = st_f<T>(dv[nb][i]);
      }
    }
}

enum { kFwd, kWeights, kBwd };

template <typename T, int D>
void launch(int what, const AttnK& k, hipStream_t s) {
  typedef Cfg<T, D> G;
  const unsigned nblk = (unsigned)ceil_div(k.L, G::kRows);
  const dim3 grid(nblk, (unsigned)k.H, (unsigned)k.B), block(G::kThreads);
  if (what == kFwd) {
    SRGANFD_LAUNCH((attn_fwd_kernel<T, D>), grid, block, 0, s, k);
  } else if (what == kWeights) {
    SRGANFD_LAUNCH((attn_weights_kernel<T, D>), dim3(nblk, (unsigned)ceil_div(k.L, kTile), (unsigned)k.B), block, 0, s, k);
  } else {
    SRGANFD_LAUNCH((attn_bwd_dq_kernel<T, D>), grid, block, 0, s, k);      // writes delta, which the second launch reads
    SRGANFD_LAUNCH((attn_bwd_dkv_kernel<T, D>), grid, block, 0, s, k);
  }
}

template <typename T>
void launch_d(int what, int d, const AttnK& k, hipStream_t s) {
  if (d == 16) launch<T, 16>(what, k, s);
  else if (d == 32) launch<T, 32>(what, k, s);
  else launch<T, 64>(what, k, s);
}

size_t workspace_need(const srganfd_attn_args* a) { return (size_t)a->batch * a->heads * a->seq * sizeof(float); }

// the checks every entry point shares; `name` prefixes the error text
int check_common(const srganfd_attn_args* a, const char* name) {
  if (!a) return set_err(SRGANFD_EINVAL, "%s: null arguments", name);
  if (a->dtype != SRGANFD_F32 && a->dtype != SRGANFD_F16 && a->dtype != SRGANFD_BF16) return set_err(SRGANFD_EINVAL, "%s: bad dtype %d", name, a->dtype);
  if (a->head_dim != 16 && a->head_dim != 32 && a->head_dim != 64)
    return set_err(SRGANFD_EINVAL, "%s: head_dim %d (16, 32 and 64 have kernels)", name, a->head_dim);
  if (a->batch < 1 || a->seq < 1 || a->heads < 1) return set_err(SRGANFD_EINVAL, "%s: non-positive size: batch %d, seq %d, heads %d", name, a->batch, a->seq, a->heads);
  if (a->batch > 65535 || a->heads > 65535 || a->seq > (1 << 20) || (long long)a->heads * a->head_dim > (1 << 20))
    return set_err(SRGANFD_EINVAL, "%s: batch %d, heads %d or seq %d exceeds the grid", name, a->batch, a->heads, a->seq);
  return SRGANFD_OK;
}

bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

int run(int what, const srganfd_attn_args* a, void* stream) {
  AttnK k;
  k.qkv = a->qkv; k.out = a->out; k.lse = a->lse; k.d_out = a->d_out; k.d_qkv = a->d_qkv; k.weights = a->weights; k.delta = (float*)a->workspace;
  k.B = a->batch; k.L = a->seq; k.H = a->heads; k.C = a->heads * a->head_dim;
  k.scale = 1.f / sqrtf((float)a->head_dim);
  hipStream_t s = (hipStream_t)stream;
  if (a->dtype == SRGANFD_F32) launch_d<float>(what, a->head_dim, k, s);
  else if (a->dtype == SRGANFD_F16) launch_d<f16_t>(what, a->head_dim, k, s);
  else launch_d<bf16_t>(what, a->head_dim, k, s);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

}  // namespace
}  // namespace srganfd

using namespace srganfd;

extern "C" size_t srganfd_attention_workspace_bytes(const srganfd_attn_args* a) {
  if (check_common(a, "attention_workspace_bytes") != SRGANFD_OK) return 0;
  return workspace_need(a);
}

extern "C" int srganfd_attention_fwd(const srganfd_attn_args* a, void* stream) {
  if (int rc = check_common(a, "attention_fwd")) return rc;
  if (!a->qkv || !a->out || !a->lse) return set_err(SRGANFD_EINVAL, "attention_fwd: null pointer (qkv, out and lse are needed)");
  if (misaligned(a->qkv) || misaligned(a->out)) return set_err(SRGANFD_EINVAL, "attention_fwd: qkv and out must be 16-byte aligned");
  if (a->out == a->qkv) return set_err(SRGANFD_EINVAL, "attention_fwd: out aliases qkv");
  return run(kFwd, a, stream);
}

extern "C" int srganfd_attention_weights(const srganfd_attn_args* a, void* stream) {
  if (int rc = check_common(a, "attention_weights")) return rc;
  if (!a->qkv || !a->lse || !a->weights) return set_err(SRGANFD_EINVAL, "attention_weights: null pointer (qkv, lse and weights are needed)");
  if (misaligned(a->qkv)) return set_err(SRGANFD_EINVAL, "attention_weights: qkv must be 16-byte aligned");
  return run(kWeights, a, stream);
}

extern "C" int srganfd_attention_bwd(const srganfd_attn_args* a, void* stream) {
  if (int rc = check_common(a, "attention_bwd")) return rc;
  if (!a->qkv || !a->out || !a->lse || !a->d_out || !a->d_qkv || !a->workspace)
    return set_err(SRGANFD_EINVAL, "attention_bwd: null pointer (qkv, out, lse, d_out, d_qkv and the workspace are needed)");
  if (misaligned(a->qkv) || misaligned(a->out) || misaligned(a->d_out) || misaligned(a->d_qkv) || misaligned(a->workspace))
    return set_err(SRGANFD_EINVAL, "attention_bwd: qkv, out, d_out, d_qkv and the workspace must be 16-byte aligned");
  if (a->d_qkv == a->qkv) return set_err(SRGANFD_EINVAL, "attention_bwd: d_qkv aliases qkv (the second launch still reads q, k and v)");
  if (a->workspace_bytes < workspace_need(a))
    return set_err(SRGANFD_EINVAL, "attention_bwd: workspace too small: %zu bytes, srganfd_attention_workspace_bytes asks for %zu", a->workspace_bytes,
                   workspace_need(a));
  return run(kBwd, a, stream);
}
