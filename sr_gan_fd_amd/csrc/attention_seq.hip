// attention_seq.hip -- multi-head self-attention over SHORT sequences stored with a token stride, with dropout on the probabilities:
// the attention of nn.TransformerEncoderLayer as the reference's BSRGANtrans calls it (A-ESRGAN/model.py:725-726, batch_first=False
// on a (B, h w, C) tensor): the sequence axis is the training batch (8 tokens), the "batch" the h w pixel positions (900 of them),
// heads of 16 channels -- each problem is 8 x 8 x 16.  An MFMA tile (16 x 16 x 32) would be mostly padding, so this is plain fp32 FMA;
// csrc/attention.hip (long sequences, one image a sequence, no dropout) is untouched.
//
// Layout: qkv (seq, nseq, 3 C) token-major, the row of token s of sequence n at (s * nseq + n) -- the (S, N, E) tensor of a
// batch_first=False encoder as it lies in memory, no transposes; q | k | v within a row, head h in channels [h D, (h + 1) D) of each
// (torch's in_proj layout), C = heads * D.  out / d_out (seq, nseq, C) and d_qkv alike; lse (nseq, heads, seq) fp32;
// keep (nseq, heads, seq, seq) uint8, 1 = keep, or NULL.
//
//   S = (q k^T) / sqrt(D), P = exp(S - lse) rounded once to the compute type, P' = P * keep * keep_scale, out = P' v.
//   backward: delta = rowsum(d_out o out) (= rowsum(P o dP) with dP = dP' * keep * keep_scale, whatever the mask),
//             dP' = d_out v^T, dS = P o (dP - delta), dq = dS k / sqrt(D), dk = dS^T q / sqrt(D), dv = P'^T d_out.
//
// A row (one token of one head of one sequence) belongs to D / 16 adjacent lanes with 16 channels each; dot products are summed
// inside that group by butterfly shuffles (every lane gets the same bits).  The forward is one launch (two sweeps over the keys:
// lse first, then the normalised P); the backward is one launch in which a row's lanes first act as a query (dq) and then as a key
// (dk, dv), recomputing S with the forward's expression, so all three see the same P.  One owner per output element, fixed
// summation order, no atomics, no workspace: two runs give the same bits, and a sequence's result does not depend on the others.
#include "elementwise.hpp"

namespace srganfd {
namespace {

constexpr int kPart = 16;          // channels per lane
constexpr int kThreads = 256;
constexpr int kMaxSeq = 128;       // every row sweeps the whole sequence: meant for sequences that are a batch size

struct SeqK {
  const void* qkv; void* out; float* lse; const void* d_out; void* d_qkv; const uint8_t* keep;
  int S, N, H, C;
  float scale, keep_scale;
  size_t total;                    // rows * lanes per row
};

template <typename T> __device__ __forceinline__ void ld16(const void* p, size_t i, float* o) {
  constexpr int N = VecN<T>::N;
#pragma unroll
  for (int v = 0; v < kPart / N; ++v) ldv<T>(p, i + v * N, o + v * N);
}
template <typename T> __device__ __forceinline__ void st16(void* p, size_t i, const float* o) {
  constexpr int N = VecN<T>::N;
#pragma unroll
  for (int v = 0; v < kPart / N; ++v) stv<T>(p, i + v * N, o + v * N);
}
template <typename T> __device__ __forceinline__ float round_to(float v) { return Elem<T>::to_f(Elem<T>::from_f(v)); }

// dot product of a row: the lane's 16 channels in order, then the D / 16 lanes of the row
template <int LPR> __device__ __forceinline__ float dot_row(const float* a, const float* b) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < kPart; ++d) s += a[d] * b[d];
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) s += __shfl_xor(s, m, 64);
  return s;
}

// which row a thread works on; false past the end (whole rows: total is a multiple of LPR, so a row's lanes agree)
template <int LPR> struct Row {
  int part, n, h, i;
  __device__ __forceinline__ bool init(const SeqK& k) {
    size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const bool live = t < k.total;
    if (!live) t = 0;
    part = (int)(t % LPR); t /= LPR;
    n = (int)(t % k.N); t /= k.N;
    h = (int)(t % k.H);
    i = (int)(t / k.H);
    return live;
  }
};

template <typename T, int D>
__global__ __launch_bounds__(kThreads) void seq_attn_fwd_kernel(SeqK k) {
  constexpr int LPR = D / kPart;
  Row<LPR> w;
  const bool live = w.init(k);                                       // (no early return: the shuffles need the row's lanes, which live together)
  const size_t pitch = 3 * (size_t)k.C, col = (size_t)w.h * D + w.part * kPart;
  const size_t tok = (size_t)w.i * k.N + w.n;
  float q[kPart], kv[kPart];
  ld16<T>(k.qkv, tok * pitch + col, q);
  float m = -INFINITY, l = 0.f;
  for (int j = 0; j < k.S; ++j) {
    ld16<T>(k.qkv, ((size_t)j * k.N + w.n) * pitch + k.C + col, kv);
    const float s = dot_row<LPR>(q, kv) * k.scale;
    const float mn = fmaxf(m, s);
    l = l * expf(m - mn) + expf(s - mn);
    m = mn;
  }
  const float lse = m + logf(l);
  float o[kPart];
#pragma unroll
  for (int d = 0; d < kPart; ++d) o[d] = 0.f;
  const uint8_t* kp = k.keep ? k.keep + (((size_t)w.n * k.H + w.h) * k.S + w.i) * k.S : nullptr;
  for (int j = 0; j < k.S; ++j) {
    const size_t row = ((size_t)j * k.N + w.n) * pitch + col;
    ld16<T>(k.qkv, row + k.C, kv);
    float p = round_to<T>(expf(dot_row<LPR>(q, kv) * k.scale - lse));
    if (kp) p = kp[j] ? p * k.keep_scale : 0.f;
    ld16<T>(k.qkv, row + 2 * (size_t)k.C, kv);
#pragma unroll
    for (int d = 0; d < kPart; ++d) o[d] += p * kv[d];
  }
  if (!live) return;
  st16<T>(k.out, tok * k.C + col, o);
  if (w.part == 0) k.lse[((size_t)w.n * k.H + w.h) * k.S + w.i] = lse;
}

template <typename T, int D>
__global__ __launch_bounds__(kThreads) void seq_attn_bwd_kernel(SeqK k) {
  constexpr int LPR = D / kPart;
  Row<LPR> w;
  const bool live = w.init(k);
  const size_t pitch = 3 * (size_t)k.C, col = (size_t)w.h * D + w.part * kPart;
  const size_t tok = (size_t)w.i * k.N + w.n;
  const size_t head = (size_t)w.n * k.H + w.h;                       // lse and keep rows of this (sequence, head)
  float acc[kPart], a[kPart], b[kPart], g[kPart];
  // ---- the row as a query: dq ----
  {
    float q[kPart], go[kPart];
    ld16<T>(k.qkv, tok * pitch + col, q);
    ld16<T>(k.d_out, tok * k.C + col, go);
    ld16<T>(k.out, tok * k.C + col, a);
    const float delta = dot_row<LPR>(go, a), lse = k.lse[head * k.S + w.i];
    const uint8_t* kp = k.keep ? k.keep + (head * k.S + w.i) * k.S : nullptr;
#pragma unroll
    for (int d = 0; d < kPart; ++d) acc[d] = 0.f;
    for (int j = 0; j < k.S; ++j) {
      const size_t row = ((size_t)j * k.N + w.n) * pitch + col;
      ld16<T>(k.qkv, row + k.C, a);
      ld16<T>(k.qkv, row + 2 * (size_t)k.C, b);
      const float p = round_to<T>(expf(dot_row<LPR>(q, a) * k.scale - lse));
      float dp = dot_row<LPR>(go, b);
      if (kp) dp = kp[j] ? dp * k.keep_scale : 0.f;
      const float ds = p * (dp - delta);
#pragma unroll
      for (int d = 0; d < kPart; ++d) acc[d] += ds * a[d];
    }
#pragma unroll
    for (int d = 0; d < kPart; ++d) acc[d] *= k.scale;
    if (live) st16<T>(k.d_qkv, tok * pitch + col, acc);
  }
  // ---- the row as a key: dk and dv ----
  float kk[kPart], vv[kPart], dv[kPart];
  ld16<T>(k.qkv, tok * pitch + k.C + col, kk);
  ld16<T>(k.qkv, tok * pitch + 2 * (size_t)k.C + col, vv);
#pragma unroll
  for (int d = 0; d < kPart; ++d) acc[d] = dv[d] = 0.f;
  for (int i = 0; i < k.S; ++i) {
    const size_t qt = (size_t)i * k.N + w.n;
    ld16<T>(k.qkv, qt * pitch + col, a);                             // q of query i
    ld16<T>(k.d_out, qt * k.C + col, g);
    ld16<T>(k.out, qt * k.C + col, b);
    const float delta = dot_row<LPR>(g, b);
    const float p = round_to<T>(expf(dot_row<LPR>(a, kk) * k.scale - k.lse[head * k.S + i]));
    float dp = dot_row<LPR>(g, vv), pk = p;
    if (k.keep) {
      const bool on = k.keep[(head * k.S + i) * k.S + w.i] != 0;
      dp = on ? dp * k.keep_scale : 0.f;
      pk = on ? p * k.keep_scale : 0.f;
    }
    const float ds = p * (dp - delta);
#pragma unroll
    for (int d = 0; d < kPart; ++d) {
      dv[d] += pk * g[d];
      acc[d] += ds * a[d];
    }
  }
  if (!live) return;
#pragma unroll
  for (int d = 0; d < kPart; ++d) acc[d] *= k.scale;
  st16<T>(k.d_qkv, tok * pitch + k.C + col, acc);
  st16<T>(k.d_qkv, tok * pitch + 2 * (size_t)k.C + col, dv);
}

template <typename T>
void launch(bool bwd, int d, const SeqK& k, hipStream_t s) {
  const dim3 grid((unsigned)((k.total + kThreads - 1) / kThreads)), block(kThreads);
  if (!bwd) {
    if (d == 16) SRGANFD_LAUNCH((seq_attn_fwd_kernel<T, 16>), grid, block, 0, s, k);
    else if (d == 32) SRGANFD_LAUNCH((seq_attn_fwd_kernel<T, 32>), grid, block, 0, s, k);
    else SRGANFD_LAUNCH((seq_attn_fwd_kernel<T, 64>), grid, block, 0, s, k);
  } else {
    if (d == 16) SRGANFD_LAUNCH((seq_attn_bwd_kernel<T, 16>), grid, block, 0, s, k);
    else if (d == 32) SRGANFD_LAUNCH((seq_attn_bwd_kernel<T, 32>), grid, block, 0, s, k);
    else SRGANFD_LAUNCH((seq_attn_bwd_kernel<T, 64>), grid, block, 0, s, k);
  }
}

bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

int run(bool bwd, const srganfd_seq_attn_args* a, void* stream) {
  const char* const name = bwd ? "seq_attention_bwd" : "seq_attention_fwd";
  if (!a) return set_err(SRGANFD_EINVAL, "%s: null arguments", name);
  if (a->dtype != SRGANFD_F32 && a->dtype != SRGANFD_F16 && a->dtype != SRGANFD_BF16) return set_err(SRGANFD_EINVAL, "%s: bad dtype %d", name, a->dtype);
  if (a->head_dim != 16 && a->head_dim != 32 && a->head_dim != 64)
    return set_err(SRGANFD_EINVAL, "%s: head_dim %d (16, 32 and 64 have kernels)", name, a->head_dim);
  if (a->seq < 1 || a->nseq < 1 || a->heads < 1) return set_err(SRGANFD_EINVAL, "%s: non-positive size: seq %d, nseq %d, heads %d", name, a->seq, a->nseq, a->heads);
  if (a->seq > kMaxSeq) return set_err(SRGANFD_EINVAL, "%s: seq %d exceeds %d (short sequences only: srganfd_attention_* takes long ones)", name, a->seq, kMaxSeq);
  if ((long long)a->heads * a->head_dim > (1 << 20)) return set_err(SRGANFD_EINVAL, "%s: heads %d x head_dim %d exceeds 2^20 channels", name, a->heads, a->head_dim);
  const unsigned long long total = (unsigned long long)a->seq * a->nseq * a->heads * (a->head_dim / kPart);
  if (total > (1ull << 31) * kThreads / 2) return set_err(SRGANFD_EINVAL, "%s: seq %d x nseq %d x heads %d exceeds the grid", name, a->seq, a->nseq, a->heads);
  if (!a->qkv || !a->out || !a->lse) return set_err(SRGANFD_EINVAL, "%s: null pointer (qkv, out and lse are needed)", name);
  if (bwd && (!a->d_out || !a->d_qkv)) return set_err(SRGANFD_EINVAL, "%s: null pointer (d_out and d_qkv are needed)", name);
  if (misaligned(a->qkv) || misaligned(a->out) || (bwd && (misaligned(a->d_out) || misaligned(a->d_qkv))))
    return set_err(SRGANFD_EINVAL, "%s: qkv, out, d_out and d_qkv must be 16-byte aligned", name);
  if (a->out == a->qkv) return set_err(SRGANFD_EINVAL, "%s: out aliases qkv", name);
  if (bwd && (a->d_qkv == a->qkv || a->d_qkv == a->out || a->d_qkv == a->d_out)) return set_err(SRGANFD_EINVAL, "%s: d_qkv aliases an input", name);
  if (a->keep && !(a->keep_scale > 0.f)) return set_err(SRGANFD_EINVAL, "%s: keep_scale must be positive with a keep-mask", name);
  SeqK k;
  k.qkv = a->qkv; k.out = a->out; k.lse = a->lse; k.d_out = a->d_out; k.d_qkv = a->d_qkv; k.keep = a->keep;
  k.S = a->seq; k.N = a->nseq; k.H = a->heads; k.C = a->heads * a->head_dim;
  k.scale = 1.f / sqrtf((float)a->head_dim);
  k.keep_scale = a->keep_scale;
  k.total = (size_t)total;
  const hipStream_t s = (hipStream_t)stream;
  if (a->dtype == SRGANFD_F32) launch<float>(bwd, a->head_dim, k, s);
  else if (a->dtype == SRGANFD_F16) launch<f16_t>(bwd, a->head_dim, k, s);
  else launch<bf16_t>(bwd, a->head_dim, k, s);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

}  // namespace
}  // namespace srganfd

extern "C" int srganfd_seq_attention_fwd(const srganfd_seq_attn_args* a, void* stream) { return srganfd::run(false, a, stream); }
extern "C" int srganfd_seq_attention_bwd(const srganfd_seq_attn_args* a, void* stream) { return srganfd::run(true, a, stream); }
