// elementwise.hpp -- what the bandwidth-bound kernel files share (elementwise, layout, resample, loss, norm, optim): typed scalar
// and 16-byte vector access to channel-slice views, the View a kernel takes and the grid-stride loops over it, the two stages of a
// reduction, and the host side's grid sizing, dtype / width dispatch and argument checks (vec_ok, views_bad).
// Those kernels are grid-stride, vectorised where the layout allows, and accumulate in fp32.  A kernel that has a vector and a scalar
// form is one body on float[N] behind ldn / stn / each<N>: N = VecN<T>::N or 1.
// Reductions are two-stage (per-block partials, then one block) -> bitwise reproducible, no atomics.
#pragma once
#include "common.hpp"
#include <initializer_list>

namespace srganfd {

template <typename T> __device__ __forceinline__ float ld(const void* p, size_t i) { return Elem<T>::to_f(((const T*)p)[i]); }
template <typename T> __device__ __forceinline__ void st(void* p, size_t i, float v) { ((T*)p)[i] = Elem<T>::from_f(v); }

__device__ __forceinline__ float block_reduce_sum(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x == 0)
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += sh[i];
  return r;  // valid on thread 0
}
// ---- the two stages of a reduction, 256 threads per block.  First stage: block b leaves the sum of its threads' s in partial[b].
__device__ __forceinline__ void store_block_sum(float s, float* sh, float* __restrict__ partial) {
  const float r = block_reduce_sum(s, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}
// Second stage: the sum of partial[0 .. nblk) in a fixed order (valid on thread 0), ...
__device__ __forceinline__ float sum_partials(const float* __restrict__ partial, int nblk, float* sh) {
  float s = 0.f;
  for (int i = threadIdx.x; i < nblk; i += 256) s += partial[i];
  return block_reduce_sum(s, sh);
}
// ... and one block that hands it to an epilogue E: E::partial() and E::nblk() name the table (blockIdx.x may pick one of a batch), E::store(r)
// says what becomes of the sum.  Every epilogue keeps its own expression: `0.f + r * scale` and `r * scale` differ at r = -0.
template <typename E>
__global__ __launch_bounds__(256) void finish_kernel(const E e) {
  __shared__ float sh[4];
  const float r = sum_partials(e.partial(), e.nblk(), sh);
  if (threadIdx.x == 0) e.store(r);
}

// ---- 16-byte vector access (8 bf16 / 4 f32 channels per lane): every view-to-view kernel below has a
// vector form used whenever channel count, view offset and buffer stride are multiples of VecN<T>.
template <typename T> struct VecN { static constexpr int N = 16 / (int)sizeof(T); };
template <typename T> __device__ __forceinline__ void ldv(const void* p, size_t i, float* o) {
  if constexpr (sizeof(T) == 2) {
    unpack8<T>(*(const u32x4*)((const T*)p + i), o);
  } else {
    const f32x4 r = *(const f32x4*)((const float*)p + i);
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3];
  }
}
// non-temporal form: outputs that are written once and are far larger than the caches (the upsampled U-Net tensors: 0.5-2 GB)
template <typename T> __device__ __forceinline__ void stv_nt(void* p, size_t i, const float* v) {
  if constexpr (sizeof(T) == 2) {
    __builtin_nontemporal_store(pack8<T>(v), (u32x4*)((T*)p + i));
  } else {
    const f32x4 o = {v[0], v[1], v[2], v[3]};
    __builtin_nontemporal_store(o, (f32x4*)((float*)p + i));
  }
}
template <typename T> __device__ __forceinline__ void stv(void* p, size_t i, const float* v) {
  if constexpr (sizeof(T) == 2) {
    *(u32x4*)((T*)p + i) = pack8<T>(v);
  } else {
    const f32x4 o = {v[0], v[1], v[2], v[3]};
    *(f32x4*)((float*)p + i) = o;
  }
}

// width-generic access for a kernel body written once on float[N]: the 16-byte vector at N = VecN<T>::N, ld / st at N = 1
// (a plain store there: the non-temporal form is for vectors)
template <typename T, int N> __device__ __forceinline__ void ldn(const void* p, size_t i, float* o) {
  if constexpr (N == 1) o[0] = ld<T>(p, i); else ldv<T>(p, i, o);
}
template <typename T, int N, bool NT = false> __device__ __forceinline__ void stn(void* p, size_t i, const float* v) {
  if constexpr (N == 1) st<T>(p, i, v[0]); else if constexpr (NT) stv_nt<T>(p, i, v); else stv<T>(p, i, v);
}
// f(q) for each of the N lanes of such a body
template <int N, typename F> __device__ __forceinline__ void each(F f) {
#pragma unroll
  for (int q = 0; q < N; ++q) f(q);
}

// an NHWC channel slice as the kernels see it; at() = element index of channel ch of a pixel.  A view that is absent has p == nullptr.
struct View {
  void* p; int cs, c0;
  __device__ __forceinline__ size_t at(size_t pixel, int ch) const { return pixel * (size_t)cs + c0 + ch; }
};

// the grid-stride loops, 256 threads per block: f(i) for i < n, and f(pixel, first channel) for every group of N channels of npix pixels
template <typename F> __device__ __forceinline__ void grid_stride(size_t n, F f) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) f(i);
}
template <int N, typename F> __device__ __forceinline__ void for_each_group(size_t npix, int c, F f) {
  const int cv = c / N;
  grid_stride(npix * cv, [&](size_t i) { f(i / cv, (int)(i % cv) * N); });
}

// raw 16-byte vector (8 halves or 4 floats), widened to floats where it is used
template <typename T> __device__ __forceinline__ u32x4 ldraw(const void* p, size_t i) { return *(const u32x4*)((const T*)p + i); }
template <typename T> __device__ __forceinline__ void widen(const u32x4 raw, float* o) {
  if constexpr (sizeof(T) == 2) unpack8<T>(raw, o);
  else { o[0] = __uint_as_float(raw[0]); o[1] = __uint_as_float(raw[1]); o[2] = __uint_as_float(raw[2]); o[3] = __uint_as_float(raw[3]); }
}

// ------------------------------------------------------------------------------------------------
// host side
inline unsigned grid_for(size_t total, int block = 256, unsigned cap = 8192) {
  size_t g = (total + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}
// the refusal the entry points on plain fp32 buffers share, under the entry point's name: a null pointer or a size that is not positive
inline int refuse_empty(const char* name) { return set_err(SRGANFD_EINVAL, "%s: null / empty argument", name); }
// CALL (the rest of the arguments: a launch's own commas pass through) names the element type as TT
#define DISPATCH_T(dtype, ...)                                                                                                          \
  if ((dtype) == SRGANFD_BF16) { using TT = bf16_t; __VA_ARGS__; } else if ((dtype) == SRGANFD_F16) { using TT = f16_t; __VA_ARGS__; } \
  else if ((dtype) == SRGANFD_F32) { using TT = float; __VA_ARGS__; }                                                                   \
  else return set_err(SRGANFD_EINVAL, "bad dtype %d", (int)(dtype));
// the same where the body also has a width: CALL names it as NN, the 16-byte vector of TT when `vec` holds and 1 when not
#define DISPATCH_TN(dtype, vec, ...) \
  DISPATCH_T(dtype, if (vec) { constexpr int NN = VecN<TT>::N; __VA_ARGS__; } else { constexpr int NN = 1; __VA_ARGS__; })
// for a launch that exists for the 16-bit types only: the caller has ruled out fp32, and what is not bf16 runs as f16
#define DISPATCH_T16(dtype, ...) \
  if ((dtype) == SRGANFD_BF16) { using TT = bf16_t; __VA_ARGS__; } else { using TT = f16_t; __VA_ARGS__; }

static constexpr int kRedBlocks = 1024;  // partial sums of a two-stage reduction; workspace floats needed by the loss entry points: 2 * kRedBlocks

inline View dev_view(const srganfd_view& v) { return v.ptr ? View{v.ptr, v.cstride, v.c0} : View{nullptr, 0, 0}; }
// elements of `dtype` in a 16-byte vector (VecN<T>::N on the host)
inline int vec_width(int dtype) { return dtype == SRGANFD_F32 ? 4 : 8; }
// grids of the grid-stride kernels over `total` elements, vn of them per thread: the scalar forms stop at grid_for's 8192 blocks, the
// vector forms (1/4 or 1/8 of the threads per element) at 65536
inline dim3 group_grid(size_t total, int vn) { return dim3(vn > 1 ? grid_for(total / vn, 256, 65536) : grid_for(total)); }

// may every view be read and written as 16-byte vectors of `dtype` over c channels?  (a null view passes)
inline bool vec_ok(int dtype, int c, std::initializer_list<srganfd_view> vs) {
  const int vn = vec_width(dtype);
  if (c % vn) return false;
  for (const auto& v : vs)
    if (v.ptr && (v.c0 % vn || v.cstride % vn || ((uintptr_t)v.ptr & 15))) return false;
  return true;
}
// The per-pixel forms of layout.hip (c <= 4 image planes, 16-bit types): is `v` a whole buffer of `pitch` channels per pixel whose
// pixels can be moved as units of `bytes`, and does the call pad to exactly that pitch?
inline bool whole_pitch(const srganfd_view& v, int pitch, int bytes) { return v.cstride == pitch && v.c0 == 0 && ((uintptr_t)v.ptr & (bytes - 1)) == 0; }
inline bool rgb_ok(int dtype, int c, int cpad, int pitch) { return dtype != SRGANFD_F32 && c <= 4 && cpad == pitch; }
// What every entry point on channel-slice views refuses before it sizes a grid: a planar view (only the convolutions read those), a
// slice of c channels that ends past its buffer's cstride.  Returns the cause, or nullptr when all is well.  (a null view passes)
inline const char* views_bad(int c, std::initializer_list<srganfd_view> vs) {
  if (c <= 0) return "c <= 0";
  for (const auto& v : vs) {
    if (!v.ptr) continue;
    if (v.planar) return "NHWC views only, not planar ones";
    if (v.c0 < 0 || (long long)v.c0 + c > (long long)v.cstride) return "a channel slice ends past its buffer (c0 + c > cstride)";
  }
  return nullptr;
}
// the same with the pixel count in front: it arrives as int64 and becomes a size_t, so a negative one would size a grid over 2^64 elements
inline const char* views_bad(long long npix, int c, std::initializer_list<srganfd_view> vs) {
  if (npix <= 0) return "npix <= 0";
  return views_bad(c, vs);
}
// the same view, cb channels further on
inline srganfd_view sub_view(srganfd_view v, int cb) { if (v.ptr) v.c0 += cb; return v; }

}  // namespace srganfd
