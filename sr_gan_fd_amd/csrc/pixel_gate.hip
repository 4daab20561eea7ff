// pixel_gate.hip -- A-ESRGAN's pixel attention (A-ESRGAN/model.py:105-106, :136-137): a feature map times 1 + sigmoid of a
// pre-activation map, per pixel and channel, and its backward.  Bandwidth-bound: one grid-stride pass, 16 bytes per lane and tensor,
// fp32 arithmetic, one rounding at the store.  Every output element has one owner: no atomics, bit-reproducible.
//   bwd = 0   z  = x * (1 + s)                      s = sigmoid(a)
//   bwd = 1   dx = dz * (1 + s),  da = dz * x * s * (1 - s)      s recomputed from a: no sigmoid map is stored
// With e = exp(-|a|): s = 1 / (1 + e) (a >= 0) or e / (1 + e), and s (1 - s) = e / (1 + e)^2 -- nothing overflows and the tails lose
// no digits to 1 - s.
#include "elementwise.hpp"

namespace srganfd {

__device__ __forceinline__ void gate_terms(float a, float& s, float& ds) {
  const float e = expf(-fabsf(a));
  const float r = 1.f / (1.f + e);
  s = a >= 0.f ? r : e * r;
  ds = e * r * r;
}

template <typename T>
__global__ __launch_bounds__(256) void pixel_gate_fwd_kernel(const void* __restrict__ x, int xC, int x0, const void* __restrict__ a, int aC, int a0,
                                                             void* __restrict__ z, int zC, int z0, size_t npix, int c) {
  constexpr int N = VecN<T>::N;
  const int cv = c / N;
  const size_t total = npix * cv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % cv) * N;
    const size_t p = i / cv;
    float vx[N], va[N];
    ldv<T>(x, p * xC + x0 + ch, vx);
    ldv<T>(a, p * aC + a0 + ch, va);
#pragma unroll
    for (int q = 0; q < N; ++q) {
      float s, ds;
      gate_terms(va[q], s, ds);
      vx[q] *= 1.f + s;
    }
    stv<T>(z, p * zC + z0 + ch, vx);
  }
}

// da may be dz itself: a lane reads its 16 bytes of dz before it writes the same 16 bytes of da, and no other lane touches them
template <typename T>
__global__ __launch_bounds__(256) void pixel_gate_bwd_kernel(const void* __restrict__ x, int xC, int x0, const void* __restrict__ a, int aC, int a0,
                                                             const void* dz, int gC, int g0, void* __restrict__ dx, int dC, int d0, void* da, int eC, int e0,
                                                             size_t npix, int c) {
  constexpr int N = VecN<T>::N;
  const int cv = c / N;
  const size_t total = npix * cv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % cv) * N;
    const size_t p = i / cv;
    float vx[N], va[N], vg[N];
    ldv<T>(x, p * xC + x0 + ch, vx);
    ldv<T>(a, p * aC + a0 + ch, va);
    ldv<T>(dz, p * gC + g0 + ch, vg);
#pragma unroll
    for (int q = 0; q < N; ++q) {
      float s, ds;
      gate_terms(va[q], s, ds);
      va[q] = vg[q] * vx[q] * ds;
      vx[q] = vg[q] * (1.f + s);
    }
    stv<T>(dx, p * dC + d0 + ch, vx);
    stv<T>(da, p * eC + e0 + ch, va);
  }
}

// do two channel slices share elements?  (slices of one buffer at disjoint channel ranges interleave in memory and do not)
static bool slices_overlap(const srganfd_view& p, const srganfd_view& q, int c) {
  return p.ptr == q.ptr && p.c0 < q.c0 + c && q.c0 < p.c0 + c;
}
static bool same_slice(const srganfd_view& p, const srganfd_view& q) { return p.ptr == q.ptr && p.c0 == q.c0 && p.cstride == q.cstride; }

extern "C" int srganfd_pixel_gate(int32_t bwd, srganfd_view x, srganfd_view a, srganfd_view z_or_dz, srganfd_view dx, srganfd_view da, int32_t dtype,
                                  int64_t npix64, int32_t c, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  const char* const what = bwd ? "pixel_gate(bwd)" : "pixel_gate";
  if (dtype != SRGANFD_BF16 && dtype != SRGANFD_F16 && dtype != SRGANFD_F32) return set_err(SRGANFD_EINVAL, "%s: bad dtype %d", what, (int)dtype);
  if (npix64 <= 0) return set_err(SRGANFD_EINVAL, "%s: npix %lld is not positive", what, (long long)npix64);
  if (c <= 0 || c % 32) return set_err(SRGANFD_EINVAL, "%s: c = %d (need a positive multiple of 32)", what, (int)c);
  const srganfd_view* used[5] = {&x, &a, &z_or_dz, &dx, &da};
  const char* const names[5] = {"x", "a", bwd ? "dz" : "z", "dx", "da"};
  const int nused = bwd ? 5 : 3;
  for (int i = 0; i < nused; ++i) {
    const srganfd_view& v = *used[i];
    if (!v.ptr) return set_err(SRGANFD_EINVAL, "%s: null pointer (%s)", what, names[i]);
    if (v.planar) return set_err(SRGANFD_EINVAL, "%s: %s is a planar view (NHWC views only)", what, names[i]);
    if (v.c0 < 0 || v.c0 % 8 || v.cstride % 8 || ((uintptr_t)v.ptr & 15))
      return set_err(SRGANFD_EINVAL, "%s: %s is misaligned (ptr 16 bytes, c0 = %d and cstride = %d multiples of 8)", what, names[i], (int)v.c0, (int)v.cstride);
    if (v.c0 + c > v.cstride) return set_err(SRGANFD_EINVAL, "%s: %s exceeds its buffer's channels (c0 %d + c %d > cstride %d)", what, names[i], (int)v.c0, (int)c, (int)v.cstride);
  }
  const size_t npix = (size_t)npix64;
  const int vn = dtype == SRGANFD_F32 ? 4 : 8;
  const unsigned grid = grid_for(npix * (size_t)(c / vn), 256, 2048);       // 256 CUs x 8 workgroups, the rest by grid stride
  if (!bwd) {
    if (slices_overlap(z_or_dz, x, c) || slices_overlap(z_or_dz, a, c)) return set_err(SRGANFD_EINVAL, "%s: z aliases an input", what);
    DISPATCH_T(dtype, SRGANFD_LAUNCH(pixel_gate_fwd_kernel<TT>, dim3(grid), dim3(256), 0, s, x.ptr, x.cstride, x.c0, a.ptr, a.cstride, a.c0, z_or_dz.ptr,
                                     z_or_dz.cstride, z_or_dz.c0, npix, c));
  } else {
    if (slices_overlap(dx, x, c) || slices_overlap(dx, a, c) || slices_overlap(dx, z_or_dz, c)) return set_err(SRGANFD_EINVAL, "%s: dx aliases an input", what);
    if (slices_overlap(da, x, c) || slices_overlap(da, a, c) || slices_overlap(da, dx, c) || (slices_overlap(da, z_or_dz, c) && !same_slice(da, z_or_dz)))
      return set_err(SRGANFD_EINVAL, "%s: da aliases something other than dz as a whole", what);
    DISPATCH_T(dtype, SRGANFD_LAUNCH(pixel_gate_bwd_kernel<TT>, dim3(grid), dim3(256), 0, s, x.ptr, x.cstride, x.c0, a.ptr, a.cstride, a.c0, z_or_dz.ptr,
                                     z_or_dz.cstride, z_or_dz.c0, dx.ptr, dx.cstride, dx.c0, da.ptr, da.cstride, da.c0, npix, c));
  }
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

}  // namespace srganfd
