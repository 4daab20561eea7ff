// elementwise.hip -- per-element maps on channel-slice views that are not fused into a conv epilogue: axpby, LeakyReLU backward,
// and the A-ESRGAN attention gate's pieces (relu(a + b), sigmoid and its backward, the gate multiply).  Layout conversion is in
// layout.hip, resampling in resample.hip, losses in loss.hip, spectral norm / BatchNorm in norm.hip, Adam + EMA in optim.hip.
#include "elementwise.hpp"

namespace srganfd {

// ---- LeakyReLU backward with the sign recovered from act - skip ----
// out may be dy itself (the engines overwrite the gradient in place), so dy is not __restrict__: every element is read before it is
// written, by the same lane.  The vector and the scalar form do the same fp32 operations per element: the same bits from both.
template <typename T>
__global__ __launch_bounds__(256) void lrelu_bwd_vec_kernel(const void* dy, int dC, int d0, const void* __restrict__ act, int aC, int a0,
                                                            const void* __restrict__ skip, int sC, int s0, void* out, int oC, int o0, size_t npix, int c, float slope) {
  constexpr int N = VecN<T>::N;
  const int cv = c / N;
  const size_t total = npix * cv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % cv) * N;
    const size_t p = i / cv;
    float g[N], z[N], sk[N];
    ldv<T>(dy, p * dC + d0 + ch, g);
    ldv<T>(act, p * aC + a0 + ch, z);
    if (skip) {
      ldv<T>(skip, p * sC + s0 + ch, sk);
#pragma unroll
      for (int q = 0; q < N; ++q) z[q] -= sk[q];
    }
#pragma unroll
    for (int q = 0; q < N; ++q) g[q] *= z[q] > 0.f ? 1.f : slope;
    stv<T>(out, p * oC + o0 + ch, g);
  }
}
template <typename T>
__global__ void lrelu_bwd_kernel(const void* dy, int dC, int d0, const void* __restrict__ act, int aC, int a0,
                                 const void* __restrict__ skip, int sC, int s0, void* out, int oC, int o0, size_t npix, int c, float slope) {
  const size_t total = npix * c;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % c);
    const size_t p = i / c;
    float z = ld<T>(act, p * aC + a0 + ch);
    if (skip) z -= ld<T>(skip, p * sC + s0 + ch);
    st<T>(out, p * oC + o0 + ch, ld<T>(dy, p * dC + d0 + ch) * (z > 0.f ? 1.f : slope));
  }
}

// ---- y = a*x + b*y on channel-slice views ----
// Both forms spell the same fmaf(a, x, b * y), so that the compiler cannot contract them differently: bit-identical in f32.
// b == 0 never reads y (a NaN there does not reach the result).
template <typename T>
__global__ void axpby_kernel(const void* __restrict__ x, int xC, int x0, void* y, int yC, int y0, size_t npix, int c, float a, float b) {
  const size_t total = npix * c;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % c);
    const size_t p = i / c;
    const float v = fmaf(a, ld<T>(x, p * xC + x0 + ch), b != 0.f ? b * ld<T>(y, p * yC + y0 + ch) : 0.f);
    st<T>(y, p * yC + y0 + ch, v);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void axpby_vec_kernel(const void* __restrict__ x, int xC, int x0, void* y, int yC, int y0, size_t npix, int c, float a, float b) {
  constexpr int N = VecN<T>::N;
  const int cv = c / N;
  const size_t total = npix * cv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % cv) * N;
    const size_t p = i / cv;
    float vx[N], vy[N];
    ldv<T>(x, p * xC + x0 + ch, vx);
    if (b != 0.f) ldv<T>(y, p * yC + y0 + ch, vy);
#pragma unroll
    for (int q = 0; q < N; ++q) vx[q] = fmaf(a, vx[q], b != 0.f ? b * vy[q] : 0.f);
    stv<T>(y, p * yC + y0 + ch, vx);
  }
}

// ---- A-ESRGAN attention gates (A-ESRGAN/model.py:239-254): relu(a+b), sigmoid, gate multiply ----
template <typename T>
__global__ __launch_bounds__(256) void add_relu_kernel(const void* __restrict__ a, int aC, int a0, const void* __restrict__ b, int bC, int b0,
                                                       void* out, int oC, int o0, size_t npix, int c) {
  constexpr int N = VecN<T>::N;
  const int cv = c / N;
  const size_t total = npix * cv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % cv) * N;
    const size_t p = i / cv;
    float va[N], vb[N];
    ldv<T>(a, p * aC + a0 + ch, va);
    ldv<T>(b, p * bC + b0 + ch, vb);
#pragma unroll
    for (int q = 0; q < N; ++q) va[q] = fmaxf(va[q] + vb[q], 0.f);
    stv<T>(out, p * oC + o0 + ch, va);
  }
}
__global__ __launch_bounds__(256) void sigmoid_kernel(float* x, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) x[i] = 1.f / (1.f + expf(-x[i]));
}
// out may be ds itself (engine_a overwrites the gradient in place): ds is not __restrict__
__global__ __launch_bounds__(256) void sigmoid_bwd_kernel(const float* ds, const float* __restrict__ s, float* out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) { const float v = s[i]; out[i] = ds[i] * v * (1.f - v); }
}
// y[p][c] = gate[p] * x[p][c]
template <typename T>
__global__ __launch_bounds__(256) void gate_fwd_kernel(const void* __restrict__ x, int xC, int x0, const float* __restrict__ gate, void* y, int yC, int y0,
                                                       size_t npix, int c) {
  constexpr int N = VecN<T>::N;
  const int cv = c / N;
  const size_t total = npix * cv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % cv) * N;
    const size_t p = i / cv;
    float v[N];
    ldv<T>(x, p * xC + x0 + ch, v);
    const float gv = gate[p];
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] *= gv;
    stv<T>(y, p * yC + y0 + ch, v);
  }
}
// dx[p][c] = gate[p] * dy[p][c] ; dgate[p] = sum_c dy[p][c] * x[p][c]   (c/N lanes of a wave per pixel, c/N a power of two <= 64)
template <typename T>
__global__ __launch_bounds__(256) void gate_bwd_kernel(const void* __restrict__ x, int xC, int x0, const float* __restrict__ gate,
                                                       const void* __restrict__ dy, int dC, int d0, void* dx, int oC, int o0, float* __restrict__ dgate,
                                                       size_t npix, int c) {
  constexpr int N = VecN<T>::N;
  const int cv = c / N;                       // lanes per pixel
  const size_t total = npix * cv;
  const size_t stride = (size_t)gridDim.x * 256;
  const size_t iters = (total + stride - 1) / stride;
  for (size_t it = 0; it < iters; ++it) {
    const size_t i = it * stride + (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool ok = i < total;
    const int ch = ok ? (int)(i % cv) * N : 0;
    const size_t p = ok ? i / cv : 0;
    float vx[N], vd[N];
    float part = 0.f;
    if (ok) {
      ldv<T>(x, p * xC + x0 + ch, vx);
      ldv<T>(dy, p * dC + d0 + ch, vd);
      const float gv = gate[p];
#pragma unroll
      for (int q = 0; q < N; ++q) { part += vd[q] * vx[q]; vd[q] *= gv; }
      stv<T>(dx, p * oC + o0 + ch, vd);
    }
    for (int o = cv >> 1; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if (ok && (i % cv) == 0) dgate[p] = part;
  }
}

// ------------------------------------------------------------------------------------------------
extern "C" int srganfd_lrelu_bwd(srganfd_view dy, srganfd_view act, srganfd_view skip, srganfd_view out, int32_t dtype, int64_t npix64, int32_t c, float slope,
                                 void* stream) {
  const size_t npix = (size_t)npix64;
  const hipStream_t s = (hipStream_t)stream;
  if (!dy.ptr || !act.ptr || !out.ptr) return set_err(SRGANFD_EINVAL, "lrelu_bwd: null");
  if (const char* why = views_bad(npix64, c, {dy, act, skip, out})) return set_err(SRGANFD_EINVAL, "lrelu_bwd: %s", why);
  {
    const int vn = dtype == SRGANFD_F32 ? 4 : 8;
    auto ok = [&](const srganfd_view& v) { return !v.ptr || (v.c0 % vn == 0 && v.cstride % vn == 0 && ((uintptr_t)v.ptr & 15) == 0); };
    if (c % vn == 0 && ok(dy) && ok(act) && ok(skip) && ok(out)) {
      DISPATCH_T(dtype,
                 SRGANFD_LAUNCH(lrelu_bwd_vec_kernel<TT>, dim3(grid_for(npix * c / vn, 256, 65536)), dim3(256), 0, s, dy.ptr, dy.cstride, dy.c0, act.ptr, act.cstride, act.c0,
                                skip.ptr, skip.cstride, skip.c0, out.ptr, out.cstride, out.c0, npix, c, slope));
      SRGANFD_HIP_CHECK(hipGetLastError());
      return SRGANFD_OK;
    }
  }
  DISPATCH_T(dtype,
             SRGANFD_LAUNCH(lrelu_bwd_kernel<TT>, dim3(grid_for(npix * c)), dim3(256), 0, s, dy.ptr, dy.cstride, dy.c0, act.ptr, act.cstride, act.c0,
                                skip.ptr, skip.cstride, skip.c0, out.ptr, out.cstride, out.c0, npix, c, slope));
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_axpby(srganfd_view x, srganfd_view y, int32_t dtype, int64_t npix64, int32_t c, float a, float b, void* stream) {
  const size_t npix = (size_t)npix64;
  const hipStream_t s = (hipStream_t)stream;
  if (!x.ptr || !y.ptr) return set_err(SRGANFD_EINVAL, "axpby: null");
  if (const char* why = views_bad(npix64, c, {x, y})) return set_err(SRGANFD_EINVAL, "axpby: %s", why);
  {
    const int vn = dtype == SRGANFD_F32 ? 4 : 8;
    auto ok = [&](const srganfd_view& v) { return v.c0 % vn == 0 && v.cstride % vn == 0 && ((uintptr_t)v.ptr & 15) == 0; };
    if (c % vn == 0 && ok(x) && ok(y)) {
      DISPATCH_T(dtype,
                 SRGANFD_LAUNCH(axpby_vec_kernel<TT>, dim3(grid_for(npix * c / vn, 256, 65536)), dim3(256), 0, s, x.ptr, x.cstride, x.c0, y.ptr, y.cstride, y.c0, npix, c, a, b));
      SRGANFD_HIP_CHECK(hipGetLastError());
      return SRGANFD_OK;
    }
  }
  DISPATCH_T(dtype,
             SRGANFD_LAUNCH(axpby_kernel<TT>, dim3(grid_for(npix * c)), dim3(256), 0, s, x.ptr, x.cstride, x.c0, y.ptr, y.cstride, y.c0, npix, c, a, b));
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_add_relu(srganfd_view a, srganfd_view b, srganfd_view out, int32_t dtype, int64_t npix64, int32_t c, void* stream) {
  const size_t npix = (size_t)npix64;
  const hipStream_t s = (hipStream_t)stream;
  if (!a.ptr || !b.ptr || !out.ptr || !vec_ok(dtype, c, {a, b, out})) return set_err(SRGANFD_EINVAL, "add_relu: bad views");
  if (const char* why = views_bad(npix64, c, {a, b, out})) return set_err(SRGANFD_EINVAL, "add_relu: %s", why);
  const int vn = dtype == SRGANFD_F32 ? 4 : 8;
  DISPATCH_T(dtype,
             SRGANFD_LAUNCH(add_relu_kernel<TT>, dim3(grid_for(npix * c / vn, 256, 65536)), dim3(256), 0, s, a.ptr, a.cstride, a.c0, b.ptr, b.cstride, b.c0, out.ptr, out.cstride, out.c0, npix, c));
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_sigmoid(float* x, int64_t numel, void* stream) {
  const size_t n = (size_t)numel;
  const hipStream_t s = (hipStream_t)stream;
  if (!x) return set_err(SRGANFD_EINVAL, "sigmoid: null");
  if (numel <= 0) return set_err(SRGANFD_EINVAL, "sigmoid: numel <= 0");
  SRGANFD_LAUNCH(sigmoid_kernel, dim3(grid_for(n)), dim3(256), 0, s, x, n);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_sigmoid_bwd(const float* ds, const float* sg, float* out, int64_t numel, void* stream) {
  const size_t n = (size_t)numel;
  const hipStream_t s = (hipStream_t)stream;
  if (!ds || !sg || !out) return set_err(SRGANFD_EINVAL, "sigmoid_bwd: null");
  if (numel <= 0) return set_err(SRGANFD_EINVAL, "sigmoid_bwd: numel <= 0");
  SRGANFD_LAUNCH(sigmoid_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, s, ds, sg, out, n);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_gate_mul(int32_t bwd, srganfd_view x, const float* gate, srganfd_view y, srganfd_view dx, float* dgate, int32_t dtype, int64_t npix64,
                                int32_t c, void* stream) {
  const size_t npix = (size_t)npix64;
  const hipStream_t s = (hipStream_t)stream;
  const int vn = dtype == SRGANFD_F32 ? 4 : 8;
  const int cv = c / vn;
  if (!x.ptr || !gate || !y.ptr || !vec_ok(dtype, c, {x, y, dx}) || cv > 64 || (cv & (cv - 1))) return set_err(SRGANFD_EINVAL, "gate_mul: bad args");
  if (const char* why = views_bad(npix64, c, {x, y, dx})) return set_err(SRGANFD_EINVAL, "gate_mul: %s", why);
  if (!bwd) {
    DISPATCH_T(dtype,
               SRGANFD_LAUNCH(gate_fwd_kernel<TT>, dim3(grid_for(npix * cv, 256, 65536)), dim3(256), 0, s, x.ptr, x.cstride, x.c0, gate, y.ptr, y.cstride, y.c0, npix, c));
  } else {
    if (!dx.ptr || !dgate) return set_err(SRGANFD_EINVAL, "gate_mul(bwd): null");
    DISPATCH_T(dtype,
               SRGANFD_LAUNCH(gate_bwd_kernel<TT>, dim3(grid_for(npix * cv, 256, 65536)), dim3(256), 0, s, x.ptr, x.cstride, x.c0, gate, y.ptr, y.cstride, y.c0, dx.ptr, dx.cstride, dx.c0, dgate, npix, c));
  }
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

}  // namespace srganfd
