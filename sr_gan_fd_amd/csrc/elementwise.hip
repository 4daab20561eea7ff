// elementwise.hip -- per-element maps on channel-slice views that are not fused into a conv epilogue: axpby, LeakyReLU backward,
// and the A-ESRGAN attention gate's pieces (relu(a + b), sigmoid and its backward, the gate multiply).  Layout conversion is in
// layout.hip, resampling in resample.hip, losses in loss.hip, spectral norm / BatchNorm in norm.hip, Adam + EMA in optim.hip.
// Every map on views is written once on float[N] (elementwise.hpp): N = VecN<T>::N is its 16-byte vector form, N = 1 its scalar form,
// and vec_ok chooses between them.  The same fp32 operations per element in both: the same bits from both.
#include "elementwise.hpp"

namespace srganfd {

// ---- LeakyReLU backward with the sign recovered from act - skip (skip optional) ----
// out may be dy itself (the engines overwrite the gradient in place), so no pointer is __restrict__: every element is read before it is
// written, by the same lane.
struct LreluK { View dy, act, skip, out; size_t npix; int c; float slope; };
template <typename T, int N>
__global__ __launch_bounds__(256) void lrelu_bwd_kernel(const LreluK k) {
  for_each_group<N>(k.npix, k.c, [&](size_t p, int ch) {
    float g[N], z[N], sk[N];
    ldn<T, N>(k.dy.p, k.dy.at(p, ch), g);
    ldn<T, N>(k.act.p, k.act.at(p, ch), z);
    if (k.skip.p) {
      ldn<T, N>(k.skip.p, k.skip.at(p, ch), sk);
      each<N>([&](int q) { z[q] -= sk[q]; });
    }
    each<N>([&](int q) { g[q] *= z[q] > 0.f ? 1.f : k.slope; });
    stn<T, N>(k.out.p, k.out.at(p, ch), g);
  });
}

// ---- y = a*x + b*y on channel-slice views ----
// Spelled fmaf(a, x, b * y), so that the compiler cannot contract the two widths differently: bit-identical in f32.
// b == 0 never reads y (a NaN there does not reach the result).
struct AxpbyK { View x, y; size_t npix; int c; float a, b; };
template <typename T, int N>
__global__ __launch_bounds__(256) void axpby_kernel(const AxpbyK k) {
  for_each_group<N>(k.npix, k.c, [&](size_t p, int ch) {
    float vx[N];
    ldn<T, N>(k.x.p, k.x.at(p, ch), vx);
    if constexpr (N == 1) {
      // The trainers add their flat fp32 gradients with this form (c = 1, millions of elements): it keeps the load of y inside the
      // expression, as it was first written, and with it the order of its loads and waits (profiles/view_kernels_refactor_isa.txt).
      vx[0] = fmaf(k.a, vx[0], k.b != 0.f ? k.b * ld<T>(k.y.p, k.y.at(p, ch)) : 0.f);
    } else {
      float vy[N];
      if (k.b != 0.f) ldn<T, N>(k.y.p, k.y.at(p, ch), vy);
      each<N>([&](int q) { vx[q] = fmaf(k.a, vx[q], k.b != 0.f ? k.b * vy[q] : 0.f); });
    }
    stn<T, N>(k.y.p, k.y.at(p, ch), vx);
  });
}

// ---- A-ESRGAN attention gates (A-ESRGAN/model.py:239-254): relu(a+b), sigmoid, gate multiply; vector forms only ----
struct AddReluK { View a, b, out; size_t npix; int c; };
template <typename T>
__global__ __launch_bounds__(256) void add_relu_kernel(const AddReluK k) {
  constexpr int N = VecN<T>::N;
  for_each_group<N>(k.npix, k.c, [&](size_t p, int ch) {
    float va[N], vb[N];
    ldv<T>(k.a.p, k.a.at(p, ch), va);
    ldv<T>(k.b.p, k.b.at(p, ch), vb);
    each<N>([&](int q) { va[q] = fmaxf(va[q] + vb[q], 0.f); });
    stv<T>(k.out.p, k.out.at(p, ch), va);
  });
}
__global__ __launch_bounds__(256) void sigmoid_kernel(float* x, size_t n) {
  grid_stride(n, [&](size_t i) { x[i] = 1.f / (1.f + expf(-x[i])); });
}
// out may be ds itself (engine_a overwrites the gradient in place): ds is not __restrict__
__global__ __launch_bounds__(256) void sigmoid_bwd_kernel(const float* ds, const float* __restrict__ s, float* out, size_t n) {
  grid_stride(n, [&](size_t i) { const float v = s[i]; out[i] = ds[i] * v * (1.f - v); });
}
// forward: out[p][c] = gate[p] * x[p][c].  backward: out = dx[p][c] = gate[p] * dy[p][c] ; dgate[p] = sum_c dy[p][c] * x[p][c]
struct GateK { View x, dy, out; const float* gate; float* dgate; size_t npix; int c; };
template <typename T>
__global__ __launch_bounds__(256) void gate_fwd_kernel(const GateK k) {
  constexpr int N = VecN<T>::N;
  for_each_group<N>(k.npix, k.c, [&](size_t p, int ch) {
    float v[N];
    ldv<T>(k.x.p, k.x.at(p, ch), v);
    const float gv = k.gate[p];
    each<N>([&](int q) { v[q] *= gv; });
    stv<T>(k.out.p, k.out.at(p, ch), v);
  });
}
// c/N lanes of a wave per pixel, c/N a power of two <= 64: every lane of a wave takes every trip, so that the shuffles are whole
template <typename T>
__global__ __launch_bounds__(256) void gate_bwd_kernel(const GateK k) {
  constexpr int N = VecN<T>::N;
  const int cv = k.c / N;                     // lanes per pixel
  const size_t total = k.npix * cv;
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
      ldv<T>(k.x.p, k.x.at(p, ch), vx);
      ldv<T>(k.dy.p, k.dy.at(p, ch), vd);
      const float gv = k.gate[p];
      each<N>([&](int q) { part += vd[q] * vx[q]; vd[q] *= gv; });
      stv<T>(k.out.p, k.out.at(p, ch), vd);
    }
    for (int o = cv >> 1; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if (ok && (i % cv) == 0) k.dgate[p] = part;
  }
}

// ------------------------------------------------------------------------------------------------
extern "C" int srganfd_lrelu_bwd(srganfd_view dy, srganfd_view act, srganfd_view skip, srganfd_view out, int32_t dtype, int64_t npix64, int32_t c, float slope,
                                 void* stream) {
  const size_t npix = (size_t)npix64;
  const hipStream_t s = (hipStream_t)stream;
  if (!dy.ptr || !act.ptr || !out.ptr) return set_err(SRGANFD_EINVAL, "lrelu_bwd: null");
  if (const char* why = views_bad(npix64, c, {dy, act, skip, out})) return set_err(SRGANFD_EINVAL, "lrelu_bwd: %s", why);
  const bool vec = vec_ok(dtype, c, {dy, act, skip, out});
  const LreluK k = {dev_view(dy), dev_view(act), dev_view(skip), dev_view(out), npix, c, slope};
  DISPATCH_TN(dtype, vec, SRGANFD_LAUNCH((lrelu_bwd_kernel<TT, NN>), group_grid(npix * c, NN), dim3(256), 0, s, k));
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_axpby(srganfd_view x, srganfd_view y, int32_t dtype, int64_t npix64, int32_t c, float a, float b, void* stream) {
  const size_t npix = (size_t)npix64;
  const hipStream_t s = (hipStream_t)stream;
  if (!x.ptr || !y.ptr) return set_err(SRGANFD_EINVAL, "axpby: null");
  if (const char* why = views_bad(npix64, c, {x, y})) return set_err(SRGANFD_EINVAL, "axpby: %s", why);
  const bool vec = vec_ok(dtype, c, {x, y});
  const AxpbyK k = {dev_view(x), dev_view(y), npix, c, a, b};
  DISPATCH_TN(dtype, vec, SRGANFD_LAUNCH((axpby_kernel<TT, NN>), group_grid(npix * c, NN), dim3(256), 0, s, k));
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_add_relu(srganfd_view a, srganfd_view b, srganfd_view out, int32_t dtype, int64_t npix64, int32_t c, void* stream) {
  const size_t npix = (size_t)npix64;
  const hipStream_t s = (hipStream_t)stream;
  if (!a.ptr || !b.ptr || !out.ptr || !vec_ok(dtype, c, {a, b, out})) return set_err(SRGANFD_EINVAL, "add_relu: bad views");
  if (const char* why = views_bad(npix64, c, {a, b, out})) return set_err(SRGANFD_EINVAL, "add_relu: %s", why);
  const AddReluK k = {dev_view(a), dev_view(b), dev_view(out), npix, c};
  DISPATCH_T(dtype, SRGANFD_LAUNCH(add_relu_kernel<TT>, group_grid(npix * c, vec_width(dtype)), dim3(256), 0, s, k));
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
// forward: y = gate * x.  backward: y carries dy, dx = gate * dy, dgate = sum_c dy * x
extern "C" int srganfd_gate_mul(int32_t bwd, srganfd_view x, const float* gate, srganfd_view y, srganfd_view dx, float* dgate, int32_t dtype, int64_t npix64,
                                int32_t c, void* stream) {
  const size_t npix = (size_t)npix64;
  const hipStream_t s = (hipStream_t)stream;
  const int vn = vec_width(dtype);
  const int cv = c / vn;
  if (!x.ptr || !gate || !y.ptr || !vec_ok(dtype, c, {x, y, dx}) || cv > 64 || (cv & (cv - 1))) return set_err(SRGANFD_EINVAL, "gate_mul: bad args");
  if (const char* why = views_bad(npix64, c, {x, y, dx})) return set_err(SRGANFD_EINVAL, "gate_mul: %s", why);
  if (!bwd) {
    const GateK k = {dev_view(x), {}, dev_view(y), gate, nullptr, npix, c};
    DISPATCH_T(dtype, SRGANFD_LAUNCH(gate_fwd_kernel<TT>, group_grid(npix * c, vn), dim3(256), 0, s, k));
  } else {
    if (!dx.ptr || !dgate) return set_err(SRGANFD_EINVAL, "gate_mul(bwd): null");
    const GateK k = {dev_view(x), dev_view(y), dev_view(dx), gate, dgate, npix, c};
    DISPATCH_T(dtype, SRGANFD_LAUNCH(gate_bwd_kernel<TT>, group_grid(npix * c, vn), dim3(256), 0, s, k));
  }
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

}  // namespace srganfd
