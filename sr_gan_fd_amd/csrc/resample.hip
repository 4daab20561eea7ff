// resample.hip -- 2-D resampling of NHWC views: nearest-x2 backward, bilinear x2 forward and backward (generic and row-grid forms),
// general bilinear resize and its gather-form backward, 2x2 max-pool, the ReLU copy, and max-pool backward with the ReLU's derivative.
// Every x2 op is written once on float[N]: N = VecN<T>::N is its 16-byte vector form, N = 1 its scalar form.
#include "elementwise.hpp"

namespace srganfd {

// what every kernel of this file takes.  x2 ops: a -> b, (h, w) as the ABI states them; act, b2, slope: the fused adjoint's LeakyReLU'
// (below).  resize: (h, w) -> (ho, wo).  maxpool2_relu_bwd: a = x, act = dy, b = dx.  No pointer is __restrict__: the ReLU copy runs in place.
struct RsK { View a, b; int h, w, c, cv_shift; View act, b2; float slope; int n, ho, wo; };

// flat index -> (image, y, x, first channel) over extents (hh, ww) and c / N channel groups; pix = the flat pixel (img * hh + y) * ww + x
struct RsPix { size_t img, pix; int y, x, ch; };
template <int N> __device__ __forceinline__ RsPix rs_decode(size_t i, int hh, int ww, int c) {
  const int cv = c / N;
  RsPix d;
  d.ch = (int)(i % cv) * N;
  size_t p = d.pix = i / cv;
  d.x = (int)(p % ww); p /= ww;
  d.y = (int)(p % hh);
  d.img = p / hh;
  return d;
}
// one weighted tap into an accumulator: the first a product, every later one an explicit fmaf (why: see the row-grid forms below)
template <int N> __device__ __forceinline__ void rs_tap(bool first, float ww, const float* t, float* acc) {
  each<N>([&](int q) { acc[q] = first ? ww * t[q] : fmaf(ww, t[q], acc[q]); });
}

// ---- bilinear x2, align_corners=False (model.py:150,154,158) ----
// dst(2k)   = 0.25*src(k-1) + 0.75*src(k)   (src index clamped to [0, n-1])
// dst(2k+1) = 0.75*src(k)   + 0.25*src(k+1)
__device__ __forceinline__ void bil_taps(int d, int n, int& i0, int& i1, float& w0, float& w1) {
  const int k = d >> 1;
  if (d & 1) { i0 = k; i1 = min(k + 1, n - 1); w0 = 0.75f; w1 = 0.25f; }
  else { i0 = max(k - 1, 0); i1 = k; w0 = 0.25f; w1 = 0.75f; }
}
// adjoint (gather form): low-res pixel k collects high-res 2k-1 .. 2k+2 with (.25, .75, .75, .25); at the borders the clamped taps fold
// into the edge pixel (weight 1) and the out-of-range tap is dropped (on[] = false).
__device__ __forceinline__ void bil_bwd_taps4(int k, int n, int* d, float* wt, bool* on) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int dd = 2 * k - 1 + j;
    on[j] = dd >= 0 && dd < 2 * n;
    d[j] = dd;
    wt[j] = (j == 0 || j == 3) ? 0.25f : 0.75f;
  }
  if (k == 0) wt[1] = 1.0f;
  if (k == n - 1) wt[2] = 1.0f;
}
// the adjoint's two results: b = acc (the U-Net skip's share, model.py:153,157,161; skipped when b is NULL) and, with act != NULL,
// b2 = acc * (act > 0 ? 1 : slope), the LeakyReLU' of the layer whose output was upsampled
template <typename T, int N, bool NT> __device__ __forceinline__ void rs_store_raw_and_masked(const RsK& k, size_t pix, int ch, float* acc) {
  if (k.b.p) stn<T, N, NT>(k.b.p, k.b.at(pix, ch), acc);
  if (k.act.p) {
    float t[N];
    ldn<T, N>(k.act.p, k.act.at(pix, ch), t);
    each<N>([&](int q) { acc[q] *= t[q] > 0.f ? 1.f : k.slope; });
    stn<T, N, NT>(k.b2.p, k.b2.at(pix, ch), acc);
  }
}

// x < 0 ? 0 : x is torch's relu on every input: a NaN stays a NaN (fmaxf would make it 0) and -0 stays -0.
__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }

// ---- the generic forms: op 0 nearest-x2 backward (model.py:372,374: the 2x2 sum), 1 bilinear-x2 forward, 2 bilinear-x2 backward,
// 3 2x2 max-pool (VGG-19; the ReLU before it is in the conv epilogue), 4 the ReLU copy (VGG taps observed pre-ReLU).
// The content loss runs op 4 in place, a and b the same view (engine_v.py).  Every element is read and then written by one thread and
// by no other, so the copy in place gives what the copy out of place gives.
template <typename T, int N, int OP>
__global__ __launch_bounds__(256) void resample_kernel(const RsK k) {
  static_assert(OP >= 0 && OP <= 4 && (N == 1 || N == VecN<T>::N), "five ops, scalar or 16-byte vector");
  const int h = k.h, w = k.w;
  // output extents: op0/2/4 -> (h, w) ; op1 -> (2h, 2w) ; op3 -> (h/2, w/2)
  const int oh = OP == 1 ? 2 * h : (OP == 3 ? h / 2 : h), ow = OP == 1 ? 2 * w : (OP == 3 ? w / 2 : w);
  const size_t total = (size_t)k.n * oh * ow * (k.c / N);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const RsPix d = rs_decode<N>(i, oh, ow, k.c);
    float acc[N], t[N];
    auto load = [&](size_t pixel, float* o) { ldn<T, N>(k.a.p, k.a.at(pixel, d.ch), o); };
    if constexpr (OP == 0 || OP == 3) {   // the 2x2 window of the input in row-major order: summed over (2h, 2w), maxed over (h, w)
      const size_t ih = OP == 0 ? 2 * (size_t)h : h, iw = OP == 0 ? 2 * (size_t)w : w;
      const size_t bq = (d.img * ih + 2 * d.y) * iw + 2 * d.x;
      auto fold = [&](size_t pixel) {
        load(pixel, t);
        each<N>([&](int q) { acc[q] = OP == 0 ? acc[q] + t[q] : fmaxf(acc[q], t[q]); });
      };
      load(bq, acc);
      fold(bq + 1); fold(bq + iw); fold(bq + iw + 1);
    } else if constexpr (OP == 1) {
      int ys[2], xs[2]; float wy[2], wx[2];
      bil_taps(d.y, h, ys[0], ys[1], wy[0], wy[1]);
      bil_taps(d.x, w, xs[0], xs[1], wx[0], wx[1]);
      if constexpr (N == 1) {
        // The scalar form keeps the nested expression it was first written with, not the fmaf chain: the attention gates' one-channel
        // fp32 maps (engine_a.py) are upsampled by it, and the chain moves their last bit (profiles/resample_refactor_ab.txt).
        const size_t r0 = (d.img * h + ys[0]) * w, r1 = (d.img * h + ys[1]) * w;
        auto px = [&](size_t pixel) { return ld<T>(k.a.p, k.a.at(pixel, d.ch)); };
        acc[0] = wy[0] * (wx[0] * px(r0 + xs[0]) + wx[1] * px(r0 + xs[1])) + wy[1] * (wx[0] * px(r1 + xs[0]) + wx[1] * px(r1 + xs[1]));
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          load((d.img * h + ys[j >> 1]) * w + xs[j & 1], t);
          rs_tap<N>(j == 0, wy[j >> 1] * wx[j & 1], t, acc);
        }
      }
    } else if constexpr (OP == 2) {
      int dys[4], dxs[4]; float wys[4], wxs[4]; bool ony[4], onx[4];
      bil_bwd_taps4(d.y, h, dys, wys, ony);
      bil_bwd_taps4(d.x, w, dxs, wxs, onx);
      each<N>([&](int q) { acc[q] = 0.f; });
#pragma unroll
      for (int ia = 0; ia < 4; ++ia)
#pragma unroll
        for (int ib = 0; ib < 4; ++ib)
          if (ony[ia] && onx[ib]) {
            load((d.img * 2 * h + dys[ia]) * 2 * w + dxs[ib], t);
            rs_tap<N>(false, wys[ia] * wxs[ib], t, acc);
          }
    } else {
      load(d.pix, acc);
      each<N>([&](int q) { acc[q] = relu_keep_nan(acc[q]); });
    }
    if constexpr (OP == 2) rs_store_raw_and_masked<T, N, false>(k, d.pix, d.ch, acc);
    else stn<T, N>(k.b.p, k.b.at(d.pix, d.ch), acc);
  }
}

// ---- bilinear x2, row-grid forms: blockIdx.y = group of kBilRows low-res rows, blockIdx.z = image, one thread per
// (low-res column, 16-byte channel vector).  The generic kernel above spends its time on 64-bit div/mod chains and per-thread tap tables;
// here the row taps are wave-uniform, the column taps closed-form, and every address is 32-bit arithmetic on top of one 64-bit row base.
// Same products and the same accumulation order per output as resample_kernel<T, N, 1 / 2>, every step after the first an explicit fmaf
// in both: results are bit-identical.  (Written as `acc += w * t` the compiler fused the steps of one form and, where it could share a
// product between two outputs, not all of the other's: the fp32 forward results then differed in the last bit.)
// Each thread walks kBilRows consecutive low-res rows with a sliding window of source rows in registers: the forward pass reads
// (R + 2) x 3 vectors for 4R stores (2x2 high-res block per low-res pixel), the adjoint (2R + 2) x 4 for R.
static constexpr int kBilRows = 4;
// this thread's (low-res column, first channel), in 32-bit arithmetic; false past the end of the row
template <int N> __device__ __forceinline__ bool rs_column(const RsK& k, int& kx, int& ch) {
  const int cv = k.c / N;
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= (unsigned)(k.w * cv)) return false;
  kx = k.cv_shift >= 0 ? (int)(i >> k.cv_shift) : (int)(i / (unsigned)cv);
  ch = ((int)i - kx * cv) * N;
  return true;
}
template <typename T>
__global__ __launch_bounds__(256) void bilinear_up2_rows_kernel(const RsK k) {
  constexpr int N = VecN<T>::N, R = kBilRows;
  const int h = k.h, w = k.w;
  int kx, ch;
  if (!rs_column<N>(k, kx, ch)) return;
  const int ky0 = blockIdx.y * R;
  const size_t img = blockIdx.z;
  const int xs[3] = {max(kx - 1, 0), kx, min(kx + 1, w - 1)};
  float t[3][3][N];                                         // window slot (row - ky0 + 1) % 3
  auto load_row = [&](float (*dst)[N], int y) {
    const size_t row = (img * h + y) * (size_t)w;
#pragma unroll
    for (int q = 0; q < 3; ++q) ldv<T>(k.a.p, k.a.at(row + xs[q], ch), dst[q]);
  };
  load_row(t[0], max(ky0 - 1, 0));
  load_row(t[1], ky0);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int ky = ky0 + r;
    if (ky >= h) break;                                     // wave-uniform
    load_row(t[(r + 2) % 3], min(ky + 1, h - 1));
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      // even output row: taps (k-1: .25, k: .75); odd: (k: .75, k+1: .25)
      const int rr[2] = {(r + dy) % 3, (r + dy + 1) % 3};
      const float wy[2] = {dy ? 0.75f : 0.25f, dy ? 0.25f : 0.75f};
      const size_t orow = (img * 2 * h + 2 * ky + dy) * (size_t)(2 * w) + 2 * kx;
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const float wx[2] = {dx ? 0.75f : 0.25f, dx ? 0.25f : 0.75f};
        float acc[N];
#pragma unroll
        for (int j = 0; j < 4; ++j) rs_tap<N>(j == 0, wy[j >> 1] * wx[j & 1], t[rr[j >> 1]][dx + (j & 1)], acc);
        // non-temporal: 142 -> 107 us (512 channels, 64^2 -> 128^2), 268 -> 199 us (256 channels), 525 -> 505 us (128 channels), bit-equal outputs
        stv_nt<T>(k.b.p, k.b.at(orow + dx, ch), acc);
      }
    }
  }
}
template <typename T, bool NT>
__global__ __launch_bounds__(256) void bilinear_up2_bwd_rows_kernel(const RsK k) {
  constexpr int N = VecN<T>::N, R = kBilRows;
  const int h = k.h, w = k.w;
  int kx, ch;
  if (!rs_column<N>(k, kx, ch)) return;
  const int ky0 = blockIdx.y * R;
  const size_t img = blockIdx.z;
  int dxs[4]; float wxs[4]; bool onx[4];
  bil_bwd_taps4(kx, w, dxs, wxs, onx);
  u32x4 win[4][4];                                          // high-res row 2*ky0 - 1 + m lives in slot m % 4, as loaded (16 bytes per tap)
  auto load_row = [&](u32x4* dst, int d) {
    if (d < 0 || d >= 2 * h) return;                        // wave-uniform
    const size_t row = (img * 2 * h + d) * (size_t)(2 * w);
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
      if (onx[ib]) dst[ib] = ldraw<T>(k.a.p, k.a.at(row + dxs[ib], ch));
  };
  load_row(win[0], 2 * ky0 - 1);
  load_row(win[1], 2 * ky0);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int ky = ky0 + r;
    if (ky >= h) break;                                     // wave-uniform
    load_row(win[(2 * r + 2) % 4], 2 * ky + 1);
    load_row(win[(2 * r + 3) % 4], 2 * ky + 2);
    int dys[4]; float wys[4]; bool ony[4];
    bil_bwd_taps4(ky, h, dys, wys, ony);
    float acc[N], t[N];
    each<N>([&](int q) { acc[q] = 0.f; });
#pragma unroll
    for (int ia = 0; ia < 4; ++ia) {
      if (!ony[ia]) continue;                               // wave-uniform
#pragma unroll
      for (int ib = 0; ib < 4; ++ib) {
        if (onx[ib]) {
          widen<T>(win[(2 * r + ia) % 4][ib], t);
          rs_tap<N>(false, wys[ia] * wxs[ib], t, acc);
        }
      }
    }
    rs_store_raw_and_masked<T, N, NT>(k, (img * h + ky) * (size_t)w + kx, ch, acc);
  }
}

// ---- general bilinear resize (the A-ESRGAN attention gates, A-ESRGAN/model.py:239-254) ----
// F.interpolate(mode="bilinear", align_corners=False) with an explicit output size (ATen area_pixel source index)
__device__ __forceinline__ void resize_taps(int d, int in, float scale, int& i0, int& i1, float& w0, float& w1) {
  float src = scale * ((float)d + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  w1 = src - (float)i0;
  w0 = 1.f - w1;
}
template <typename T>
__global__ __launch_bounds__(256) void resize_fwd_kernel(const RsK k) {
  constexpr int N = VecN<T>::N;
  const int hi = k.h, wi = k.w, ho = k.ho, wo = k.wo;
  const float sy = (float)hi / (float)ho, sx = (float)wi / (float)wo;
  const size_t total = (size_t)k.n * ho * wo * (k.c / N);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const RsPix d = rs_decode<N>(i, ho, wo, k.c);
    int ya, yb, xa, xb; float wya, wyb, wxa, wxb;
    resize_taps(d.y, hi, sy, ya, yb, wya, wyb);
    resize_taps(d.x, wi, sx, xa, xb, wxa, wxb);
    float acc[N], t[N];
    ldv<T>(k.a.p, k.a.at((d.img * hi + ya) * wi + xa, d.ch), t);
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] = wya * wxa * t[q];
    ldv<T>(k.a.p, k.a.at((d.img * hi + ya) * wi + xb, d.ch), t);
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] += wya * wxb * t[q];
    ldv<T>(k.a.p, k.a.at((d.img * hi + yb) * wi + xa, d.ch), t);
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] += wyb * wxa * t[q];
    ldv<T>(k.a.p, k.a.at((d.img * hi + yb) * wi + xb, d.ch), t);
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] += wyb * wxb * t[q];
    stv<T>(k.b.p, k.b.at(d.pix, d.ch), acc);
  }
}
// backward as a deterministic gather: input pixel k collects every output pixel whose two taps include k
__device__ __forceinline__ int resize_bwd_range(int k, int in, int out, float scale, int& lo) {
  // outputs d with src(d) in (k-1, k+1): d in ((k-0.5)/scale - 0.5 - 1, (k+1.5)/scale - 0.5 + 1)
  int l = (int)floorf(((float)k - 0.5f) / scale - 0.5f) - 1, h = (int)ceilf(((float)k + 1.5f) / scale - 0.5f) + 1;
  if (k == 0) l = 0;   // clamped sources
  if (l < 0) l = 0;
  if (h > out - 1) h = out - 1;
  lo = l;
  return h;
}
template <typename T>
__global__ __launch_bounds__(256) void resize_bwd_kernel(const RsK k) {   // a = dy (ho x wo), b = dx (h x w)
  constexpr int N = VecN<T>::N;
  const int hi = k.h, wi = k.w, ho = k.ho, wo = k.wo;
  const float sy = (float)hi / (float)ho, sx = (float)wi / (float)wo;
  const size_t total = (size_t)k.n * hi * wi * (k.c / N);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const RsPix d = rs_decode<N>(i, hi, wi, k.c);
    int ylo, xlo;
    const int yhi = resize_bwd_range(d.y, hi, ho, sy, ylo), xhi = resize_bwd_range(d.x, wi, wo, sx, xlo);
    float acc[N], t[N];
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
      int ya, yb; float wya, wyb;
      resize_taps(oy, hi, sy, ya, yb, wya, wyb);
      const float wy = (ya == d.y ? wya : 0.f) + (yb == d.y ? wyb : 0.f);
      if (wy == 0.f) continue;
      for (int ox = xlo; ox <= xhi; ++ox) {
        int xa, xb; float wxa, wxb;
        resize_taps(ox, wi, sx, xa, xb, wxa, wxb);
        const float wx = (xa == d.x ? wxa : 0.f) + (xb == d.x ? wxb : 0.f);
        if (wx == 0.f) continue;
        ldv<T>(k.a.p, k.a.at((d.img * ho + oy) * wo + ox, d.ch), t);
        const float ww = wy * wx;
#pragma unroll
        for (int q = 0; q < N; ++q) acc[q] += ww * t[q];
      }
    }
    stv<T>(k.b.p, k.b.at(d.pix, d.ch), acc);
  }
}

// ---- max-pool backward with the preceding ReLU's derivative folded in (differentiable VGG tap, ESRGAN/model.py:281-292) ----
// x: pre-pool activation (a ReLU output), dy: gradient of the pooled map, dx: gradient w.r.t. the ReLU's INPUT.
// The gradient goes to the first maximum of each 2x2 window in row-major order (ATen max_pool2d) and is zero where
// that maximum is not positive (ReLU').
template <typename T>
__global__ __launch_bounds__(256) void maxpool2_relu_bwd_kernel(const RsK k) {
  const View &x = k.a, &dy = k.act, &dx = k.b;
  const int h = k.h, w = k.w, ho = h / 2, wo = w / 2;
  const size_t total = (size_t)k.n * ho * wo * k.c;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const RsPix d = rs_decode<1>(i, ho, wo, k.c);
    const size_t b = (d.img * h + 2 * d.y) * w + 2 * d.x;
    const size_t q[4] = {b, b + 1, b + w, b + w + 1};
    float best = ld<T>(x.p, x.at(q[0], d.ch));
    int arg = 0;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      const float v = ld<T>(x.p, x.at(q[j], d.ch));
      if (v > best) { best = v; arg = j; }
    }
    const float g = best > 0.f ? ld<T>(dy.p, dy.at(d.pix, d.ch)) : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) st<T>(dx.p, dx.at(q[j], d.ch), j == arg ? g : 0.f);
  }
}

// ------------------------------------------------------------------------------------------------
// host side.  An instantiation per dtype and its label side by side: a launch and srganfd_resample_describe read the same table entry.
struct RsKernel { int op; bool vec, rows, nt; void (*fn[3])(const RsK); const char* label; };   // fn: bf16, f16, f32
template <typename T, bool VEC> constexpr int kRsWidth = VEC ? VecN<T>::N : 1;
template <int OP, bool VEC> static RsKernel rs_generic(const char* label) {
  return {OP, VEC, false, false, {resample_kernel<bf16_t, kRsWidth<bf16_t, VEC>, OP>, resample_kernel<f16_t, kRsWidth<f16_t, VEC>, OP>, resample_kernel<float, kRsWidth<float, VEC>, OP>}, label};
}
static const RsKernel kResample[] = {      // keyed by (op, vector, row grid, non-temporal)
    rs_generic<0, false>("resample_kernel<op0,scalar>"), rs_generic<0, true>("resample_kernel<op0,vec>"),
    rs_generic<1, false>("resample_kernel<op1,scalar>"), rs_generic<1, true>("resample_kernel<op1,vec>"),
    rs_generic<2, false>("resample_kernel<op2,scalar>"), rs_generic<2, true>("resample_kernel<op2,vec>"),
    rs_generic<3, false>("resample_kernel<op3,scalar>"), rs_generic<3, true>("resample_kernel<op3,vec>"),
    rs_generic<4, false>("resample_kernel<op4,scalar>"), rs_generic<4, true>("resample_kernel<op4,vec>"),
    {1, true, true, false, {bilinear_up2_rows_kernel<bf16_t>, bilinear_up2_rows_kernel<f16_t>, bilinear_up2_rows_kernel<float>}, "bilinear_up2_rows_kernel"},
    {2, true, true, false, {bilinear_up2_bwd_rows_kernel<bf16_t, false>, bilinear_up2_bwd_rows_kernel<f16_t, false>, bilinear_up2_bwd_rows_kernel<float, false>}, "bilinear_up2_bwd_rows_kernel"},
    {2, true, true, true, {bilinear_up2_bwd_rows_kernel<bf16_t, true>, bilinear_up2_bwd_rows_kernel<f16_t, true>, bilinear_up2_bwd_rows_kernel<float, true>}, "bilinear_up2_bwd_rows_kernel<NT>"}};
static const RsKernel kResize[2] = {{0, true, false, false, {resize_fwd_kernel<bf16_t>, resize_fwd_kernel<f16_t>, resize_fwd_kernel<float>}, "resize_fwd_kernel"},
                                    {1, true, false, false, {resize_bwd_kernel<bf16_t>, resize_bwd_kernel<f16_t>, resize_bwd_kernel<float>}, "resize_bwd_kernel"}};
static const RsKernel kMaxpoolBwd = {0, false, false, false, {maxpool2_relu_bwd_kernel<bf16_t>, maxpool2_relu_bwd_kernel<f16_t>, maxpool2_relu_bwd_kernel<float>}, "maxpool2_relu_bwd_kernel"};

// launches kn for the dtype, or writes "<label>/<dtype>" where srganfd_resample_describe asked for it
static int rs_launch(const RsKernel& kn, int dtype, dim3 grid, hipStream_t s, const RsK& k) {
  const int t = dtype == SRGANFD_BF16 ? 0 : dtype == SRGANFD_F16 ? 1 : dtype == SRGANFD_F32 ? 2 : -1;
  if (t < 0) return set_err(SRGANFD_EINVAL, "bad dtype %d", dtype);
  static const char* const names[3] = {"bf16", "f16", "f32"};
  if (g_describe) { snprintf(g_describe, g_describe_len, "%s/%s", kn.label, names[t]); return SRGANFD_OK; }
  SRGANFD_LAUNCH(kn.fn[t], grid, dim3(256), 0, s, k);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

// the x2 ops' dispatch.  may_nt: the fused entry's results may leave through non-temporal stores.
static int rs_dispatch(int op, bool vec, bool may_nt, int dtype, RsK& k, hipStream_t s) {
  const int vn = !vec ? 1 : vec_width(dtype), esize = dtype == SRGANFD_F32 ? 4 : 2;
  const size_t lo = (size_t)k.n * k.h * k.w * k.c;
  // row-grid forms of the two bilinear ops, grid (column blocks, groups of low-res rows, images): a grid's y and z extents end at 65535,
  // and the column decode is 32-bit
  const int cv = k.c / vn;
  const bool rows = vec && (op == 1 || op == 2) && k.h <= 65535 && k.n <= 65535 && (size_t)k.w * cv < (1u << 31);
  // non-temporal stores for results one pass cannot keep in the 256 MiB Infinity Cache anyway: 867 -> 805 us (128 channels, 512^2 -> 256^2, batch 32),
  // 427 -> 414 (256 channels), bit-equal; 8 / 16 rows per thread instead of 4 measured 3-10 % slower (the bwd+ rows of tools/rsbench.py)
  const bool nt = rows && may_nt && lo * esize >= ((size_t)192 << 20);
  dim3 grid;
  if (rows) {
    k.cv_shift = (cv & (cv - 1)) == 0 ? __builtin_ctz(cv) : -1;
    grid = dim3((unsigned)(((size_t)k.w * cv + 255) / 256), (unsigned)((k.h + kBilRows - 1) / kBilRows), (unsigned)k.n);
  } else {
    grid = group_grid(op == 1 ? lo * 4 : op == 3 ? lo / 4 : lo, vn);
  }
  for (const RsKernel& kn : kResample)
    if (kn.op == op && kn.vec == vec && kn.rows == rows && kn.nt == nt) return rs_launch(kn, dtype, grid, s, k);
  return set_err(SRGANFD_EINVAL, "resample: bad op %d", op);
}

// op: 0 nearest-x2 backward, 1 bilinear-x2 forward, 2 bilinear-x2 backward, 3 maxpool2, 4 ReLU copy ; (h, w) = low-res dims (ops 3, 4: input dims)
extern "C" int srganfd_resample(int32_t op, srganfd_view a, srganfd_view b, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, void* stream) {
  if (!a.ptr || !b.ptr) return set_err(SRGANFD_EINVAL, "resample: null view");
  if (const char* bad = views_bad(c, {a, b})) return set_err(SRGANFD_EINVAL, "resample: %s", bad);
  RsK k = {dev_view(a), dev_view(b), h, w, c, 0, {}, {}, 0.f, n, 0, 0};
  return rs_dispatch(op, vec_ok(dtype, c, {a, b}), false, dtype, k, (hipStream_t)stream);
}
// bilinear-x2 backward fused with the LeakyReLU' of the upsampled layer: dx_raw (optional) = adjoint of the upsampling applied to dy,
// dx_masked = dx_raw * (act > 0 ? 1 : slope).  16-byte-vectorised views only (the discriminators' channel counts).
extern "C" int srganfd_resample_bwd_lrelu(srganfd_view dy, srganfd_view dx_raw, srganfd_view act, srganfd_view dx_masked, int32_t dtype, int32_t n, int32_t h,
                                          int32_t w, int32_t c, float slope, void* stream) {
  if (!dy.ptr || !act.ptr || !dx_masked.ptr) return set_err(SRGANFD_EINVAL, "resample_bwd_lrelu: null view");
  if (const char* bad = views_bad(c, {dy, dx_raw, act, dx_masked})) return set_err(SRGANFD_EINVAL, "resample_bwd_lrelu: %s", bad);
  if (!vec_ok(dtype, c, {dy, dx_raw, act, dx_masked})) return set_err(SRGANFD_EINVAL, "resample_bwd_lrelu: views must be 16-byte aligned NHWC slices");
  RsK k = {dev_view(dy), dev_view(dx_raw), h, w, c, 0, dev_view(act), dev_view(dx_masked), slope, n, 0, 0};
  return rs_dispatch(2, true, true, dtype, k, (hipStream_t)stream);
}
// entry 0: srganfd_resample(op, a, b) ; entry 1: srganfd_resample_bwd_lrelu(dy = a, dx_raw = b, act = act, dx_masked = b2).  Writes the
// label of the instantiation that call launches, "<kernel>/<dtype>", or refuses as that call does; launches nothing.
extern "C" int srganfd_resample_describe(int32_t entry, int32_t op, srganfd_view a, srganfd_view b, srganfd_view act, srganfd_view b2, int32_t dtype, int32_t n,
                                         int32_t h, int32_t w, int32_t c, char* out, size_t out_len) {
  if (!out || !out_len) return set_err(SRGANFD_EINVAL, "resample_describe: no buffer");
  if (entry < 0 || entry > 1) return set_err(SRGANFD_EINVAL, "resample_describe: entry %d is none of 0 (resample), 1 (resample_bwd_lrelu)", entry);
  out[0] = 0;
  g_describe = out; g_describe_len = out_len;
  const int rc = entry == 0 ? srganfd_resample(op, a, b, dtype, n, h, w, c, nullptr) : srganfd_resample_bwd_lrelu(a, b, act, b2, dtype, n, h, w, c, 0.f, nullptr);
  g_describe = nullptr; g_describe_len = 0;
  return rc;
}
extern "C" int srganfd_resize_bilinear(int32_t bwd, srganfd_view a, srganfd_view b, int32_t dtype, int32_t n, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                                       int32_t c, void* stream) {
  if (!a.ptr || !b.ptr || !vec_ok(dtype, c, {a, b})) return set_err(SRGANFD_EINVAL, "resize_bilinear: views must be 16-byte aligned channel multiples");
  if (const char* bad = views_bad(c, {a, b})) return set_err(SRGANFD_EINVAL, "resize_bilinear: %s", bad);
  RsK k = {dev_view(a), dev_view(b), hi, wi, c, 0, {}, {}, 0.f, n, ho, wo};
  const size_t total = bwd ? (size_t)n * hi * wi * c : (size_t)n * ho * wo * c;
  return rs_launch(kResize[bwd ? 1 : 0], dtype, group_grid(total, vec_width(dtype)), (hipStream_t)stream, k);
}
extern "C" int srganfd_maxpool2_relu_bwd(srganfd_view x, srganfd_view dy, srganfd_view dx, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c,
                                         void* stream) {
  if (!x.ptr || !dy.ptr || !dx.ptr || n <= 0 || h <= 0 || w <= 0 || (h & 1) || (w & 1)) return set_err(SRGANFD_EINVAL, "maxpool2_relu_bwd: bad args");
  if (const char* bad = views_bad(c, {x, dy, dx})) return set_err(SRGANFD_EINVAL, "maxpool2_relu_bwd: %s", bad);
  RsK k = {dev_view(x), dev_view(dx), h, w, c, 0, dev_view(dy), {}, 0.f, n, 0, 0};
  return rs_launch(kMaxpoolBwd, dtype, group_grid((size_t)n * (h / 2) * (w / 2) * c, 1), (hipStream_t)stream, k);
}

}  // namespace srganfd
