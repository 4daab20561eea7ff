// resample.hip -- 2-D resampling of NHWC views: nearest-x2 backward, bilinear x2 forward and backward (generic and row-grid forms),
// general bilinear resize and its gather-form backward, 2x2 max-pool, the ReLU copy, and max-pool backward with the ReLU's derivative.
#include "elementwise.hpp"

namespace srganfd {

// generic 2-D resampling on vectors: op 0 nearest-x2 backward, 1 bilinear-x2 forward, 2 bilinear-x2 backward, 3 maxpool2 (op 4, the ReLU
// copy, has relu_copy_vec_kernel below: it runs in place, which this kernel's __restrict__ input rules out)
__device__ __forceinline__ void bil_taps(int d, int n, int& i0, int& i1, float& w0, float& w1);
__device__ __forceinline__ int bil_bwd_taps(int k, int n, int* d, float* wt);

// OP 2 only: act != NULL also writes b2 = result * (act > 0 ? 1 : slope) (LeakyReLU' of the layer whose output was upsampled: the
// raw gradient b is the U-Net skip's share, model.py:153,157,161; b may be NULL when only the masked one is wanted)
template <typename T, int OP>
__global__ __launch_bounds__(256) void resample_vec_kernel(const void* __restrict__ a, int aC, int a0, void* b, int bC, int b0, int n, int h, int w, int c,
                                                           const void* __restrict__ act = nullptr, int actC = 0, int act0 = 0, void* b2 = nullptr, int b2C = 0,
                                                           int b20 = 0, float slope = 0.f) {
  constexpr int N = VecN<T>::N;
  const int cv = c / N;
  static_assert(OP >= 0 && OP <= 3, "op 4 is relu_copy_vec_kernel");
  // output extents: op0/2 -> (h, w) low-res ; op1 -> (2h, 2w) ; op3 -> (h/2, w/2)
  const int oh = OP == 1 ? 2 * h : (OP == 3 ? h / 2 : h), ow = OP == 1 ? 2 * w : (OP == 3 ? w / 2 : w);
  const size_t total = (size_t)n * oh * ow * cv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % cv) * N;
    size_t p = i / cv;
    const int ox = (int)(p % ow); p /= ow;
    const int oy = (int)(p % oh);
    const size_t img = p / oh;
    float acc[N], t[N];
    if constexpr (OP == 0) {          // sum of the 2x2 high-res pixels
      const size_t bq = (img * 2 * h + 2 * oy) * 2 * w + 2 * ox;
      ldv<T>(a, bq * aC + a0 + ch, acc);
      ldv<T>(a, (bq + 1) * aC + a0 + ch, t);
#pragma unroll
      for (int q = 0; q < N; ++q) acc[q] += t[q];
      ldv<T>(a, (bq + 2 * w) * aC + a0 + ch, t);
#pragma unroll
      for (int q = 0; q < N; ++q) acc[q] += t[q];
      ldv<T>(a, (bq + 2 * w + 1) * aC + a0 + ch, t);
#pragma unroll
      for (int q = 0; q < N; ++q) acc[q] += t[q];
    } else if constexpr (OP == 1) {   // bilinear forward
      int ya, yb, xa, xb; float wya, wyb, wxa, wxb;
      bil_taps(oy, h, ya, yb, wya, wyb);
      bil_taps(ox, w, xa, xb, wxa, wxb);
      const size_t r0 = (img * h + ya) * w, r1 = (img * h + yb) * w;
      ldv<T>(a, (r0 + xa) * aC + a0 + ch, t);
#pragma unroll
      for (int q = 0; q < N; ++q) acc[q] = wya * wxa * t[q];
      ldv<T>(a, (r0 + xb) * aC + a0 + ch, t);
#pragma unroll
      for (int q = 0; q < N; ++q) acc[q] = fmaf(wya * wxb, t[q], acc[q]);
      ldv<T>(a, (r1 + xa) * aC + a0 + ch, t);
#pragma unroll
      for (int q = 0; q < N; ++q) acc[q] = fmaf(wyb * wxa, t[q], acc[q]);
      ldv<T>(a, (r1 + xb) * aC + a0 + ch, t);
#pragma unroll
      for (int q = 0; q < N; ++q) acc[q] = fmaf(wyb * wxb, t[q], acc[q]);
    } else if constexpr (OP == 2) {   // bilinear backward (gather form)
      int dys[6], dxs[6]; float wys[6], wxs[6];
      const int ny = bil_bwd_taps(oy, h, dys, wys), nx = bil_bwd_taps(ox, w, dxs, wxs);
#pragma unroll
      for (int q = 0; q < N; ++q) acc[q] = 0.f;
      for (int ia = 0; ia < ny; ++ia)
        for (int ib = 0; ib < nx; ++ib) {
          ldv<T>(a, ((img * 2 * h + dys[ia]) * 2 * w + dxs[ib]) * aC + a0 + ch, t);
          const float ww = wys[ia] * wxs[ib];
#pragma unroll
          for (int q = 0; q < N; ++q) acc[q] = fmaf(ww, t[q], acc[q]);
        }
    } else {                           // 2x2 max pool
      const size_t bq = (img * h + 2 * oy) * w + 2 * ox;
      ldv<T>(a, bq * aC + a0 + ch, acc);
      ldv<T>(a, (bq + 1) * aC + a0 + ch, t);
#pragma unroll
      for (int q = 0; q < N; ++q) acc[q] = fmaxf(acc[q], t[q]);
      ldv<T>(a, (bq + w) * aC + a0 + ch, t);
#pragma unroll
      for (int q = 0; q < N; ++q) acc[q] = fmaxf(acc[q], t[q]);
      ldv<T>(a, (bq + w + 1) * aC + a0 + ch, t);
#pragma unroll
      for (int q = 0; q < N; ++q) acc[q] = fmaxf(acc[q], t[q]);
    }
    if constexpr (OP == 2) {
      const size_t op_ = (img * oh + oy) * ow + ox;
      if (b) stv<T>(b, op_ * (size_t)bC + b0 + ch, acc);
      if (act) {
        ldv<T>(act, op_ * (size_t)actC + act0 + ch, t);
#pragma unroll
        for (int q = 0; q < N; ++q) acc[q] *= t[q] > 0.f ? 1.f : slope;
        stv<T>(b2, op_ * (size_t)b2C + b20 + ch, acc);
      }
    } else {
      stv<T>(b, ((img * oh + oy) * ow + ox) * (size_t)bC + b0 + ch, acc);
    }
  }
}

// ---- bilinear x2 (align_corners=False, model.py:150-158), row-grid forms: blockIdx.y = group of kBilRows low-res rows, blockIdx.z = image, one thread per
// (low-res column, 16-byte channel vector).  The generic kernel above spends its time on 64-bit div/mod chains and per-thread tap tables;
// here the row taps are wave-uniform, the column taps closed-form, and every address is 32-bit arithmetic on top of one 64-bit row base.
// Same products and the same accumulation order per output as resample_vec_kernel<T, 1 / 2>, every step after the first an explicit fmaf
// in both: results are bit-identical.  (Written as `acc += w * t` the compiler fused the steps of one form and, where it could share a
// product between two outputs, not all of the other's: the fp32 forward results then differed in the last bit.)
// Each thread walks kBilRows consecutive low-res rows with a sliding window of source rows in registers: the forward pass reads
// (R + 2) x 3 vectors for 4R stores (2x2 high-res block per low-res pixel), the adjoint (2R + 2) x 4 for R.
static constexpr int kBilRows = 4;
template <typename T>
__global__ __launch_bounds__(256) void bilinear_up2_block_kernel(const void* __restrict__ a, int aC, int a0, void* b, int bC, int b0, int h, int w, int c, int cv_shift) {
  constexpr int N = VecN<T>::N, R = kBilRows;
  const int cv = c / N;
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= (unsigned)(w * cv)) return;
  const int kx = cv_shift >= 0 ? (int)(i >> cv_shift) : (int)(i / (unsigned)cv), ch = ((int)i - kx * cv) * N;
  const int ky0 = blockIdx.y * R;
  const size_t img = blockIdx.z;
  const int xs[3] = {max(kx - 1, 0), kx, min(kx + 1, w - 1)};
  float t[3][3][N];                                         // window slot (row - ky0 + 1) % 3
  auto load_row = [&](float (*dst)[N], int y) {
    const size_t row = (img * h + y) * (size_t)w;
#pragma unroll
    for (int q = 0; q < 3; ++q) ldv<T>(a, (row + xs[q]) * aC + a0 + ch, dst[q]);
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
      const int ra = (r + dy) % 3, rb = (r + dy + 1) % 3;
      const float wya = dy ? 0.75f : 0.25f, wyb = dy ? 0.25f : 0.75f;
      const size_t orow = (img * 2 * h + 2 * ky + dy) * (size_t)(2 * w) + 2 * kx;
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int qa = dx, qb = dx + 1;
        const float wxa = dx ? 0.75f : 0.25f, wxb = dx ? 0.25f : 0.75f;
        float acc[N];
#pragma unroll
        for (int q = 0; q < N; ++q) acc[q] = wya * wxa * t[ra][qa][q];
#pragma unroll
        for (int q = 0; q < N; ++q) acc[q] = fmaf(wya * wxb, t[ra][qb][q], acc[q]);
#pragma unroll
        for (int q = 0; q < N; ++q) acc[q] = fmaf(wyb * wxa, t[rb][qa][q], acc[q]);
#pragma unroll
        for (int q = 0; q < N; ++q) acc[q] = fmaf(wyb * wxb, t[rb][qb][q], acc[q]);
        // non-temporal: 142 -> 107 us (512 channels, 64^2 -> 128^2), 268 -> 199 us (256 channels), 525 -> 505 us (128 channels), bit-equal outputs
        stv_nt<T>(b, (orow + dx) * (size_t)bC + b0 + ch, acc);
      }
    }
  }
}
// adjoint (gather form): low-res pixel k collects high-res 2k-1 .. 2k+2 with (.25, .75, .75, .25); at the borders the clamped taps fold
// into the edge pixel (weight 1) and the out-of-range tap is dropped -- the table bil_bwd_taps builds, in closed form.
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
template <typename T, int R = kBilRows, bool NT = false>
__global__ __launch_bounds__(256) void bilinear_up2_bwd_rows_kernel(const void* __restrict__ a, int aC, int a0, void* b, int bC, int b0, int h, int w, int c, int cv_shift,
                                                                    const void* __restrict__ act, int actC, int act0, void* b2, int b2C, int b20, float slope) {
  constexpr int N = VecN<T>::N;
  const int cv = c / N;
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= (unsigned)(w * cv)) return;
  const int kx = cv_shift >= 0 ? (int)(i >> cv_shift) : (int)(i / (unsigned)cv), ch = ((int)i - kx * cv) * N;
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
      if (onx[ib]) dst[ib] = ldraw<T>(a, (row + dxs[ib]) * aC + a0 + ch);
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
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] = 0.f;
#pragma unroll
    for (int ia = 0; ia < 4; ++ia) {
      if (!ony[ia]) continue;                               // wave-uniform
#pragma unroll
      for (int ib = 0; ib < 4; ++ib) {
        if (onx[ib]) {
          widen<T>(win[(2 * r + ia) % 4][ib], t);
          const float ww = wys[ia] * wxs[ib];
#pragma unroll
          for (int q = 0; q < N; ++q) acc[q] = fmaf(ww, t[q], acc[q]);
        }
      }
    }
    const size_t op_ = (img * h + ky) * (size_t)w + kx;
    if (b) { if constexpr (NT) stv_nt<T>(b, op_ * (size_t)bC + b0 + ch, acc); else stv<T>(b, op_ * (size_t)bC + b0 + ch, acc); }
    if (act) {
      ldv<T>(act, op_ * (size_t)actC + act0 + ch, t);
#pragma unroll
      for (int q = 0; q < N; ++q) acc[q] *= t[q] > 0.f ? 1.f : slope;
      if constexpr (NT) stv_nt<T>(b2, op_ * (size_t)b2C + b20 + ch, acc); else stv<T>(b2, op_ * (size_t)b2C + b20 + ch, acc);
    }
  }
}

// ---- backward of F.interpolate(scale_factor=2, mode="nearest") (model.py:372,374): 2x2 sum ----
template <typename T>
__global__ void up2_nearest_bwd_kernel(const void* __restrict__ dy, int yC, int y0, void* dx, int xC, int x0, int n, int h, int w, int c) {
  const size_t total = (size_t)n * h * w * c;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % c);
    size_t p = i / c;
    const int x = (int)(p % w); p /= w;
    const int y = (int)(p % h);
    const size_t img = p / h;
    const size_t b = ((img * 2 * h + 2 * y) * 2 * w + 2 * x);
    const float s = ld<T>(dy, b * yC + y0 + ch) + ld<T>(dy, (b + 1) * yC + y0 + ch) + ld<T>(dy, (b + 2 * w) * yC + y0 + ch) +
                    ld<T>(dy, (b + 2 * w + 1) * yC + y0 + ch);
    st<T>(dx, (i / c) * xC + x0 + ch, s);
  }
}

// ---- bilinear x2, align_corners=False (model.py:150,154,158) forward and backward ----
// dst(2k)   = 0.25*src(k-1) + 0.75*src(k)   (src index clamped to [0, n-1])
// dst(2k+1) = 0.75*src(k)   + 0.25*src(k+1)
__device__ __forceinline__ void bil_taps(int d, int n, int& i0, int& i1, float& w0, float& w1) {
  const int k = d >> 1;
  if (d & 1) { i0 = k; i1 = min(k + 1, n - 1); w0 = 0.75f; w1 = 0.25f; }
  else { i0 = max(k - 1, 0); i1 = k; w0 = 0.25f; w1 = 0.75f; }
}
template <typename T>
__global__ void up2_bilinear_fwd_kernel(const void* __restrict__ x, int xC, int x0, void* y, int yC, int y0, int n, int h, int w, int c) {
  const size_t total = (size_t)n * 4 * h * w * c;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % c);
    size_t p = i / c;
    const int ox = (int)(p % (2 * w)); p /= (2 * w);
    const int oy = (int)(p % (2 * h));
    const size_t img = p / (2 * h);
    int ya, yb, xa, xb; float wya, wyb, wxa, wxb;
    bil_taps(oy, h, ya, yb, wya, wyb);
    bil_taps(ox, w, xa, xb, wxa, wxb);
    const size_t r0 = (img * h + ya) * w, r1 = (img * h + yb) * w;
    const float v = wya * (wxa * ld<T>(x, (r0 + xa) * xC + x0 + ch) + wxb * ld<T>(x, (r0 + xb) * xC + x0 + ch)) +
                    wyb * (wxa * ld<T>(x, (r1 + xa) * xC + x0 + ch) + wxb * ld<T>(x, (r1 + xb) * xC + x0 + ch));
    st<T>(y, (i / c) * yC + y0 + ch, v);
  }
}
// gather form of the transpose: src pixel k receives from dst 2k-1 (0.25), 2k (0.75), 2k+1 (0.75), 2k+2 (0.25),
// plus the clamped border contributions (dst 0 -> src 0 with the 0.25 that would go to src -1; same at the top).
__device__ __forceinline__ int bil_bwd_taps(int k, int n, int* d, float* wt) {
  int cnt = 0;
  for (int dd = 2 * k - 2; dd <= 2 * k + 3; ++dd) {
    if (dd < 0 || dd >= 2 * n) continue;
    int i0, i1; float w0, w1;
    bil_taps(dd, n, i0, i1, w0, w1);
    float ww = 0.f;
    if (i0 == k) ww += w0;
    if (i1 == k) ww += w1;
    if (ww != 0.f) { d[cnt] = dd; wt[cnt] = ww; ++cnt; }
  }
  return cnt;
}
template <typename T>
__global__ void up2_bilinear_bwd_kernel(const void* __restrict__ dy, int yC, int y0, void* dx, int xC, int x0, int n, int h, int w, int c) {
  const size_t total = (size_t)n * h * w * c;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % c);
    size_t p = i / c;
    const int x = (int)(p % w); p /= w;
    const int y = (int)(p % h);
    const size_t img = p / h;
    int dys[6], dxs[6]; float wys[6], wxs[6];
    const int ny = bil_bwd_taps(y, h, dys, wys), nx = bil_bwd_taps(x, w, dxs, wxs);
    float s = 0.f;
    for (int a = 0; a < ny; ++a)
      for (int b = 0; b < nx; ++b)
        s += wys[a] * wxs[b] * ld<T>(dy, ((img * 2 * h + dys[a]) * 2 * w + dxs[b]) * yC + y0 + ch);
    st<T>(dx, (i / c) * xC + x0 + ch, s);
  }
}

// ---- 2x2 max pool (+ the preceding ReLU is already in the conv epilogue) for VGG-19 features ----
template <typename T>
__global__ void maxpool2_kernel(const void* __restrict__ x, int xC, int x0, void* y, int yC, int y0, int n, int h, int w, int c) {
  const int ho = h / 2, wo = w / 2;
  const size_t total = (size_t)n * ho * wo * c;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % c);
    size_t p = i / c;
    const int ox = (int)(p % wo); p /= wo;
    const int oy = (int)(p % ho);
    const size_t img = p / ho;
    const size_t b = (img * h + 2 * oy) * w + 2 * ox;
    const float v = fmaxf(fmaxf(ld<T>(x, b * xC + x0 + ch), ld<T>(x, (b + 1) * xC + x0 + ch)),
                          fmaxf(ld<T>(x, (b + w) * xC + x0 + ch), ld<T>(x, (b + w + 1) * xC + x0 + ch)));
    st<T>(y, (i / c) * yC + y0 + ch, v);
  }
}

// ---- ReLU copy (VGG taps observed pre-ReLU) ----
// The content loss runs it in place, x and y the same view (engine_v.py): neither pointer is __restrict__.  Every element is read and
// then written by one thread and by no other, so the copy in place gives what the copy out of place gives.
// x < 0 ? 0 : x is torch's relu on every input: a NaN stays a NaN (fmaxf would make it 0) and -0 stays -0.
__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }
template <typename T>
__global__ void relu_copy_kernel(const void* x, int xC, int x0, void* y, int yC, int y0, int n, int h, int w, int c) {
  const size_t total = (size_t)n * h * w * c;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % c);
    const size_t p = i / c;
    st<T>(y, p * yC + y0 + ch, relu_keep_nan(ld<T>(x, p * xC + x0 + ch)));
  }
}
template <typename T>
__global__ __launch_bounds__(256) void relu_copy_vec_kernel(const void* x, int xC, int x0, void* y, int yC, int y0, int n, int h, int w, int c) {
  constexpr int N = VecN<T>::N;
  const int cv = c / N;
  const size_t total = (size_t)n * h * w * cv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % cv) * N;
    const size_t p = i / cv;
    float v[N];
    ldv<T>(x, p * xC + x0 + ch, v);
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = relu_keep_nan(v[q]);
    stv<T>(y, p * (size_t)yC + y0 + ch, v);
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
__global__ __launch_bounds__(256) void resize_fwd_kernel(const void* __restrict__ a, int aC, int a0, void* b, int bC, int b0, int n, int hi, int wi,
                                                         int ho, int wo, int c) {
  constexpr int N = VecN<T>::N;
  const int cv = c / N;
  const float sy = (float)hi / (float)ho, sx = (float)wi / (float)wo;
  const size_t total = (size_t)n * ho * wo * cv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % cv) * N;
    size_t p = i / cv;
    const int ox = (int)(p % wo); p /= wo;
    const int oy = (int)(p % ho);
    const size_t img = p / ho;
    int ya, yb, xa, xb; float wya, wyb, wxa, wxb;
    resize_taps(oy, hi, sy, ya, yb, wya, wyb);
    resize_taps(ox, wi, sx, xa, xb, wxa, wxb);
    float acc[N], t[N];
    ldv<T>(a, ((img * hi + ya) * wi + xa) * (size_t)aC + a0 + ch, t);
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] = wya * wxa * t[q];
    ldv<T>(a, ((img * hi + ya) * wi + xb) * (size_t)aC + a0 + ch, t);
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] += wya * wxb * t[q];
    ldv<T>(a, ((img * hi + yb) * wi + xa) * (size_t)aC + a0 + ch, t);
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] += wyb * wxa * t[q];
    ldv<T>(a, ((img * hi + yb) * wi + xb) * (size_t)aC + a0 + ch, t);
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] += wyb * wxb * t[q];
    stv<T>(b, ((img * ho + oy) * wo + ox) * (size_t)bC + b0 + ch, acc);
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
__global__ __launch_bounds__(256) void resize_bwd_kernel(const void* __restrict__ dy, int yC, int y0, void* dx, int xC, int x0, int n, int hi, int wi,
                                                         int ho, int wo, int c) {
  constexpr int N = VecN<T>::N;
  const int cv = c / N;
  const float sy = (float)hi / (float)ho, sx = (float)wi / (float)wo;
  const size_t total = (size_t)n * hi * wi * cv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % cv) * N;
    size_t p = i / cv;
    const int x = (int)(p % wi); p /= wi;
    const int y = (int)(p % hi);
    const size_t img = p / hi;
    int ylo, xlo;
    const int yhi = resize_bwd_range(y, hi, ho, sy, ylo), xhi = resize_bwd_range(x, wi, wo, sx, xlo);
    float acc[N], t[N];
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
      int ya, yb; float wya, wyb;
      resize_taps(oy, hi, sy, ya, yb, wya, wyb);
      const float wy = (ya == y ? wya : 0.f) + (yb == y ? wyb : 0.f);
      if (wy == 0.f) continue;
      for (int ox = xlo; ox <= xhi; ++ox) {
        int xa, xb; float wxa, wxb;
        resize_taps(ox, wi, sx, xa, xb, wxa, wxb);
        const float wx = (xa == x ? wxa : 0.f) + (xb == x ? wxb : 0.f);
        if (wx == 0.f) continue;
        ldv<T>(dy, ((img * ho + oy) * wo + ox) * (size_t)yC + y0 + ch, t);
        const float ww = wy * wx;
#pragma unroll
        for (int q = 0; q < N; ++q) acc[q] += ww * t[q];
      }
    }
    stv<T>(dx, ((img * hi + y) * wi + x) * (size_t)xC + x0 + ch, acc);
  }
}

// ---- max-pool backward with the preceding ReLU's derivative folded in (differentiable VGG tap, ESRGAN/model.py:281-292) ----
// x: pre-pool activation (a ReLU output), dy: gradient of the pooled map, dx: gradient w.r.t. the ReLU's INPUT.
// The gradient goes to the first maximum of each 2x2 window in row-major order (ATen max_pool2d) and is zero where
// that maximum is not positive (ReLU').
template <typename T>
__global__ __launch_bounds__(256) void maxpool2_relu_bwd_kernel(const void* __restrict__ x, int xC, int x0, const void* __restrict__ dy, int yC, int y0,
                                                                void* dx, int dC, int d0, int n, int h, int w, int c) {
  const int ho = h / 2, wo = w / 2;
  const size_t total = (size_t)n * ho * wo * c;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % c);
    size_t p = i / c;
    const int ox = (int)(p % wo); p /= wo;
    const int oy = (int)(p % ho);
    const size_t img = p / ho;
    const size_t b = (img * h + 2 * oy) * w + 2 * ox;
    const size_t q[4] = {b, b + 1, b + w, b + w + 1};
    float best = ld<T>(x, q[0] * xC + x0 + ch);
    int arg = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const float v = ld<T>(x, q[k] * xC + x0 + ch);
      if (v > best) { best = v; arg = k; }
    }
    const float g = best > 0.f ? ld<T>(dy, (i / c) * yC + y0 + ch) : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) st<T>(dx, q[k] * dC + d0 + ch, k == arg ? g : 0.f);
  }
}

// ------------------------------------------------------------------------------------------------
// op: 0 nearest-x2 backward, 1 bilinear-x2 forward, 2 bilinear-x2 backward, 3 maxpool2 ; (h, w) = low-res dims (op 3: input dims)
extern "C" int srganfd_resample(int32_t op, srganfd_view a, srganfd_view b, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!a.ptr || !b.ptr || a.c0 + c > a.cstride || b.c0 + c > b.cstride) return set_err(SRGANFD_EINVAL, "resample: bad args");
  if (a.planar || b.planar) return set_err(SRGANFD_EINVAL, "resample: NHWC views only, not planar ones");
  const size_t lo = (size_t)n * h * w * c;
#define RS(K, TOTAL) DISPATCH_T(dtype, \
    SRGANFD_LAUNCH(K<TT>, dim3(grid_for(TOTAL)), dim3(256), 0, s, a.ptr, a.cstride, a.c0, b.ptr, b.cstride, b.c0, n, h, w, c))
  const int vn = dtype == SRGANFD_F32 ? 4 : 8;
  const bool vec = c % vn == 0 && a.c0 % vn == 0 && b.c0 % vn == 0 && a.cstride % vn == 0 && b.cstride % vn == 0 &&
                   ((uintptr_t)a.ptr & 15) == 0 && ((uintptr_t)b.ptr & 15) == 0;
#define RSV(OP, TOTAL) DISPATCH_T(dtype, \
    SRGANFD_LAUNCH((resample_vec_kernel<TT, OP>), dim3(grid_for((TOTAL) / vn, 256, 65536)), dim3(256), 0, s, a.ptr, a.cstride, a.c0, b.ptr, b.cstride, b.c0, n, h, w, c))
  // row-grid forms of the two bilinear ops: grid (column blocks, low-res rows, images)
  const int cv = c / vn, cv_shift = (cv & (cv - 1)) == 0 ? __builtin_ctz(cv) : -1;
  const bool rows_ok = h <= 65535 && n <= 65535 && (size_t)w * cv < (1u << 31);
  const dim3 rows_grid((unsigned)(((size_t)w * cv + 255) / 256), (unsigned)((h + kBilRows - 1) / kBilRows), (unsigned)n);
  if (vec) {
    if (op == 0) { RSV(0, lo); }
    else if (rows_ok && op == 1) {
      DISPATCH_T(dtype, SRGANFD_LAUNCH(bilinear_up2_block_kernel<TT>, rows_grid, dim3(256), 0, s, a.ptr, a.cstride, a.c0, b.ptr, b.cstride, b.c0, h, w, c, cv_shift));
    } else if (rows_ok && op == 2) {
      DISPATCH_T(dtype, SRGANFD_LAUNCH(bilinear_up2_bwd_rows_kernel<TT>, rows_grid, dim3(256), 0, s, a.ptr, a.cstride, a.c0, b.ptr, b.cstride, b.c0, h, w, c, cv_shift,
                                       (const void*)nullptr, 0, 0, (void*)nullptr, 0, 0, 0.f));
    }
    else if (op == 1) { RSV(1, lo * 4); }
    else if (op == 2) { RSV(2, lo); }
    else if (op == 3) { RSV(3, lo / 4); }
    else if (op == 4) {
      DISPATCH_T(dtype, SRGANFD_LAUNCH(relu_copy_vec_kernel<TT>, dim3(grid_for(lo / vn, 256, 65536)), dim3(256), 0, s, a.ptr, a.cstride, a.c0, b.ptr, b.cstride, b.c0, n, h, w, c));
    }
    else return set_err(SRGANFD_EINVAL, "resample: bad op %d", op);
  }
  else if (op == 0) { RS(up2_nearest_bwd_kernel, lo); }
  else if (op == 1) { RS(up2_bilinear_fwd_kernel, lo * 4); }
  else if (op == 2) { RS(up2_bilinear_bwd_kernel, lo); }
  else if (op == 3) { RS(maxpool2_kernel, lo / 4); }
  else if (op == 4) { RS(relu_copy_kernel, lo); }
  else return set_err(SRGANFD_EINVAL, "resample: bad op %d", op);
#undef RS
#undef RSV
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
// bilinear-x2 backward fused with the LeakyReLU' of the upsampled layer: dx_raw (optional) = adjoint of the upsampling applied to dy,
// dx_masked = dx_raw * (act > 0 ? 1 : slope).  16-byte-vectorised views only (the discriminators' channel counts).
extern "C" int srganfd_resample_bwd_lrelu(srganfd_view dy, srganfd_view dx_raw, srganfd_view act, srganfd_view dx_masked, int32_t dtype, int32_t n, int32_t h,
                                          int32_t w, int32_t c, float slope, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!dy.ptr || !act.ptr || !dx_masked.ptr) return set_err(SRGANFD_EINVAL, "resample_bwd_lrelu: null view");
  const int vn = dtype == SRGANFD_F32 ? 4 : 8;
  auto ok = [&](const srganfd_view& v) { return !v.ptr || (v.c0 % vn == 0 && v.cstride % vn == 0 && ((uintptr_t)v.ptr & 15) == 0 && v.c0 + c <= v.cstride && !v.planar); };
  if (c % vn || !ok(dy) || !ok(dx_raw) || !ok(act) || !ok(dx_masked))
    return set_err(SRGANFD_EINVAL, "resample_bwd_lrelu: views must be 16-byte aligned NHWC slices, not planar ones");
  const size_t lo = (size_t)n * h * w * c;
  const int cv = c / vn, cv_shift = (cv & (cv - 1)) == 0 ? __builtin_ctz(cv) : -1;
  if (h <= 65535 && n <= 65535 && (size_t)w * cv < (1u << 31)) {
    // non-temporal stores for results one pass cannot keep in the 256 MiB Infinity Cache anyway: 867 -> 805 us (128 channels, 512^2 -> 256^2, batch 32),
    // 427 -> 414 (256 channels), bit-equal; 8 / 16 rows per thread instead of 4 measured 3-10 % slower (tools/r4/bil_bwd_bench.py)
    const bool nt = lo * (size_t)(dtype == SRGANFD_F32 ? 4 : 2) >= ((size_t)192 << 20);
#define BB(NTT) DISPATCH_T(dtype, SRGANFD_LAUNCH((bilinear_up2_bwd_rows_kernel<TT, kBilRows, NTT>), dim3((unsigned)(((size_t)w * cv + 255) / 256), (unsigned)((h + kBilRows - 1) / kBilRows), (unsigned)n), dim3(256), 0, s, dy.ptr, \
                                     dy.cstride, dy.c0, dx_raw.ptr, dx_raw.cstride, dx_raw.c0, h, w, c, cv_shift, (const void*)act.ptr, act.cstride, act.c0, \
                                     dx_masked.ptr, dx_masked.cstride, dx_masked.c0, slope))
    if (nt) { BB(true); } else { BB(false); }
#undef BB
  } else
  DISPATCH_T(dtype, SRGANFD_LAUNCH((resample_vec_kernel<TT, 2>), dim3(grid_for(lo / vn, 256, 65536)), dim3(256), 0, s, dy.ptr, dy.cstride, dy.c0, dx_raw.ptr, dx_raw.cstride,
                                   dx_raw.c0, n, h, w, c, (const void*)act.ptr, act.cstride, act.c0, dx_masked.ptr, dx_masked.cstride, dx_masked.c0, slope));
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_resize_bilinear(int32_t bwd, srganfd_view a, srganfd_view b, int32_t dtype, int32_t n, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                                       int32_t c, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!a.ptr || !b.ptr || !vec_ok(dtype, c, {a, b})) return set_err(SRGANFD_EINVAL, "resize_bilinear: views must be 16-byte aligned channel multiples");
  if (a.planar || b.planar) return set_err(SRGANFD_EINVAL, "resize_bilinear: NHWC views only, not planar ones");
  const int vn = dtype == SRGANFD_F32 ? 4 : 8;
  if (!bwd) {
    const size_t total = (size_t)n * ho * wo * c / vn;
    DISPATCH_T(dtype,
               SRGANFD_LAUNCH(resize_fwd_kernel<TT>, dim3(grid_for(total, 256, 65536)), dim3(256), 0, s, a.ptr, a.cstride, a.c0, b.ptr, b.cstride, b.c0, n, hi, wi, ho, wo, c));
  } else {
    const size_t total = (size_t)n * hi * wi * c / vn;
    DISPATCH_T(dtype,
               SRGANFD_LAUNCH(resize_bwd_kernel<TT>, dim3(grid_for(total, 256, 65536)), dim3(256), 0, s, a.ptr, a.cstride, a.c0, b.ptr, b.cstride, b.c0, n, hi, wi, ho, wo, c));
  }
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_maxpool2_relu_bwd(srganfd_view x, srganfd_view dy, srganfd_view dx, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c,
                                         void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!x.ptr || !dy.ptr || !dx.ptr || n <= 0 || h <= 0 || w <= 0 || (h & 1) || (w & 1) || c <= 0) return set_err(SRGANFD_EINVAL, "maxpool2_relu_bwd: bad args");
  if (x.planar || dy.planar || dx.planar) return set_err(SRGANFD_EINVAL, "maxpool2_relu_bwd: NHWC views only, not planar ones");
  const size_t total = (size_t)n * (h / 2) * (w / 2) * c;
  DISPATCH_T(dtype,
             SRGANFD_LAUNCH(maxpool2_relu_bwd_kernel<TT>, dim3(grid_for(total)), dim3(256), 0, s, x.ptr, x.cstride, x.c0, dy.ptr, dy.cstride, dy.c0, dx.ptr, dx.cstride, dx.c0, n, h, w, c));
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

}  // namespace srganfd
