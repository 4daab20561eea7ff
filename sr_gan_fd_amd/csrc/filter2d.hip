// filter2d.hip -- the tiled 2-D filters of the degradation pipelines: one plane at a time, mirror padding without repeating the edge sample
// (torch 'reflect', scipy 'mirror'), cross-correlation (no flip).
//   filter2d_kernel<SEP>          Real-ESRGAN's filter2d_torch (Real_ESRGAN/imgproc.py:1092-1124) in fp32, every channel of image n with kernel n
//                                 (or the one shared kernel), k <= 51; the USM sharpener's two passes (imgproc.py:1517-1540) are its epilogues.
//   filter2d_mirror_f64_kernel    the blur of BSRGAN's blind degradation (BSRGAN/imgproc.py:212-225): every image with its own k x k kernel
//                                 (k = 7 .. 25) the way scipy's ndimage.convolve runs it on a float32 image with a float64 kernel: float64 products
//                                 and sums, ONE rounding to float32 at the end.  That is what makes the result land on scipy's float32 values (an
//                                 fp32 accumulation is off by up to 1e-6, enough to move a pixel to the next 8-bit level under the JPEG stage that
//                                 follows).
// Both are the same tiling: a 256-thread workgroup owns a 32-row x 64-column output tile of one plane, staged with its halo in LDS as fp32;
// thread (tx, ty) -> column tx, rows 8 ty .. 8 ty + 7, an 8-deep register window sliding down its LDS column so that one LDS read (and, in
// fp64, one conversion) feeds 8 fused multiply-adds; the taps are wave-uniform (scalar loads).  The pieces below are that tiling, written
// once for both accumulator types; MAXK, the largest kernel, sizes the LDS arrays (51 in fp32, 25 in fp64).
#include <math.h>
#include "elementwise.hpp"

namespace srganfd {

static constexpr int kF2dRows = 32, kF2dCols = 64, kF2dMaxK = 51, kF64MaxK = 25;
template <int MAXK> struct F2dLds {
  static constexpr int kPitch = kF2dCols + MAXK - 1;             // floats per staged row
  static constexpr int kHaloRows = kF2dRows + MAXK - 1;
};

__device__ __forceinline__ int reflect_idx(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return min(max(i, 0), n - 1);   // only positions no output reads get clamped
}

// the tile of a workgroup of the grid (tiles_x * tiles_y, b * c), and what a thread of it owns
struct F2dTile {
  int plane, img, ty_base, tx_base, tx, ty0;
  __device__ __forceinline__ F2dTile(int c, int tiles_x)
      : plane(blockIdx.y), img(plane / c), ty_base((blockIdx.x / tiles_x) * kF2dRows), tx_base((blockIdx.x % tiles_x) * kF2dCols),
        tx(threadIdx.x & 63), ty0((threadIdx.x >> 6) * 8) {}
  // the tile's (32 + k - 1) x (64 + k - 1) inputs, mirrored at the plane's edges, into LDS rows of `pitch` floats
  __device__ __forceinline__ void stage(const float* __restrict__ sp, int h, int w, int k, float* tile, int pitch) const {
    const int r = k / 2, in_rows = kF2dRows + k - 1, in_cols = kF2dCols + k - 1;
    for (int i = threadIdx.x; i < in_rows * in_cols; i += 256) {
      const int iy = i / in_cols, ix = i % in_cols;
      tile[iy * pitch + ix] = sp[(size_t)reflect_idx(ty_base + iy - r, h) * w + reflect_idx(tx_base + ix - r, w)];
    }
  }
  // f(o, y * w + x) for this thread's outputs o = 0 .. 7 that lie inside the plane
  template <typename F> __device__ __forceinline__ void store(int h, int w, F f) const {
    const int x = tx_base + tx;
    if (x >= w) return;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      const int y = ty_base + ty0 + o;
      if (y >= h) break;
      f(o, (size_t)y * w + x);
    }
  }
};

__device__ __forceinline__ float f2d_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double f2d_fma(double a, double b, double c) { return fma(a, b, c); }

// acc[o] += sum over ky < k of taps[ky * tap_stride] * col[(o + ky) * pitch]: the window slides down the LDS column `col`
template <typename ACC>
__device__ __forceinline__ void f2d_slide(const float* col, int pitch, const ACC* __restrict__ taps, int tap_stride, int k, ACC (&acc)[8]) {
  ACC win[8];
#pragma unroll
  for (int o = 0; o < 7; ++o) win[o] = (ACC)col[o * pitch];
  for (int ky0 = 0; ky0 < k; ky0 += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ky = ky0 + j;
      if (ky < k) {                                          // wave-uniform
        win[(j + 7) & 7] = (ACC)col[(ky + 7) * pitch];
        const ACC wv = taps[ky * tap_stride];
#pragma unroll
        for (int o = 0; o < 8; ++o) acc[o] = f2d_fma(wv, win[(j + o) & 7], acc[o]);
      }
    }
  }
}

// SEP: the k x k filter is the outer product kcol (vertical taps) x krow (horizontal taps), handed over as kernels[0..k) and
// kernels[k..2k): a horizontal pass into a second LDS image, then the same sliding-window pass vertically -- 2k instead of
// k*k multiply-adds per pixel (the 51x51 Gaussian of the USM sharpener: 25x fewer).  The USM epilogues:
//   mode 1: residual = x - blur -> out;  mask = (|residual| * 255 > threshold) -> out2
//   mode 2: soft = blur(mask);  out = soft * clip(x + weight * residual, 0, 1) + (1 - soft) * x
template <bool SEP>
__global__ __launch_bounds__(256) void filter2d_kernel(const float* __restrict__ src, const float* __restrict__ kernels, int kernel_batch, int c, int h,
                                                       int w, int k, int tiles_x, int mode, const float* __restrict__ x_in,
                                                       const float* __restrict__ res_in, float weight, float threshold, float* __restrict__ out,
                                                       float* __restrict__ out2) {
  using L = F2dLds<kF2dMaxK>;
  constexpr int kTileRows = L::kHaloRows + (SEP ? 0 : 8);        // the unrolled window may address (never use) 8 rows past the halo
  constexpr int kHRows = SEP ? L::kHaloRows + 8 : 1;
  __shared__ float tile[kTileRows * L::kPitch];
  __shared__ float hbuf[kHRows * kF2dCols];
  const F2dTile t(c, tiles_x);
  const size_t base = (size_t)t.plane * h * w;
  const float* sp = src + base;
  const float* kw = kernels + (kernel_batch > 1 ? (size_t)t.img * (SEP ? 2 * k : k * k) : 0);
  t.stage(sp, h, w, k, tile, L::kPitch);
  __syncthreads();
  float acc[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) acc[o] = 0.f;
  if (SEP) {
    const float* krow = kw + k;
    for (int row = threadIdx.x >> 6; row < kF2dRows + k - 1; row += 4) {
      const float* tr = tile + row * L::kPitch + t.tx;
      float a = 0.f;
      for (int kx = 0; kx < k; ++kx) a = fmaf(krow[kx], tr[kx], a);
      hbuf[row * kF2dCols + t.tx] = a;
    }
    __syncthreads();
    f2d_slide(hbuf + t.ty0 * kF2dCols + t.tx, kF2dCols, kw, 1, k, acc);
  } else {
    for (int kx = 0; kx < k; ++kx) f2d_slide(tile + t.ty0 * L::kPitch + t.tx + kx, L::kPitch, kw + kx, k, k, acc);
  }
  t.store(h, w, [&](int o, size_t pix) {
    const size_t idx = base + pix;
    if (mode == 0) {
      out[idx] = acc[o];
    } else if (mode == 1) {
      const float res = sp[pix] - acc[o];
      out[idx] = res;
      out2[idx] = (fabsf(res) * 255.f > threshold) ? 1.f : 0.f;
    } else {
      const float xv = x_in[idx], soft = acc[o];
      const float sharp = fminf(fmaxf(xv + weight * res_in[idx], 0.f), 1.f);
      out[idx] = soft * sharp + (1.f - soft) * xv;
    }
  });
}

// Each image's own k x k taps sit centred in a kmax x kmax float64 array; ksize[img] = 0 copies the plane through.
__global__ __launch_bounds__(256) void filter2d_mirror_f64_kernel(const float* __restrict__ src, const double* __restrict__ kernels, int kmax,
                                                                  const int* __restrict__ ksize, int c, int h, int w, int tiles_x,
                                                                  float* __restrict__ out) {
  using L = F2dLds<kF64MaxK>;
  __shared__ float tile[(L::kHaloRows + 8) * L::kPitch];         // the unrolled window may address (never use) 8 rows past the halo
  const F2dTile t(c, tiles_x);
  const float* sp = src + (size_t)t.plane * h * w;
  float* op = out + (size_t)t.plane * h * w;
  int k = ksize[t.img];
  if (k < 3 || k > kmax || !(k & 1)) k = 0;                        // the host refuses such sizes where it can see them; here they copy through
  if (k == 0) {
    for (int i = threadIdx.x; i < kF2dRows * kF2dCols; i += 256) {
      const int y = t.ty_base + i / kF2dCols, x = t.tx_base + i % kF2dCols;
      if (y < h && x < w) op[(size_t)y * w + x] = sp[(size_t)y * w + x];
    }
    return;
  }
  t.stage(sp, h, w, k, tile, L::kPitch);
  const int in_rows = kF2dRows + k - 1;
  for (int i = in_rows * L::kPitch + threadIdx.x; i < (in_rows + 8) * L::kPitch; i += 256) tile[i] = 0.f;   // addressed by the window, never used
  __syncthreads();
  const int off = (kmax - k) / 2;
  const double* kw = kernels + (size_t)t.img * kmax * kmax + (size_t)off * kmax + off;
  double acc[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) acc[o] = 0.0;
  for (int kx = 0; kx < k; ++kx) f2d_slide(tile + t.ty0 * L::kPitch + t.tx + kx, L::kPitch, kw + kx, kmax, k, acc);
  t.store(h, w, [&](int o, size_t pix) { op[pix] = (float)acc[o]; });
}

// The refusals the fp32 and the fp64 check lists share, each worded as its entry point always worded it; every list keeps its own order.
struct F2dRefusals {
  const char *name, *pad, *by;
  int padding(int r, int h, int w) const {
    if (r < h && r < w) return SRGANFD_OK;
    return set_err(SRGANFD_EINVAL, "%s: %s padding %d needs an image larger than that (%d%s%d)", name, pad, r, h, by, w);
  }
  int planes(int b, int c) const { return (long long)b * c > 65535 ? set_err(SRGANFD_EINVAL, "%s: more than 65535 planes", name) : SRGANFD_OK; }
};
static dim3 f2d_grid(int b, int c, int h, int w) { return dim3(ceil_div(w, kF2dCols) * ceil_div(h, kF2dRows), b * c); }
static constexpr F2dRefusals kF32{"filter2d", "reflect", "x"}, kF64{"filter2d_mirror_f64", "mirror", " x "};

// shared by srganfd_filter2d, srganfd_filter2d_separable and the two passes of srganfd_usm_sharp
static int filter2d_impl(const float* src, const float* kernels, int kernel_batch, int b, int c, int h, int w, int k, int mode, const float* x_in,
                         const float* res_in, float weight, float threshold, float* out, float* out2, hipStream_t s, bool separable) {
  if (!src || !kernels || !out || b <= 0 || c <= 0 || h <= 0 || w <= 0) return refuse_empty("filter2d");
  if (k % 2 == 0 || k < 1) return set_err(SRGANFD_EINVAL, "Wrong kernel size.");                     // the reference's ValueError text
  if (k > kF2dMaxK) return set_err(SRGANFD_EINVAL, "filter2d: kernel size %d above the LDS tile's %d", k, kF2dMaxK);
  if (int rc = kF32.padding(k / 2, h, w)) return rc;
  if (kernel_batch != 1 && kernel_batch != b) return set_err(SRGANFD_EINVAL, "filter2d: %d kernels for %d images", kernel_batch, b);
  if ((mode == 1 && !out2) || (mode == 2 && (!x_in || !res_in)) || mode < 0 || mode > 2) return set_err(SRGANFD_EINVAL, "filter2d: bad epilogue arguments");
  if (int rc = kF32.planes(b, c)) return rc;
  const int tiles_x = ceil_div(w, kF2dCols);
  if (separable)
    SRGANFD_LAUNCH(filter2d_kernel<true>, f2d_grid(b, c, h, w), dim3(256), 0, s, src, kernels, kernel_batch, c, h, w, k, tiles_x, mode, x_in, res_in, weight,
                   threshold, out, out2);
  else
    SRGANFD_LAUNCH(filter2d_kernel<false>, f2d_grid(b, c, h, w), dim3(256), 0, s, src, kernels, kernel_batch, c, h, w, k, tiles_x, mode, x_in, res_in, weight,
                   threshold, out, out2);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_filter2d(const float* image, const float* kernels, int32_t kernel_batch, int32_t b, int32_t c, int32_t h, int32_t w, int32_t k, float* out,
                                void* stream) {
  return filter2d_impl(image, kernels, kernel_batch, b, c, h, w, k, 0, nullptr, nullptr, 0.f, 0.f, out, nullptr, (hipStream_t)stream, false);
}
extern "C" int srganfd_usm_sharp(const float* image, const float* kernel, int32_t separable, int32_t b, int32_t c, int32_t h, int32_t w, int32_t k, float weight,
                                 float threshold, float* out, float* workspace, void* stream) {
  if (!workspace) return set_err(SRGANFD_EINVAL, "usm_sharp: workspace of 2 * b*c*h*w floats needed");
  const size_t n = (size_t)b * c * h * w;
  float* residual = workspace;
  float* mask = workspace + n;
  int rc = filter2d_impl(image, kernel, 1, b, c, h, w, k, 1, nullptr, nullptr, weight, threshold, residual, mask, (hipStream_t)stream, separable != 0);
  if (rc != SRGANFD_OK) return rc;
  return filter2d_impl(mask, kernel, 1, b, c, h, w, k, 2, image, residual, weight, threshold, out, nullptr, (hipStream_t)stream, separable != 0);
}
extern "C" int srganfd_filter2d_separable(const float* image, const float* taps, int32_t kernel_batch, int32_t b, int32_t c, int32_t h, int32_t w, int32_t k,
                                          float* out, void* stream) {
  return filter2d_impl(image, taps, kernel_batch, b, c, h, w, k, 0, nullptr, nullptr, 0.f, 0.f, out, nullptr, (hipStream_t)stream, true);
}

extern "C" int srganfd_filter2d_mirror_f64(const float* src, const double* kernels, int32_t kmax, const int32_t* ksize, const int32_t* ksize_host, int32_t b,
                                           int32_t c, int32_t h, int32_t w, float* out, void* stream) {
  if (!src || !kernels || !ksize || !out) return set_err(SRGANFD_EINVAL, "filter2d_mirror_f64: null pointer");
  if (b <= 0 || c <= 0 || h <= 0 || w <= 0) return set_err(SRGANFD_EINVAL, "filter2d_mirror_f64: bad args (b %d, c %d, %d x %d: all must be positive)", b, c, h, w);
  if (kmax < 3 || kmax > kF64MaxK || kmax % 2 == 0) return set_err(SRGANFD_EINVAL, "filter2d_mirror_f64: kmax %d is not an odd size from 3 to %d", kmax, kF64MaxK);
  if (src == out) return set_err(SRGANFD_EINVAL, "filter2d_mirror_f64: the output may not alias the input");
  int need = kmax;                       // without a host copy of the sizes every image must fit the largest one
  if (ksize_host) {
    need = 0;
    for (int i = 0; i < b; ++i) {
      const int k = ksize_host[i];
      if (k != 0 && (k < 3 || k > kmax || k % 2 == 0))
        return set_err(SRGANFD_EINVAL, "filter2d_mirror_f64: ksize[%d] = %d is neither 0 nor an odd size from 3 to kmax = %d", i, k, kmax);
      if (k > need) need = k;
    }
  }
  if (int rc = kF64.padding(need / 2, h, w)) return rc;
  if (int rc = kF64.planes(b, c)) return rc;
  SRGANFD_LAUNCH(filter2d_mirror_f64_kernel, f2d_grid(b, c, h, w), dim3(256), 0, (hipStream_t)stream, src, kernels, kmax, ksize, c, h, w, ceil_div(w, kF2dCols), out);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

}  // namespace srganfd
