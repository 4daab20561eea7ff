// iqa.hip -- NIQE's feature extraction (BSRGAN/image_quality_assessment.py:1138-1333 of the reference) as three kernels:
//   niqe_luma_kernel    crop, BT.601 luma in fp32, x255, round half to even, crop to whole blocks -> fp64 plane of integers
//   resize_half_kernel  the reference's 0.5x antialiased cubic resize (10 taps, symmetric padding, rows then columns), one 16x16
//                       output tile per workgroup, both passes through LDS
//   niqe_block_kernel   one workgroup per block and scale: the block plus a 3-pixel halo staged in LDS, the MSCN map formed in LDS
//                       (it never goes to HBM: the circular shifts wrap inside the block), 5 maps x 6 sums reduced over the workgroup
//                       in a fixed order, the AGGD fits and the 18 features by the first lanes of wave 0
// Launch plan per batch: luma, block kernel (scale 1), resize, block kernel (scale 2).  fp64 vector arithmetic throughout (no MFMA),
// except the resize, which the reference runs in float32 (see resize_half_kernel).
// PSNR and SSIM are in psnr_ssim.hip: this file compiles with floating-point contraction off (below), they were validated with it on.
#include "common.hpp"
#include <math.h>

// parity with the reference's separate multiply and subtract (sigma = sqrt(|E[x^2] - mu^2| + 1e-8) cancels on flat regions) and with its
// float32 resize, where every product is rounded before it is added: no implicit fused multiply-add in this file; fma() is explicit
#pragma clang fp contract(off)

namespace srganfd {

static constexpr int kNiqeThreads = 512;              // 8 waves; one workgroup per CU (its LDS plan is > 80 KB at the default block)
static constexpr int kNiqeWaves = kNiqeThreads / 64;
static constexpr int kNiqeHalo = 3;                   // 7 x 7 window
static constexpr int kNiqeMaps = 5, kNiqeSums = 6;    // s and its four shifted products; {#neg, #pos, sum x^2 | x<0, sum x^2 | x>0, sum |x|, sum x^2}
static constexpr size_t kNiqeLdsMax = 160 * 1024;
static constexpr int kNiqeRed = (kNiqeThreads / 64 + 1) * 5 * 6;   // reduction scratch in doubles: one row of 30 per wave, one for the totals
// doubles of the first LDS region: the block and its halo, later the reduction scratch
__host__ __device__ static inline size_t niqe_stage_doubles(int bh, int bw) {
  const size_t t = (size_t)(bh + 6) * (bw + 6);
  return t > (size_t)kNiqeRed ? t : (size_t)kNiqeRed;
}

struct NiqeWindow { double g[49]; };

// The 7 x 7 Gaussian, sigma 7/6, normalised in fp64, rounded to float32 and widened again (the reference builds it in numpy fp64 and
// stores it with .float()).
static NiqeWindow niqe_window() {
  NiqeWindow w;
  const double sigma = 7.0 / 6.0;
  double sum = 0.0;
  for (int i = 0; i < 7; ++i)
    for (int j = 0; j < 7; ++j) {
      const double y = i - 3.0, x = j - 3.0;
      w.g[i * 7 + j] = exp(-(x * x + y * y) / (2.0 * sigma * sigma));
      sum += w.g[i * 7 + j];
    }
  for (int i = 0; i < 49; ++i) w.g[i] = (double)(float)(w.g[i] / sum);
  return w;
}

// grid-stride over the n * lh * lw luma pixels
__global__ __launch_bounds__(256) void niqe_luma_kernel(const float* __restrict__ rgb, int h, int w, int cb, int lh, int lw, size_t total,
                                                        double* __restrict__ luma) {
  const size_t plane = (size_t)h * w;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int x = (int)(i % lw);
    const size_t t = i / lw;
    const int y = (int)(t % lh);
    const size_t img = t / lh;
    const float* p = rgb + img * 3 * plane + (size_t)(y + cb) * w + (x + cb);
    // the same fp32 chain as psnr_partial_kernel (torch.matmul with the (3, 1) weight, + 16, / 255), then the reference's *= 255 and round()
    float v = p[0] * 65.481f;
    v = fmaf(p[plane], 128.553f, v);
    v = fmaf(p[2 * plane], 24.966f, v);
    v = (v + 16.0f) / 255.f;
    luma[i] = (double)rintf(v * 255.0f);
  }
}

// 0.5x cubic (a = -0.5) with antialiasing: the kernel stretched by 2 covers 8 inputs, the reference keeps a margin of one on each side
// (10 taps, the outer two weigh 0); output i reads inputs 2i-4 .. 2i+5; the weights cubic((4.5 - k) / 2), k = 0..9, sum to exactly 2
// and are dyadic, so the normalised weights below are exact in float32.
__constant__ float kHalfTaps[10] = {0.0f, -0.01171875f, -0.03515625f, 0.11328125f, 0.43359375f,
                                    0.43359375f, 0.11328125f, -0.03515625f, -0.01171875f, 0.0f};
static constexpr int kHalfTile = 16, kHalfIn = 2 * kHalfTile + 8;   // inputs 2*t0 - 4 .. 2*(t0 + 15) + 5
// MATLAB symmetric padding: the edge sample is used twice (-1 -> 0, n -> n - 1); one reflection is enough for n >= 4 (even) / 5 (odd)
__device__ __forceinline__ int half_reflect(int j, int n) { return j < 0 ? -1 - j : (j >= n ? 2 * n - 1 - j : j); }

// The reference's resize casts its input to float32 whatever it is given (its dtype test is always true), runs both passes in float32
// and casts back, so the half-size image holds float32 values and every NIQE score depends on those roundings.  They are reproduced:
// src / div rounded to float32, each product rounded, the ten products added in tap order, rows first, then columns.
// grid (tiles_x, tiles_y, planes)
__global__ __launch_bounds__(256) void resize_half_kernel(const double* __restrict__ src, int h, int w, int oh, int ow, double div,
                                                          double* __restrict__ dst) {
  __shared__ float sin_[kHalfIn * kHalfIn], srow[kHalfTile * kHalfIn];
  const double* p = src + (size_t)blockIdx.z * h * w;
  const int oy0 = blockIdx.y * kHalfTile, ox0 = blockIdx.x * kHalfTile;
  for (int i = threadIdx.x; i < kHalfIn * kHalfIn; i += 256) {
    // rows and columns past what the image's own outputs read (a tile overhanging the edge) are clamped: they feed no stored output
    const int iy = min(max(half_reflect(2 * oy0 - 4 + i / kHalfIn, h), 0), h - 1);
    const int ix = min(max(half_reflect(2 * ox0 - 4 + i % kHalfIn, w), 0), w - 1);
    sin_[i] = (float)(p[(size_t)iy * w + ix] / div);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kHalfTile * kHalfIn; i += 256) {     // rows: output row r of the tile, every staged column
    const int r = i / kHalfIn, c = i % kHalfIn;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 10; ++k) acc = acc + kHalfTaps[k] * sin_[(2 * r + k) * kHalfIn + c];
    srow[i] = acc;
  }
  __syncthreads();
  const int r = threadIdx.x / kHalfTile, c = threadIdx.x % kHalfTile;
  if (oy0 + r < oh && ox0 + c < ow) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 10; ++k) acc = acc + kHalfTaps[k] * srow[r * kHalfIn + 2 * c + k];
    dst[((size_t)blockIdx.z * oh + oy0 + r) * ow + ox0 + c] = (double)acc;
  }
}

// first table index that minimises |r_gam - v|, as argmin does: the table rises strictly, so it is the lower bound of v or the entry
// before it; every |r_gam - v| is NaN or inf for a NaN or infinite v, and argmin then answers 0
__device__ int niqe_table_pick(const double* __restrict__ r_gam, int len, double v) {
  if (!(v == v) || isinf(v)) return 0;
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (r_gam[mid] < v) lo = mid + 1; else hi = mid;
  }
  if (lo == len) return len - 1;
  if (lo > 0 && fabs(r_gam[lo - 1] - v) <= fabs(r_gam[lo] - v)) return lo - 1;
  return lo;
}

struct NiqeBlockArgs {
  const double* plane;     // (n, ph, pw) fp64
  const double* table;     // (4, table_len): shape, r_gam, sqrt(exp(lgamma(1/a) - lgamma(3/a))), exp(lgamma(2/a) - lgamma(1/a))
  double* feat;            // (n, nby * nbx, 36), already offset by 18 * scale index
  double mult;             // 255 for the half-size plane (kept in [0,1]), 1 for the luma plane
  int ph, pw, bh, bw, nby, table_len;
  NiqeWindow win;
};

// grid (nby * nbx, n); dynamic LDS: (bh + 6) * (bw + 6) doubles of pixels (reused for the reduction) + bh * bw doubles of MSCN values
__global__ __launch_bounds__(kNiqeThreads) void niqe_block_kernel(const NiqeBlockArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int bh = a.bh, bw = a.bw, tw = bw + 2 * kNiqeHalo, th = bh + 2 * kNiqeHalo;
  double* xs = (double*)smem;
  double* ss = xs + niqe_stage_doubles(bh, bw);
  const int blk = blockIdx.x;                       // the reference's block order: column-major, index = bx * nby + by
  const int by = blk % a.nby, bx = blk / a.nby;
  const double* p = a.plane + (size_t)blockIdx.y * a.ph * a.pw;
  const int y0 = by * bh - kNiqeHalo, x0 = bx * bw - kNiqeHalo;
  for (int i = threadIdx.x; i < th * tw; i += kNiqeThreads) {
    const int gy = min(max(y0 + i / tw, 0), a.ph - 1), gx = min(max(x0 + i % tw, 0), a.pw - 1);     // replicate padding of the image
    xs[i] = p[(size_t)gy * a.pw + gx] * a.mult;
  }
  __syncthreads();
  const int npix = bh * bw;
  for (int i = threadIdx.x; i < npix; i += kNiqeThreads) {
    const int y = i / bw, x = i % bw;
    double mu = 0.0, m2 = 0.0;
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) {
      const double* row = xs + (y + ky) * tw + x;
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) {
        const double v = row[kx], g = a.win.g[ky * 7 + kx];
        mu = fma(g, v, mu);
        m2 = fma(g, v * v, m2);
      }
    }
    const double sigma = sqrt(fabs(m2 - mu * mu) + 1e-8);
    ss[i] = (xs[(y + kNiqeHalo) * tw + x + kNiqeHalo] - mu) / (sigma + 1.0);
  }
  __syncthreads();
  // map 0: s; maps 1..4: s * roll(s, (sy, sx)) for (0,1), (1,0), (1,1), (1,-1); rolled[y][x] = s[(y - sy) mod bh][(x - sx) mod bw]
  double acc[kNiqeMaps][kNiqeSums];
#pragma unroll
  for (int m = 0; m < kNiqeMaps; ++m)
#pragma unroll
    for (int q = 0; q < kNiqeSums; ++q) acc[m][q] = 0.0;
  for (int i = threadIdx.x; i < npix; i += kNiqeThreads) {
    const int y = i / bw, x = i % bw;
    const int yu = y == 0 ? bh - 1 : y - 1, xl = x == 0 ? bw - 1 : x - 1, xr = x == bw - 1 ? 0 : x + 1;
    const double s = ss[i];
    const double v[kNiqeMaps] = {s, s * ss[y * bw + xl], s * ss[yu * bw + x], s * ss[yu * bw + xl], s * ss[yu * bw + xr]};
#pragma unroll
    for (int m = 0; m < kNiqeMaps; ++m) {
      const double sq = v[m] * v[m];
      if (v[m] < 0.0) { acc[m][0] += 1.0; acc[m][2] += sq; }
      if (v[m] > 0.0) { acc[m][1] += 1.0; acc[m][3] += sq; }
      acc[m][4] += fabs(v[m]);
      acc[m][5] += sq;
    }
  }
  // fixed-order reduction: lanes by shuffle, then the waves' partials in wave order (identical bits on every run, whatever the batch)
  double* red = xs;                                  // the staged pixels are dead
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < kNiqeMaps; ++m)
#pragma unroll
    for (int q = 0; q < kNiqeSums; ++q) {
      double t = acc[m][q];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
      if (lane == 0) red[wave * (kNiqeMaps * kNiqeSums) + m * kNiqeSums + q] = t;
    }
  __syncthreads();
  if (threadIdx.x < kNiqeMaps * kNiqeSums) {
    double t = 0.0;
    for (int wv = 0; wv < kNiqeWaves; ++wv) t += red[wv * (kNiqeMaps * kNiqeSums) + threadIdx.x];
    red[kNiqeWaves * kNiqeMaps * kNiqeSums + threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x < kNiqeMaps) {
    const int m = threadIdx.x;
    const double* q = red + kNiqeWaves * kNiqeMaps * kNiqeSums + m * kNiqeSums;
    // the reference counts in float32 and adds 1e-8 there: the sum is the count itself, or float32(1e-8) for an empty side
    const double dl = (double)((float)q[0] + 1e-8f), dr = (double)((float)q[1] + 1e-8f);
    const double lstd = sqrt(q[2] / dl), rstd = sqrt(q[3] / dr);
    const double gh = lstd / rstd;
    const double mean_abs = q[4] / (double)npix;
    const double rhat = (mean_abs * mean_abs) / (q[5] / (double)npix);
    const double g2 = gh * gh + 1.0;
    const double rhat_norm = (rhat * (gh * gh * gh + 1.0) * (gh + 1.0)) / (g2 * g2);
    const int k = niqe_table_pick(a.table + a.table_len, a.table_len, rhat_norm);
    const double alpha = a.table[k], cb = a.table[2 * a.table_len + k], cm = a.table[3 * a.table_len + k];
    const double lb = lstd * cb, rb = rstd * cb;
    double* f = a.feat + ((size_t)blockIdx.y * gridDim.x + blk) * 36;
    if (m == 0) {
      f[0] = alpha; f[1] = (lb + rb) / 2.0;
    } else {
      f += 2 + 4 * (m - 1);
      f[0] = alpha; f[1] = (rb - lb) * cm; f[2] = lb; f[3] = rb;
    }
  }
}

static size_t niqe_block_lds(int bh, int bw) {
  return (niqe_stage_doubles(bh, bw) + (size_t)bh * bw) * sizeof(double);
}

// geometry shared by the entry points: lh x lw = the cropped image cut to whole blocks
static int niqe_geometry(const char* who, int n, int hc, int wc, int bh, int bw, int* lh, int* lw) {
  if (n <= 0 || n > 65535 || hc <= 0 || wc <= 0) return set_err(SRGANFD_EINVAL, "%s: bad args (n = %d, cropped image %d x %d)", who, n, hc, wc);
  if (bh < 2 || bw < 2 || (bh & 1) || (bw & 1))
    return set_err(SRGANFD_EINVAL, "%s: block size %d x %d must be even (scale 2 halves it) and at least 2", who, bh, bw);
  if (bh > hc || bw > wc) return set_err(SRGANFD_EINVAL, "%s: block %d x %d is larger than the cropped image %d x %d", who, bh, bw, hc, wc);
  const int nby = hc / bh, nbx = wc / bw;
  if ((long long)nby * nbx < 2)
    return set_err(SRGANFD_EINVAL, "%s: the cropped image %d x %d holds %d block of %d x %d; the covariance over blocks needs at least 2", who, hc, wc,
                   nby * nbx, bh, bw);
  if (niqe_block_lds(bh, bw) > kNiqeLdsMax)
    return set_err(SRGANFD_EINVAL, "%s: block %d x %d needs %zu bytes of LDS (block + halo + its MSCN map in fp64), the CU has %zu", who, bh, bw,
                   niqe_block_lds(bh, bw), kNiqeLdsMax);
  *lh = nby * bh;
  *lw = nbx * bw;
  if (*lh < 4 || *lw < 4) return set_err(SRGANFD_EINVAL, "%s: the half-size resize needs at least 4 x 4 pixels, have %d x %d", who, *lh, *lw);
  return SRGANFD_OK;
}

extern "C" int64_t srganfd_niqe_workspace_doubles(int32_t n, int32_t c, int32_t h, int32_t w, int32_t crop_border, int32_t bh, int32_t bw) {
  int lh = 0, lw = 0;
  if (c != 3) { set_err(SRGANFD_EINVAL, "niqe: needs 3-channel RGB input, have %d channels", c); return -1; }
  if (crop_border < 0 || niqe_geometry("niqe", n, h - 2 * crop_border, w - 2 * crop_border, bh, bw, &lh, &lw) != SRGANFD_OK) {
    if (crop_border < 0) set_err(SRGANFD_EINVAL, "niqe: negative crop_border");
    return -1;
  }
  return (int64_t)n * lh * lw + (int64_t)n * (lh / 2) * (lw / 2);
}

// shared by srganfd_resize_half (div 1) and srganfd_niqe_features_luma (div 255: the second scale works on [0, 1])
static int resize_half_impl(const double* src, int planes, int h, int w, double div, double* dst, hipStream_t s) {
  if (!src || !dst || planes <= 0 || planes > 65535 || h < 4 + (h & 1) || w < 4 + (w & 1))
    return set_err(SRGANFD_EINVAL, "resize_half: bad args (planes 1..65535 of at least 4 x 4 pixels, 5 along an odd side)");
  const int oh = (h + 1) / 2, ow = (w + 1) / 2;
  SRGANFD_LAUNCH(resize_half_kernel, dim3(ceil_div(ow, kHalfTile), ceil_div(oh, kHalfTile), planes), dim3(256), 0, s, src, h, w, oh, ow, div, dst);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_resize_half(const double* src, int32_t planes, int32_t h, int32_t w, double* dst, void* stream) {
  return resize_half_impl(src, planes, h, w, 1.0, dst, (hipStream_t)stream);
}

static int niqe_block_launch(const double* plane, int n, int ph, int pw, int bh, int bw, double mult, const double* table, int table_len,
                             double* feat, hipStream_t s) {
  const size_t lds = niqe_block_lds(bh, bw);
  static unsigned long long attr_done = 0;   // one bit per device: the attribute belongs to the device's code object
  if (!g_dry_run) {
    int dev = 0;
    SRGANFD_HIP_CHECK(hipGetDevice(&dev));
    if (!(attr_done >> (dev & 63) & 1ULL)) {
      SRGANFD_HIP_CHECK(hipFuncSetAttribute((const void*)niqe_block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kNiqeLdsMax));
      attr_done |= 1ULL << (dev & 63);
    }
  }
  static const NiqeWindow win = niqe_window();
  NiqeBlockArgs a;
  a.plane = plane; a.table = table; a.feat = feat; a.mult = mult;
  a.ph = ph; a.pw = pw; a.bh = bh; a.bw = bw; a.nby = ph / bh; a.table_len = table_len;
  a.win = win;
  SRGANFD_LAUNCH(niqe_block_kernel, dim3((ph / bh) * (pw / bw), n), dim3(kNiqeThreads), lds, s, a);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

// luma (n, h, w) with h, w whole multiples of the block -> feat (n, blocks, 36), half (n, h/2, w/2) in [0,1]
extern "C" int srganfd_niqe_features_luma(const double* luma, int32_t n, int32_t h, int32_t w, int32_t bh, int32_t bw, const double* table, int32_t table_len,
                                          double* feat, double* half, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  int lh = 0, lw = 0;
  if (!luma || !table || !feat || !half || table_len < 2) return set_err(SRGANFD_EINVAL, "niqe_features_luma: null pointer or a table of fewer than 2 entries");
  int rc = niqe_geometry("niqe_features_luma", n, h, w, bh, bw, &lh, &lw);
  if (rc != SRGANFD_OK) return rc;
  if (lh != h || lw != w) return set_err(SRGANFD_EINVAL, "niqe_features_luma: the plane %d x %d is not a whole number of %d x %d blocks", h, w, bh, bw);
  if ((rc = niqe_block_launch(luma, n, h, w, bh, bw, 1.0, table, table_len, feat, s)) != SRGANFD_OK) return rc;
  if ((rc = resize_half_impl(luma, n, h, w, 255.0, half, s)) != SRGANFD_OK) return rc;
  return niqe_block_launch(half, n, h / 2, w / 2, bh / 2, bw / 2, 255.0, table, table_len, feat + 18, s);
}

extern "C" int srganfd_niqe_features(const float* rgb, int32_t n, int32_t c, int32_t h, int32_t w, int32_t crop_border, int32_t bh, int32_t bw,
                                     const double* table, int32_t table_len, double* feat, double* ws, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!rgb || !table || !feat || !ws || table_len < 2) return set_err(SRGANFD_EINVAL, "niqe_features: null pointer or a table of fewer than 2 entries");
  if (srganfd_niqe_workspace_doubles(n, c, h, w, crop_border, bh, bw) < 0) return SRGANFD_EINVAL;
  const int lh = (h - 2 * crop_border) / bh * bh, lw = (w - 2 * crop_border) / bw * bw;
  const size_t total = (size_t)n * lh * lw;
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  SRGANFD_LAUNCH(niqe_luma_kernel, dim3(grid), dim3(256), 0, s, rgb, h, w, crop_border, lh, lw, total, ws);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return srganfd_niqe_features_luma(ws, n, lh, lw, bh, bw, table, table_len, feat, ws + total, stream);
}

}  // namespace srganfd
