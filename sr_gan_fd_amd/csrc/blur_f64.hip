// blur_f64.hip -- the blur of BSRGAN's blind degradation (BSRGAN/imgproc.py:212-225): every image of a batch filtered with its own k x k
// kernel (k = 7 .. 25), mirror padding, the way scipy's ndimage.convolve runs it on a float32 image with a float64 kernel: float64
// products and sums, ONE rounding to float32 at the end.  That is what makes the result land on scipy's float32 values (an fp32
// accumulation is off by up to 1e-6, enough to move a pixel to the next 8-bit level under the JPEG stage that follows); the fp32
// srganfd_filter2d of degrade.hip stays what Real-ESRGAN's filter2d_torch is.
// Same tiling as that kernel: a 256-thread workgroup owns a 32-row x 64-column output tile of one plane, staged with its halo in LDS as
// fp32; thread (tx, ty) -> column tx, rows 8 ty .. 8 ty + 7, an 8-deep register window sliding down its LDS column so that one LDS read
// (and one conversion to fp64) feeds 8 fused multiply-adds; the taps are read at a wave-uniform address.  The workgroup loops over its
// image's own k x k taps only, which sit centred in a kmax x kmax array.  Cross-correlation (no flip), like srganfd_filter2d.
#include "common.hpp"

namespace srganfd {

static constexpr int kB64Rows = 32, kB64Cols = 64, kB64MaxK = 25;

// reflect without repeating the edge sample (scipy 'mirror', torch 'reflect'); only positions no output reads get clamped
__device__ __forceinline__ int b64_mirror(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return min(max(i, 0), n - 1);
}

// grid (tiles_x * tiles_y, b * c)
__global__ __launch_bounds__(256) void filter2d_mirror_f64_kernel(const float* __restrict__ src, const double* __restrict__ kernels, int kmax,
                                                                  const int* __restrict__ ksize, int c, int h, int w, int tiles_x,
                                                                  float* __restrict__ out) {
  constexpr int kPitch = kB64Cols + kB64MaxK - 1;                 // 88
  constexpr int kTileRows = kB64Rows + kB64MaxK - 1 + 8;          // the unrolled window may address (never use) 8 rows past the halo
  __shared__ float tile[kTileRows * kPitch];
  const int plane = blockIdx.y, img = plane / c;
  const int ty_base = (blockIdx.x / tiles_x) * kB64Rows, tx_base = (blockIdx.x % tiles_x) * kB64Cols;
  const float* sp = src + (size_t)plane * h * w;
  float* op = out + (size_t)plane * h * w;
  int k = ksize[img];
  if (k < 3 || k > kmax || !(k & 1)) k = 0;                        // the host refuses such sizes where it can see them; here they copy through
  if (k == 0) {
    for (int i = threadIdx.x; i < kB64Rows * kB64Cols; i += 256) {
      const int y = ty_base + i / kB64Cols, x = tx_base + i % kB64Cols;
      if (y < h && x < w) op[(size_t)y * w + x] = sp[(size_t)y * w + x];
    }
    return;
  }
  const int r = k / 2, in_rows = kB64Rows + k - 1, in_cols = kB64Cols + k - 1;
  for (int i = threadIdx.x; i < in_rows * in_cols; i += 256) {
    const int iy = i / in_cols, ix = i - iy * in_cols;
    tile[iy * kPitch + ix] = sp[(size_t)b64_mirror(ty_base + iy - r, h) * w + b64_mirror(tx_base + ix - r, w)];
  }
  for (int i = in_rows * kPitch + threadIdx.x; i < (in_rows + 8) * kPitch; i += 256) tile[i] = 0.f;   // addressed by the window, never used
  __syncthreads();
  const int off = (kmax - k) / 2;
  const double* kw = kernels + (size_t)img * kmax * kmax + (size_t)off * kmax + off;
  const int tx = threadIdx.x & 63, ty0 = (threadIdx.x >> 6) * 8;
  double acc[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) acc[o] = 0.0;
  for (int kx = 0; kx < k; ++kx) {
    const float* col = tile + ty0 * kPitch + tx + kx;
    double win[8];
#pragma unroll
    for (int o = 0; o < 7; ++o) win[o] = (double)col[o * kPitch];
    for (int ky0 = 0; ky0 < k; ky0 += 8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ky = ky0 + j;
        if (ky < k) {                                              // wave-uniform
          win[(j + 7) & 7] = (double)col[(ky + 7) * kPitch];
          const double wv = kw[ky * kmax + kx];
#pragma unroll
          for (int o = 0; o < 8; ++o) acc[o] = fma(wv, win[(j + o) & 7], acc[o]);
        }
      }
    }
  }
  const int x = tx_base + tx;
  if (x >= w) return;
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    const int y = ty_base + ty0 + o;
    if (y >= h) break;
    op[(size_t)y * w + x] = (float)acc[o];
  }
}

extern "C" int srganfd_filter2d_mirror_f64(const float* src, const double* kernels, int32_t kmax, const int32_t* ksize, const int32_t* ksize_host, int32_t b,
                                           int32_t c, int32_t h, int32_t w, float* out, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!src || !kernels || !ksize || !out) return set_err(SRGANFD_EINVAL, "filter2d_mirror_f64: null pointer");
  if (b <= 0 || c <= 0 || h <= 0 || w <= 0) return set_err(SRGANFD_EINVAL, "filter2d_mirror_f64: bad args (b %d, c %d, %d x %d: all must be positive)", b, c, h, w);
  if (kmax < 3 || kmax > kB64MaxK || kmax % 2 == 0) return set_err(SRGANFD_EINVAL, "filter2d_mirror_f64: kmax %d is not an odd size from 3 to %d", kmax, kB64MaxK);
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
  if (need / 2 >= h || need / 2 >= w)
    return set_err(SRGANFD_EINVAL, "filter2d_mirror_f64: mirror padding %d needs an image larger than that (%d x %d)", need / 2, h, w);
  if ((long long)b * c > 65535) return set_err(SRGANFD_EINVAL, "filter2d_mirror_f64: more than 65535 planes");
  const int tiles_x = ceil_div(w, kB64Cols), tiles_y = ceil_div(h, kB64Rows);
  SRGANFD_LAUNCH(filter2d_mirror_f64_kernel, dim3(tiles_x * tiles_y, b * c), dim3(256), 0, s, src, kernels, kmax, ksize, c, h, w, tiles_x, out);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

}  // namespace srganfd
