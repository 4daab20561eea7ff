// layout.hip -- layout / dtype conversion at the module boundary: NCHW fp32 <-> NHWC bf16/f16/f32 views, the clamp's gradient mask
// folded into the relayout, the batch crop and the uint8 HWC ingest of the data side.
#include "elementwise.hpp"

namespace srganfd {

// ---- NCHW fp32 -> NHWC T view, zero padded to cpad channels (BSRGAN.forward input, model.py:366) ----
template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ src, void* dst, int dC, int d0, int n, int c, int hw, int cpad,
                                    const float* __restrict__ mean, const float* __restrict__ stdv) {
  const size_t total = (size_t)n * hw * cpad;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % cpad);
    const size_t p = i / cpad;
    const size_t img = p / hw, pix = p % hw;
    float v = 0.f;
    if (ch < c) {
      v = src[(img * c + ch) * hw + pix];
      if (mean) v = (v - mean[ch]) / stdv[ch];
    }
    st<T>(dst, p * dC + d0 + ch, v);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void nchw_to_nhwc_vec_kernel(const float* __restrict__ src, void* dst, int dC, int d0, int n, int c, int hw, int cpad,
                                                               const float* __restrict__ mean, const float* __restrict__ stdv) {
  constexpr int N = VecN<T>::N;
  const int cv = cpad / N;
  const size_t total = (size_t)n * hw * cv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ck = (int)(i % cv) * N;
    const size_t p = i / cv;
    const size_t img = p / hw, pix = p % hw;
    float v[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const int ch = ck + q;
      float t = 0.f;
      if (ch < c) {
        t = src[(img * c + ch) * hw + pix];
        if (mean) t = (t - mean[ch]) / stdv[ch];
      }
      v[q] = t;
    }
    stv<T>(dst, p * dC + d0 + ck, v);
  }
}

// ---- NHWC view (T or fp32) -> NCHW fp32, optional clamp to [0,1] (model.py:379) ----
template <typename T>
__global__ void nhwc_to_nchw_kernel(const void* __restrict__ src, int sC, int s0, float* __restrict__ dst, int n, int c, int hw, int clamp01) {
  const size_t total = (size_t)n * c * hw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = i % hw;
    const size_t t = i / hw;
    const int ch = (int)(t % c);
    const size_t img = t / c;
    float v = ld<T>(src, (img * hw + pix) * sC + s0 + ch);
    if (clamp01) v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);       // torch's clamp_: a NaN stays a NaN (fminf(fmaxf(v, 0), 1) made it 0), -0 stays -0
    dst[i] = v;
  }
}

// ---- gradient of clamp_(0,1) + NCHW fp32 -> NHWC T (zero padded): d pre = (0 <= pre <= 1) ? d sr : 0 ----
template <typename T>
__global__ void clamp_grad_kernel(const float* __restrict__ dsr, const float* __restrict__ pre, int pC, int p0, void* dst, int dC, int d0,
                                  int n, int c, int hw, int cpad) {
  const size_t total = (size_t)n * hw * cpad;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % cpad);
    const size_t p = i / cpad;
    const size_t img = p / hw, pix = p % hw;
    float v = 0.f;
    if (ch < c) {
      const float q = pre[p * pC + p0 + ch];
      if (q >= 0.f && q <= 1.f) v = dsr[(img * c + ch) * hw + pix];
    }
    st<T>(dst, p * dC + d0 + ch, v);
  }
}

// the generator's case (3 image channels, fp32 pre-clamp SR with a 4-channel pitch, 16-bit gradient padded to 32 channels): one thread
// per pixel, one 16-byte read of the pre-clamp pixel, three coalesced plane reads, four 16-byte stores (the 29 padding channels are
// zeros the data-gradient conv multiplies by padded weights)
template <typename T>
__global__ __launch_bounds__(256) void clamp_grad_rgb16_kernel(const float* __restrict__ dsr, const f32x4* __restrict__ pre, u32x4* __restrict__ dst,
                                                               size_t npix, size_t hw, int c) {
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (size_t)gridDim.x * 256) {
    const size_t img = p / hw, pix = p % hw;
    const f32x4 q = pre[p];
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < c && q[k] >= 0.f && q[k] <= 1.f) v[k] = dsr[(img * c + k) * hw + pix];
    const float v8[8] = {v[0], v[1], v[2], v[3], 0.f, 0.f, 0.f, 0.f};
    const u32x4 w0 = pack8<T>(v8);
    const u32x4 z = {0u, 0u, 0u, 0u};
    dst[p * 4 + 0] = w0; dst[p * 4 + 1] = z; dst[p * 4 + 2] = z; dst[p * 4 + 3] = z;
  }
}

// the same into a 4-channel pitch ("NHWC4", 8 bytes per pixel): the thin-side kernels' operand (conv_thin.hip)
template <typename T>
__global__ __launch_bounds__(256) void clamp_grad_rgb4_kernel(const float* __restrict__ dsr, const f32x4* __restrict__ pre, unsigned long long* __restrict__ dst,
                                                              size_t npix, size_t hw, int c) {
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (size_t)gridDim.x * 256) {
    const size_t img = p / hw, pix = p % hw;
    const f32x4 q = pre[p];
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < c && q[k] >= 0.f && q[k] <= 1.f) v[k] = dsr[(img * c + k) * hw + pix];
    const u32x4 w0 = pack8<T>(v);
    dst[p] = (unsigned long long)w0[0] | ((unsigned long long)w0[1] << 32);
  }
}

// NCHW fp32 (c <= 4 planes) -> NHWC4 16-bit: one thread per pixel, c coalesced plane reads, one 8-byte store
template <typename T>
__global__ __launch_bounds__(256) void nchw_to_nhwc4_kernel(const float* __restrict__ src, unsigned long long* __restrict__ dst, size_t npix, size_t hw, int c,
                                                            const float* __restrict__ mean, const float* __restrict__ stdv) {
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (size_t)gridDim.x * 256) {
    const size_t img = p / hw, pix = p % hw;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < c) {
        float t = src[(img * c + k) * hw + pix];
        if (mean) t = (t - mean[k]) / stdv[k];
        v[k] = t;
      }
    const u32x4 w0 = pack8<T>(v);
    dst[p] = (unsigned long long)w0[0] | ((unsigned long long)w0[1] << 32);
  }
}

// the differentiable VGG tap's relayout (ESRGAN/model.py:281-292): NHWC fp32 -> NCHW that also undoes the 1/std of the input normalisation
__global__ __launch_bounds__(256) void nhwc_to_nchw_scaled_kernel(const float* __restrict__ src, int sC, int s0, float* __restrict__ dst, int n, int c,
                                                                  int hw, const float* __restrict__ ch_div) {
  const size_t total = (size_t)n * c * hw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t pix = i % hw;
    const size_t t = i / hw;
    const int ch = (int)(t % c);
    const size_t img = t / c;
    dst[i] = src[(img * hw + pix) * sC + s0 + ch] / ch_div[ch];
  }
}

// ------------------------------------------------------------------------------------------------
// validation / data side
// random_crop (imgproc.py:846-886): one (top, left) for the whole batch -> ONE strided copy instead of B slice copies
__global__ __launch_bounds__(256) void crop_nchw_kernel(const float* __restrict__ src, float* __restrict__ dst, int planes, int h, int w, int top,
                                                        int left, int ph, int pw) {
  const size_t total = (size_t)planes * ph * pw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int x = (int)(i % pw);
    const size_t t = i / pw;
    const int y = (int)(t % ph);
    const size_t pl = t / ph;
    dst[i] = src[(pl * h + top + y) * w + left + x];
  }
}

// ---- uint8 ingest (dataset.py:64-96): what the reference does per image on the host -- cv2.imread(...).astype(float32) / 255,
// crop, BGR -> RGB, image_to_tensor's HWC -> CHW (imgproc.py:331-358) -- for a whole batch of decoded uint8 HWC images on the device:
// a quarter of the host-to-device bytes, and the float batch never exists in host memory.  One thread per output pixel: three byte reads
// of one pixel (a wave reads 192 contiguous bytes), three coalesced plane stores.
__global__ __launch_bounds__(256) void u8hwc_to_nchw_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int n, int h, int w, int top, int left,
                                                            int ph, int pw, int swap_rb, float scale) {
  const size_t total = (size_t)n * ph * pw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int x = (int)(i % pw);
    const size_t t = i / pw;
    const int y = (int)(t % ph);
    const size_t img = t / ph;
    const unsigned char* p = src + ((img * h + top + y) * (size_t)w + left + x) * 3;
    const float c0 = (float)p[0] / scale, c1 = (float)p[1] / scale, c2 = (float)p[2] / scale;
    float* d = dst + (img * 3 * ph + y) * (size_t)pw + x;
    const size_t plane = (size_t)ph * pw;
    d[0] = swap_rb ? c2 : c0;
    d[plane] = c1;
    d[2 * plane] = swap_rb ? c0 : c2;
  }
}

// ------------------------------------------------------------------------------------------------
extern "C" int srganfd_nchw_to_nhwc(const float* src, int32_t n, int32_t c, int32_t h, int32_t w, srganfd_view dst, int32_t dtype, int32_t cpad,
                                    const float* mean, const float* stdv, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!src || !dst.ptr || n <= 0 || c <= 0 || cpad < c || dst.c0 + cpad > dst.cstride) return set_err(SRGANFD_EINVAL, "nchw_to_nhwc: bad args");
  if (dst.planar) return set_err(SRGANFD_EINVAL, "nchw_to_nhwc: NHWC views only, not planar ones");
  const size_t total = (size_t)n * h * w * cpad;
  if (dtype != SRGANFD_F32 && c <= 4 && cpad == 4 && dst.cstride == 4 && dst.c0 == 0 && ((uintptr_t)dst.ptr & 7) == 0) {
    const size_t npix = (size_t)n * h * w;
    if (dtype == SRGANFD_BF16) SRGANFD_LAUNCH(nchw_to_nhwc4_kernel<bf16_t>, dim3(grid_for(npix)), dim3(256), 0, s, src, (unsigned long long*)dst.ptr, npix, (size_t)h * w, c, mean, stdv);
    else SRGANFD_LAUNCH(nchw_to_nhwc4_kernel<f16_t>, dim3(grid_for(npix)), dim3(256), 0, s, src, (unsigned long long*)dst.ptr, npix, (size_t)h * w, c, mean, stdv);
    SRGANFD_HIP_CHECK(hipGetLastError());
    return SRGANFD_OK;
  }
  {
    const int vn = dtype == SRGANFD_F32 ? 4 : 8;
    if (cpad % vn == 0 && dst.c0 % vn == 0 && dst.cstride % vn == 0 && ((uintptr_t)dst.ptr & 15) == 0) {
      DISPATCH_T(dtype,
                 SRGANFD_LAUNCH(nchw_to_nhwc_vec_kernel<TT>, dim3(grid_for(total / vn, 256, 65536)), dim3(256), 0, s, src, dst.ptr, dst.cstride, dst.c0, n, c, h * w, cpad, mean, stdv));
      SRGANFD_HIP_CHECK(hipGetLastError());
      return SRGANFD_OK;
    }
  }
  DISPATCH_T(dtype,
             SRGANFD_LAUNCH(nchw_to_nhwc_kernel<TT>, dim3(grid_for(total)), dim3(256), 0, s, src, dst.ptr, dst.cstride, dst.c0, n, c, h * w, cpad, mean, stdv));
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_nhwc_to_nchw(srganfd_view src, int32_t dtype, int32_t n, int32_t c, int32_t h, int32_t w, float* dst, int32_t clamp01, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!src.ptr || !dst || src.c0 + c > src.cstride) return set_err(SRGANFD_EINVAL, "nhwc_to_nchw: bad args");
  if (src.planar) return set_err(SRGANFD_EINVAL, "nhwc_to_nchw: NHWC views only, not planar ones");
  const size_t total = (size_t)n * h * w * c;
  DISPATCH_T(dtype,
             SRGANFD_LAUNCH(nhwc_to_nchw_kernel<TT>, dim3(grid_for(total)), dim3(256), 0, s, src.ptr, src.cstride, src.c0, dst, n, c, h * w, clamp01));
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_clamp_grad_to_nhwc(const float* dsr, srganfd_view pre, int32_t n, int32_t c, int32_t h, int32_t w, srganfd_view dst, int32_t dtype,
                                          int32_t cpad, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!dsr || !pre.ptr || !dst.ptr || dst.c0 + cpad > dst.cstride) return set_err(SRGANFD_EINVAL, "clamp_grad: bad args");
  if (pre.planar || dst.planar) return set_err(SRGANFD_EINVAL, "clamp_grad: NHWC views only, not planar ones");
  const size_t total = (size_t)n * h * w * cpad;
  if (dtype != SRGANFD_F32 && c <= 4 && cpad == 4 && pre.cstride == 4 && pre.c0 == 0 && dst.cstride == 4 && dst.c0 == 0 &&
      ((uintptr_t)pre.ptr & 15) == 0 && ((uintptr_t)dst.ptr & 7) == 0) {
    const size_t npix = (size_t)n * h * w;
    if (dtype == SRGANFD_BF16) SRGANFD_LAUNCH(clamp_grad_rgb4_kernel<bf16_t>, dim3(grid_for(npix)), dim3(256), 0, s, dsr, (const f32x4*)pre.ptr, (unsigned long long*)dst.ptr, npix, (size_t)h * w, c);
    else SRGANFD_LAUNCH(clamp_grad_rgb4_kernel<f16_t>, dim3(grid_for(npix)), dim3(256), 0, s, dsr, (const f32x4*)pre.ptr, (unsigned long long*)dst.ptr, npix, (size_t)h * w, c);
    SRGANFD_HIP_CHECK(hipGetLastError());
    return SRGANFD_OK;
  }
  if (dtype != SRGANFD_F32 && c <= 4 && cpad == 32 && pre.cstride == 4 && pre.c0 == 0 && dst.cstride == 32 && dst.c0 == 0 &&
      ((uintptr_t)pre.ptr & 15) == 0 && ((uintptr_t)dst.ptr & 15) == 0) {
    const size_t npix = (size_t)n * h * w;
    if (dtype == SRGANFD_BF16) SRGANFD_LAUNCH(clamp_grad_rgb16_kernel<bf16_t>, dim3(grid_for(npix)), dim3(256), 0, s, dsr, (const f32x4*)pre.ptr, (u32x4*)dst.ptr, npix, (size_t)h * w, c);
    else SRGANFD_LAUNCH(clamp_grad_rgb16_kernel<f16_t>, dim3(grid_for(npix)), dim3(256), 0, s, dsr, (const f32x4*)pre.ptr, (u32x4*)dst.ptr, npix, (size_t)h * w, c);
    SRGANFD_HIP_CHECK(hipGetLastError());
    return SRGANFD_OK;
  }
  DISPATCH_T(dtype,
             SRGANFD_LAUNCH(clamp_grad_kernel<TT>, dim3(grid_for(total)), dim3(256), 0, s, dsr, (const float*)pre.ptr, pre.cstride, pre.c0, dst.ptr, dst.cstride, dst.c0, n, c, h * w, cpad));
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_nhwc_to_nchw_scaled(srganfd_view src, int32_t n, int32_t c, int32_t h, int32_t w, float* dst, const float* ch_div, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!src.ptr || !dst || !ch_div || n <= 0 || c <= 0) return set_err(SRGANFD_EINVAL, "nhwc_to_nchw_scaled: bad args");
  if (src.planar) return set_err(SRGANFD_EINVAL, "nhwc_to_nchw_scaled: NHWC views only, not planar ones");
  SRGANFD_LAUNCH(nhwc_to_nchw_scaled_kernel, dim3(grid_for((size_t)n * c * h * w)), dim3(256), 0, s, (const float*)src.ptr, src.cstride, src.c0, dst, n, c, h * w, ch_div);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_crop_nchw(const float* src, float* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t top, int32_t left, int32_t ph, int32_t pw,
                                 void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!src || !dst || n <= 0 || c <= 0 || top < 0 || left < 0 || ph <= 0 || pw <= 0 || top + ph > h || left + pw > w)
    return set_err(SRGANFD_EINVAL, "crop: window %dx%d at (%d,%d) outside %dx%d", ph, pw, top, left, h, w);
  SRGANFD_LAUNCH(crop_nchw_kernel, dim3(grid_for((size_t)n * c * ph * pw)), dim3(256), 0, s, src, dst, n * c, h, w, top, left, ph, pw);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_u8hwc_to_nchw(const unsigned char* src, float* dst, int32_t n, int32_t h, int32_t w, int32_t top, int32_t left, int32_t ph, int32_t pw,
                                     int32_t swap_rb, float scale, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!src || !dst || n <= 0 || ph <= 0 || pw <= 0 || top < 0 || left < 0 || top + ph > h || left + pw > w || !(scale > 0.f))
    return set_err(SRGANFD_EINVAL, "u8hwc_to_nchw: bad args / window outside the image");
  SRGANFD_LAUNCH(u8hwc_to_nchw_kernel, dim3(grid_for((size_t)n * ph * pw)), dim3(256), 0, s, src, dst, n, h, w, top, left, ph, pw, swap_rb, scale);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

}  // namespace srganfd
