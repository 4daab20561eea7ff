// layout.hip -- layout / dtype conversion at the module boundary: NCHW fp32 <-> NHWC bf16/f16/f32 views, the clamp's gradient mask
// folded into the relayout, the batch crop and the uint8 HWC ingest of the data side.  NCHW -> NHWC has three forms: one per-pixel
// kernel for c <= 4 image planes into a whole 16-bit buffer (rgb_to_nhwc_kernel, with or without the clamp mask, chosen by rgb_ok /
// whole_pitch of elementwise.hpp), and the generic body's vector and scalar widths (vec_ok).
#include "elementwise.hpp"

namespace srganfd {

// What the relayouts take: an NCHW fp32 batch (n images of c planes of hw pixels) on one side, an NHWC view on the other, zero padded
// to cpad channels where it is written.  nchw_to_nhwc: src -> view, with (x - mean[ch]) / stdv[ch] when mean is given.  clamp_grad:
// src = d sr, pre = the pre-clamp SR (fp32), view = the gradient.  nhwc_to_nchw (+ scaled): view -> dst.
struct LayK { const float* src; float* dst; View view, pre; int n, c, hw, cpad; const float *mean, *stdv, *ch_div; int clamp01; };

// ---- NCHW fp32 -> NHWC T view, zero padded to cpad channels (BSRGAN.forward input, model.py:366): vector form N = VecN<T>::N, scalar N = 1 ----
template <typename T, int N>
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const LayK k) {
  for_each_group<N>((size_t)k.n * k.hw, k.cpad, [&](size_t p, int ck) {
    const size_t img = p / k.hw, pix = p % k.hw;
    float v[N];
    each<N>([&](int q) {
      const int ch = ck + q;
      float t = 0.f;
      if (ch < k.c) {
        t = k.src[(img * k.c + ch) * k.hw + pix];
        if (k.mean) t = (t - k.mean[ch]) / k.stdv[ch];
      }
      v[q] = t;
    });
    stn<T, N>(k.view.p, k.view.at(p, ck), v);
  });
}

// ---- NHWC view (T or fp32) -> NCHW fp32, optional clamp to [0,1] (model.py:379) ----
template <typename T>
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const LayK k) {
  grid_stride((size_t)k.n * k.c * k.hw, [&](size_t i) {
    const size_t pix = i % k.hw;
    const size_t t = i / k.hw;
    const int ch = (int)(t % k.c);
    const size_t img = t / k.c;
    float v = ld<T>(k.view.p, k.view.at(img * k.hw + pix, ch));
    if (k.clamp01) v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);       // torch's clamp_: a NaN stays a NaN (fminf(fmaxf(v, 0), 1) made it 0), -0 stays -0
    k.dst[i] = v;
  });
}

// ---- gradient of clamp_(0,1) + NCHW fp32 -> NHWC T (zero padded): d pre = (0 <= pre <= 1) ? d sr : 0 ----
template <typename T>
__global__ __launch_bounds__(256) void clamp_grad_kernel(const LayK k) {
  for_each_group<1>((size_t)k.n * k.hw, k.cpad, [&](size_t p, int ch) {
    const size_t img = p / k.hw, pix = p % k.hw;
    float v = 0.f;
    if (ch < k.c) {
      const float q = ((const float*)k.pre.p)[k.pre.at(p, ch)];
      if (q >= 0.f && q <= 1.f) v = k.src[(img * k.c + ch) * k.hw + pix];
    }
    st<T>(k.view.p, k.view.at(p, ch), v);
  });
}

// ---- the per-pixel forms: c <= 4 image planes into a 16-bit view that is a whole buffer.  One thread per pixel, c coalesced plane reads,
// the pixel packed once.  CLAMP: the clamp's gradient mask, from one 16-byte read of the pre-clamp pixel (fp32, 4-channel pitch); without
// it the input normalisation.  WIDE = false: a 4-channel pitch ("NHWC4", the thin-side kernels' operand, conv_thin.hip), one 8-byte store.
// WIDE = true: the generator's gradient padded to 32 channels, four 16-byte stores (the 29 padding channels are zeros the data-gradient
// conv multiplies by padded weights).
template <typename T, bool CLAMP, bool WIDE>
__global__ __launch_bounds__(256) void rgb_to_nhwc_kernel(const LayK k) {
  static_assert(CLAMP || !WIDE, "the input side has the 4-channel pitch only");
  const size_t hw = k.hw;
  grid_stride((size_t)k.n * hw, [&](size_t p) {
    const size_t img = p / hw, pix = p % hw;
    f32x4 q = {0.f, 0.f, 0.f, 0.f};
    if constexpr (CLAMP) q = ((const f32x4*)k.pre.p)[p];
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < k.c && (!CLAMP || (q[j] >= 0.f && q[j] <= 1.f))) {
        float t = k.src[(img * k.c + j) * hw + pix];
        if constexpr (!CLAMP) { if (k.mean) t = (t - k.mean[j]) / k.stdv[j]; }
        v[j] = t;
      }
    const u32x4 w0 = pack8<T>(v);
    if constexpr (WIDE) {
      u32x4* dst = (u32x4*)k.view.p;
      const u32x4 z = {0u, 0u, 0u, 0u};
      dst[p * 4 + 0] = w0; dst[p * 4 + 1] = z; dst[p * 4 + 2] = z; dst[p * 4 + 3] = z;
    } else {
      ((unsigned long long*)k.view.p)[p] = (unsigned long long)w0[0] | ((unsigned long long)w0[1] << 32);
    }
  });
}

// the differentiable VGG tap's relayout (ESRGAN/model.py:281-292): NHWC fp32 -> NCHW that also undoes the 1/std of the input normalisation
__global__ __launch_bounds__(256) void nhwc_to_nchw_scaled_kernel(const LayK k) {
  grid_stride((size_t)k.n * k.c * k.hw, [&](size_t i) {
    const size_t pix = i % k.hw;
    const size_t t = i / k.hw;
    const int ch = (int)(t % k.c);
    const size_t img = t / k.c;
    k.dst[i] = ((const float*)k.view.p)[k.view.at(img * k.hw + pix, ch)] / k.ch_div[ch];
  });
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
  const size_t npix = (size_t)n * h * w;
  const LayK k = {src, nullptr, dev_view(dst), {}, n, c, h * w, cpad, mean, stdv, nullptr, 0};
  if (rgb_ok(dtype, c, cpad, 4) && whole_pitch(dst, 4, 8)) {
    DISPATCH_T16(dtype, SRGANFD_LAUNCH((rgb_to_nhwc_kernel<TT, false, false>), dim3(grid_for(npix)), dim3(256), 0, s, k));
  } else {
    DISPATCH_TN(dtype, vec_ok(dtype, cpad, {dst}), SRGANFD_LAUNCH((nchw_to_nhwc_kernel<TT, NN>), group_grid(npix * cpad, NN), dim3(256), 0, s, k));
  }
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_nhwc_to_nchw(srganfd_view src, int32_t dtype, int32_t n, int32_t c, int32_t h, int32_t w, float* dst, int32_t clamp01, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!src.ptr || !dst || src.c0 + c > src.cstride) return set_err(SRGANFD_EINVAL, "nhwc_to_nchw: bad args");
  if (src.planar) return set_err(SRGANFD_EINVAL, "nhwc_to_nchw: NHWC views only, not planar ones");
  const LayK k = {nullptr, dst, dev_view(src), {}, n, c, h * w, 0, nullptr, nullptr, nullptr, clamp01};
  DISPATCH_T(dtype, SRGANFD_LAUNCH(nhwc_to_nchw_kernel<TT>, dim3(grid_for((size_t)n * h * w * c)), dim3(256), 0, s, k));
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_clamp_grad_to_nhwc(const float* dsr, srganfd_view pre, int32_t n, int32_t c, int32_t h, int32_t w, srganfd_view dst, int32_t dtype,
                                          int32_t cpad, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!dsr || !pre.ptr || !dst.ptr || dst.c0 + cpad > dst.cstride) return set_err(SRGANFD_EINVAL, "clamp_grad: bad args");
  if (pre.planar || dst.planar) return set_err(SRGANFD_EINVAL, "clamp_grad: NHWC views only, not planar ones");
  const size_t npix = (size_t)n * h * w;
  const LayK k = {dsr, nullptr, dev_view(dst), dev_view(pre), n, c, h * w, cpad, nullptr, nullptr, nullptr, 0};
  if (rgb_ok(dtype, c, cpad, 4) && whole_pitch(pre, 4, 16) && whole_pitch(dst, 4, 8)) {
    DISPATCH_T16(dtype, SRGANFD_LAUNCH((rgb_to_nhwc_kernel<TT, true, false>), dim3(grid_for(npix)), dim3(256), 0, s, k));
  } else if (rgb_ok(dtype, c, cpad, 32) && whole_pitch(pre, 4, 16) && whole_pitch(dst, 32, 16)) {
    DISPATCH_T16(dtype, SRGANFD_LAUNCH((rgb_to_nhwc_kernel<TT, true, true>), dim3(grid_for(npix)), dim3(256), 0, s, k));
  } else {
    DISPATCH_T(dtype, SRGANFD_LAUNCH(clamp_grad_kernel<TT>, dim3(grid_for(npix * cpad)), dim3(256), 0, s, k));
  }
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}
extern "C" int srganfd_nhwc_to_nchw_scaled(srganfd_view src, int32_t n, int32_t c, int32_t h, int32_t w, float* dst, const float* ch_div, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!src.ptr || !dst || !ch_div || n <= 0 || c <= 0) return set_err(SRGANFD_EINVAL, "nhwc_to_nchw_scaled: bad args");
  if (src.planar) return set_err(SRGANFD_EINVAL, "nhwc_to_nchw_scaled: NHWC views only, not planar ones");
  const LayK k = {nullptr, dst, dev_view(src), {}, n, c, h * w, 0, nullptr, nullptr, ch_div, 0};
  SRGANFD_LAUNCH(nhwc_to_nchw_scaled_kernel, dim3(grid_for((size_t)n * c * h * w)), dim3(256), 0, s, k);
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
