// lpips.hip -- LPIPS v0.1 on AlexNet (the `lpips` package's LPIPS(net='alex'), eval mode, spatial=False) in fp32, forward only:
// the decision metric of the reference's validate() (train_bsrgan.py:115,571; bsrgan_config.py:65).
//
//   lpips_conv_kernel<KS, STRIDE, PAD, MODE>   implicit GEMM on v_mfma_f32_32x32x2_f32 (an exact fp32 fma chain): 64 output pixels x
//       64 output channels per workgroup, four waves of one 32 x 32 accumulator each, K walked in chunks of 32 staged in LDS
//       (global -> registers for chunk i + 1 is issued before the MFMA phase of chunk i); each chunk is summed from zero and
//       added to the running total (blocked summation).  The pixel axis is the flat index over
//       (image, y, x), so any H, W runs and only the last tile is predicated.  Bias and ReLU in the epilogue, NHWC fp32 out.
//       MODE 0  the 11 x 11 stride-4 conv on the caller's two NCHW images (any strides: the test scripts pass slices), the 2N
//               batch formed by reading in0 for the first half and in1 for the second; the scaling layer (and the optional
//               2x - 1) is applied to in-bounds taps while staging, a padded tap stays 0.  K = 363 in (c, ky, kx) order, the
//               rows 363..383 of the last chunk are zero-filled in LDS.
//       MODE 1  NHWC input, K = (ky, kx, c) with c fastest: a chunk is 32 channels of one tap, 16-byte loads.
//       MODE 2  the same through MaxPool(3, 2) (floor, no padding): the 3 x 3 maximum of the stored map is taken while staging,
//               the pooled map never exists in memory.
//   lpips_head_kernel      one wave per pixel of a tap: channel L2 norms of both images' vectors, normalised squared difference
//       weighted by lin_k, reduced over the wave by a fixed butterfly -> one float per pixel.
//   lpips_finish_kernel    one workgroup per image: the spatial mean of every tap in a fixed order (strided partial sums, LDS
//       tree), the per-tap values and their sum.  No floating-point atomics anywhere: two runs are bit-equal.
#include "common.hpp"

namespace srganfd {

static constexpr int kLpTM = 64, kLpTN = 64, kLpKC = 32, kLpThreads = 256;
static constexpr int kLpLdA = kLpKC + 1;              // A tile [pixel][k]: the MFMA read (lane -> pixel, k) is then conflict free
static constexpr int kLpTaps = 5;
static constexpr int kLpChannels[kLpTaps] = {64, 192, 384, 256, 256};

struct LpipsConvK {
  const float* x;                 // MODE 1, 2: (n, h_src, w_src, cin) fp32
  const float* in0;               // MODE 0: the two (n / 2, 3, h_src, w_src) images and their element strides
  const float* in1;
  long long s0[4], s1[4];
  const float* w;                 // [ktotal][cout]
  const float* bias;              // [cout]
  float* y;                       // (n, h_out, w_out, cout)
  int n, h_src, w_src;            // stored input
  int h_in, w_in;                 // the conv's logical input (the pooled dims in MODE 2)
  int cin, cout, h_out, w_out, ktotal, nchunks;
  long long m_total;
  float shift[3], scale[3], in_mul, in_add;
};

template <int KS, int STRIDE, int PAD, int MODE>
__global__ __launch_bounds__(kLpThreads) void lpips_conv_kernel(const LpipsConvK a) {
  __shared__ float As[kLpTM * kLpLdA];
  __shared__ __attribute__((aligned(16))) float Bs[kLpKC * kLpTN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = (long long)blockIdx.x * kLpTM;
  const int n0 = blockIdx.y * kLpTN;
  // staging roles.  A: pixels pr and pr + 32 of the tile, 4 consecutive k at kq.  B: rows br and br + 16, 4 columns at bc.
  const int kq = (tid & 7) * 4, pr = tid >> 3;
  const int br = tid >> 4, bc = (tid & 15) * 4;
  int img[2], oy[2], ox[2];
  bool pv[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long long m = m0 + pr + 32 * i;
    pv[i] = m < a.m_total;
    const long long mm = pv[i] ? m : 0;
    const int per = a.h_out * a.w_out;
    img[i] = (int)(mm / per);
    const int r = (int)(mm - (long long)img[i] * per);
    oy[i] = r / a.w_out;
    ox[i] = r - oy[i] * a.w_out;
  }
  float av[2][4];
  f32x4 bv[2];

  auto fetch = [&](int chunk) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int k = chunk * kLpKC + br + 16 * i;
      bv[i] = k < a.ktotal ? *(const f32x4*)(a.w + (size_t)k * a.cout + n0 + bc) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if constexpr (MODE == 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float* base = img[i] < a.n / 2 ? a.in0 + (long long)img[i] * a.s0[0] : a.in1 + (long long)(img[i] - a.n / 2) * a.s1[0];
        const long long sc = img[i] < a.n / 2 ? a.s0[1] : a.s1[1], sy = img[i] < a.n / 2 ? a.s0[2] : a.s1[2], sx = img[i] < a.n / 2 ? a.s0[3] : a.s1[3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = chunk * kLpKC + kq + j;
          const int ci = k / (KS * KS), r = k - ci * (KS * KS), ky = r / KS, kx = r - ky * KS;
          const int iy = oy[i] * STRIDE - PAD + ky, ix = ox[i] * STRIDE - PAD + kx;
          float v = 0.f;
          if (pv[i] && k < a.ktotal && iy >= 0 && iy < a.h_in && ix >= 0 && ix < a.w_in) {
            const float raw = base[ci * sc + iy * sy + ix * sx] * a.in_mul + a.in_add;
            const float sh = ci == 0 ? a.shift[0] : (ci == 1 ? a.shift[1] : a.shift[2]);
            const float sl = ci == 0 ? a.scale[0] : (ci == 1 ? a.scale[1] : a.scale[2]);
            v = (raw - sh) / sl;
          }
          av[i][j] = v;
        }
      }
    } else {
      const int cpb = a.cin / kLpKC;
      const int tap = chunk / cpb, ch = (chunk - tap * cpb) * kLpKC + kq;
      const int ky = tap / KS, kx = tap - ky * KS;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int iy = oy[i] * STRIDE - PAD + ky, ix = ox[i] * STRIDE - PAD + kx;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (pv[i] && iy >= 0 && iy < a.h_in && ix >= 0 && ix < a.w_in) {
          if constexpr (MODE == 1) {
            v = *(const f32x4*)(a.x + (((size_t)img[i] * a.h_src + iy) * a.w_src + ix) * a.cin + ch);
          } else {
            // floor pooling without padding: rows 2 iy .. 2 iy + 2 and columns 2 ix .. 2 ix + 2 are all inside the stored map
            const float* p = a.x + (((size_t)img[i] * a.h_src + 2 * iy) * a.w_src + 2 * ix) * a.cin + ch;
            v = *(const f32x4*)p;
#pragma unroll
            for (int t = 1; t < 9; ++t) {
              const f32x4 u = *(const f32x4*)(p + ((size_t)(t / 3) * a.w_src + (t % 3)) * a.cin);
#pragma unroll
              for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], u[j]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) av[i][j] = v[j];
      }
    }
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  fetch(0);
  for (int chunk = 0; chunk < a.nchunks; ++chunk) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) As[(pr + 32 * i) * kLpLdA + kq + j] = av[i][j];
      *(f32x4*)(Bs + (br + 16 * i) * kLpTN + bc) = bv[i];
    }
    __syncthreads();
    if (chunk + 1 < a.nchunks) fetch(chunk + 1);
    const float* ap = As + (wm + (lane & 31)) * kLpLdA + (lane >> 5);
    const float* bp = Bs + (lane >> 5) * kLpTN + wn + (lane & 31);
    // a chunk's 32 terms are one fma chain from zero, and the chunks' sums are added to the running total: blocked summation.
    // One chain over all of K (up to 3456 terms) carries about four times the rounding error in the per-layer values.
    f32x16 part;
#pragma unroll
    for (int r = 0; r < 16; ++r) part[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < kLpKC; kk += 2) part = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], bp[kk * kLpTN], part, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] += part[r];
    __syncthreads();
  }
  const int col = n0 + wn + (lane & 31);
  const float b = a.bias[col];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long m = m0 + wm + mfma32_row(r, lane);
    if (m < a.m_total) a.y[(size_t)m * a.cout + col] = fmaxf(acc[r] + b, 0.f);
  }
}

// ---- head ----
struct LpipsTapK {
  const float* f;      // (2 n, hw, c): image i's pixels, then at n + i the other input's
  const float* lin;    // [c]
  int hw, c;
  long long pix_off;   // floats from `pix`: this tap's (n, hw) per-pixel values
};
struct LpipsHeadK {
  LpipsTapK t[kLpTaps];
  int ntaps, n;
  long long waves;     // n * sum of hw
  float* pix;
  float* out;          // (ntaps + 1, n): the per-tap values, then their sum
};

__device__ __forceinline__ float lpips_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void lpips_head_kernel(const LpipsHeadK a) {
  const int lane = threadIdx.x & 63;
  long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= a.waves) return;
  int k = 0;
  while (k + 1 < a.ntaps && g >= (long long)a.n * a.t[k].hw) { g -= (long long)a.n * a.t[k].hw; ++k; }
  const LpipsTapK t = a.t[k];
  const int img = (int)(g / t.hw), p = (int)(g - (long long)img * t.hw);
  const float* f0 = t.f + ((size_t)img * t.hw + p) * t.c;
  const float* f1 = t.f + ((size_t)(a.n + img) * t.hw + p) * t.c;
  float v0[6], v1[6], s0 = 0.f, s1 = 0.f;
  const int per = t.c >> 6;                      // 1, 3, 6 or 4 channels per lane
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    v0[j] = j < per ? f0[lane + 64 * j] : 0.f;
    v1[j] = j < per ? f1[lane + 64 * j] : 0.f;
    s0 += v0[j] * v0[j];
    s1 += v1[j] * v1[j];
  }
  const float d0 = sqrtf(lpips_wave_sum(s0)) + 1e-10f, d1 = sqrtf(lpips_wave_sum(s1)) + 1e-10f;
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    if (j < per) {
      const float d = v0[j] / d0 - v1[j] / d1;
      acc += t.lin[lane + 64 * j] * (d * d);
    }
  }
  acc = lpips_wave_sum(acc);
  if (lane == 0) a.pix[t.pix_off + g] = acc;
}

__global__ __launch_bounds__(256) void lpips_finish_kernel(const LpipsHeadK a) {
  __shared__ float red[256];
  const int img = blockIdx.x, tid = threadIdx.x;
  float total = 0.f;
  for (int k = 0; k < a.ntaps; ++k) {
    const int hw = a.t[k].hw;
    const float* p = a.pix + a.t[k].pix_off + (size_t)img * hw;
    float s = 0.f;
    for (int i = tid; i < hw; i += 256) s += p[i];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    const float sk = red[0] / (float)hw;
    __syncthreads();
    total += sk;
    if (tid == 0) a.out[(size_t)k * a.n + img] = sk;
  }
  if (tid == 0) a.out[(size_t)a.ntaps * a.n + img] = total;
}

// ---- host side ----
// sizes of the five tap maps of an h x w input; false when a pool would see a map smaller than its window
static bool lpips_maps(int h, int w, int* th, int* tw) {
  if (h < 11 - 4 || w < 11 - 4) return false;
  th[0] = (h + 4 - 11) / 4 + 1; tw[0] = (w + 4 - 11) / 4 + 1;
  if (th[0] < 3 || tw[0] < 3) return false;
  th[1] = (th[0] - 3) / 2 + 1; tw[1] = (tw[0] - 3) / 2 + 1;
  if (th[1] < 3 || tw[1] < 3) return false;
  th[2] = th[3] = th[4] = (th[1] - 3) / 2 + 1;
  tw[2] = tw[3] = tw[4] = (tw[1] - 3) / 2 + 1;
  return true;
}

extern "C" int64_t srganfd_lpips_workspace_bytes(int32_t n, int32_t h, int32_t w) {
  int th[kLpTaps], tw[kLpTaps];
  if (n < 1) { set_err(SRGANFD_EINVAL, "lpips: batch size %d", n); return -1; }
  if (!lpips_maps(h, w, th, tw)) {
    set_err(SRGANFD_EINVAL, "lpips: a %d x %d image is too small: AlexNet's second 3 x 3 max-pool needs a 7 x 7 first feature map, "
            "so H and W must be at least 31", h, w);
    return -1;
  }
  int64_t floats = 0;
  for (int k = 0; k < kLpTaps; ++k) floats += (int64_t)th[k] * tw[k] * (2 * (int64_t)n * kLpChannels[k] + n);   // the map, and one value per pixel
  if (2 * (int64_t)n * th[0] * tw[0] > 0x7fffffffLL / 64) { set_err(SRGANFD_EINVAL, "lpips: %d images of %d x %d exceed the 32-bit pixel index", n, h, w); return -1; }
  return floats * 4;
}

template <int KS, int STRIDE, int PAD, int MODE> static void lpips_conv_launch(const LpipsConvK& k, hipStream_t s) {
  const dim3 grid((unsigned)((k.m_total + kLpTM - 1) / kLpTM), k.cout / kLpTN);
  SRGANFD_LAUNCH((lpips_conv_kernel<KS, STRIDE, PAD, MODE>), grid, dim3(kLpThreads), 0, s, k);
}

extern "C" int srganfd_lpips_conv(const srganfd_lpips_conv_args* a, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!a) return set_err(SRGANFD_EINVAL, "lpips_conv: null arguments");
  if (!a->w || !a->bias || !a->y) return set_err(SRGANFD_EINVAL, "lpips_conv: null weight, bias or output pointer");
  if (a->n < 1 || a->h_in < 1 || a->w_in < 1) return set_err(SRGANFD_EINVAL, "lpips_conv: bad input dims n %d, %d x %d", a->n, a->h_in, a->w_in);
  if (a->cout < kLpTN || a->cout % kLpTN) return set_err(SRGANFD_EINVAL, "lpips_conv: cout %d is not a multiple of %d", a->cout, kLpTN);
  const bool first = a->first != 0, pool = a->pool != 0;
  const bool shape_first = a->ksize == 11 && a->stride == 4 && a->pad == 2, shape5 = a->ksize == 5 && a->stride == 1 && a->pad == 2,
             shape3 = a->ksize == 3 && a->stride == 1 && a->pad == 1;
  if (first ? (!shape_first || a->cin != 3 || pool) : !(shape5 || shape3))
    return set_err(SRGANFD_EINVAL, "lpips_conv: ksize %d stride %d pad %d cin %d pool %d first %d has no kernel (first: 11,4,2 on 3 channels without "
                   "pool; else 5,1,2 or 3,1,1)", a->ksize, a->stride, a->pad, a->cin, a->pool, a->first);
  if (!first && (a->cin < kLpKC || a->cin % kLpKC)) return set_err(SRGANFD_EINVAL, "lpips_conv: cin %d is not a multiple of %d", a->cin, kLpKC);
  LpipsConvK k = {};
  k.h_src = a->h_in; k.w_src = a->w_in;
  k.h_in = a->h_in; k.w_in = a->w_in;
  if (pool) {
    if (a->h_in < 3 || a->w_in < 3) return set_err(SRGANFD_EINVAL, "lpips_conv: a %d x %d map is smaller than the 3 x 3 pool window", a->h_in, a->w_in);
    k.h_in = (a->h_in - 3) / 2 + 1; k.w_in = (a->w_in - 3) / 2 + 1;
  }
  const int ho = (k.h_in + 2 * a->pad - a->ksize) / a->stride + 1, wo = (k.w_in + 2 * a->pad - a->ksize) / a->stride + 1;
  if (k.h_in + 2 * a->pad < a->ksize || k.w_in + 2 * a->pad < a->ksize || ho != a->h_out || wo != a->w_out)
    return set_err(SRGANFD_EINVAL, "lpips_conv: output %d x %d does not follow from input %d x %d (expected %d x %d)", a->h_out, a->w_out, a->h_in, a->w_in, ho, wo);
  k.m_total = (long long)a->n * ho * wo;
  if (k.m_total > 0x7fffffffLL / kLpTM) return set_err(SRGANFD_EINVAL, "lpips_conv: %lld output pixels exceed the 32-bit tile index", k.m_total);
  if (first) {
    if (!a->in0 || !a->in1 || (a->n & 1)) return set_err(SRGANFD_EINVAL, "lpips_conv: the first conv needs both images and an even batch (n = 2 N), have n %d", a->n);
    for (int c = 0; c < 3; ++c)
      if (!(a->scale[c] != 0.f)) return set_err(SRGANFD_EINVAL, "lpips_conv: scaling layer scale[%d] is zero", c);
    k.in0 = a->in0; k.in1 = a->in1;
    for (int i = 0; i < 4; ++i) { k.s0[i] = a->stride0[i]; k.s1[i] = a->stride1[i]; }
    for (int c = 0; c < 3; ++c) { k.shift[c] = a->shift[c]; k.scale[c] = a->scale[c]; }
    k.in_mul = a->normalize ? 2.f : 1.f; k.in_add = a->normalize ? -1.f : 0.f;
  } else {
    if (!a->x || ((uintptr_t)a->x & 15)) return set_err(SRGANFD_EINVAL, "lpips_conv: null or unaligned (16 bytes) input map");
  }
  if ((uintptr_t)a->w & 15) return set_err(SRGANFD_EINVAL, "lpips_conv: the weights must be 16-byte aligned");
  k.x = a->x; k.w = a->w; k.bias = a->bias; k.y = a->y;
  k.n = a->n; k.cin = a->cin; k.cout = a->cout; k.h_out = ho; k.w_out = wo;
  k.ktotal = a->ksize * a->ksize * a->cin;
  k.nchunks = (k.ktotal + kLpKC - 1) / kLpKC;
  if (first) lpips_conv_launch<11, 4, 2, 0>(k, s);
  else if (shape5) { if (pool) lpips_conv_launch<5, 1, 2, 2>(k, s); else lpips_conv_launch<5, 1, 2, 1>(k, s); }
  else { if (pool) lpips_conv_launch<3, 1, 1, 2>(k, s); else lpips_conv_launch<3, 1, 1, 1>(k, s); }
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

extern "C" int srganfd_lpips_head(const srganfd_lpips_tap* taps, int32_t ntaps, int32_t n, float* out, float* ws, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!taps || !out || !ws) return set_err(SRGANFD_EINVAL, "lpips_head: null pointer");
  if (ntaps < 1 || ntaps > kLpTaps || n < 1) return set_err(SRGANFD_EINVAL, "lpips_head: %d taps (1..%d), n %d", ntaps, kLpTaps, n);
  LpipsHeadK k = {};
  long long off = 0;
  for (int i = 0; i < ntaps; ++i) {
    const srganfd_lpips_tap& t = taps[i];
    if (!t.maps || !t.lin) return set_err(SRGANFD_EINVAL, "lpips_head: tap %d has a null pointer", i);
    if (t.h < 1 || t.w < 1 || (long long)t.h * t.w * n > 0x7fffffffLL) return set_err(SRGANFD_EINVAL, "lpips_head: tap %d is %d x %d", i, t.h, t.w);
    if (t.c < 64 || t.c > 384 || t.c % 64) return set_err(SRGANFD_EINVAL, "lpips_head: tap %d has %d channels; a multiple of 64 up to 384 is needed", i, t.c);
    k.t[i].f = t.maps; k.t[i].lin = t.lin; k.t[i].hw = t.h * t.w; k.t[i].c = t.c; k.t[i].pix_off = off;
    off += (long long)n * t.h * t.w;
  }
  if ((off + 3) / 4 > 0x7fffffffLL) return set_err(SRGANFD_EINVAL, "lpips_head: %lld pixels exceed the grid", off);
  k.ntaps = ntaps; k.n = n; k.waves = off; k.pix = ws; k.out = out;
  SRGANFD_LAUNCH(lpips_head_kernel, dim3((unsigned)((off + 3) / 4)), dim3(256), 0, s, k);
  SRGANFD_LAUNCH(lpips_finish_kernel, dim3(n), dim3(256), 0, s, k);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

}  // namespace srganfd
