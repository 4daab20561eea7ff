// jpeg.hip -- the two JPEG round trips (encode at a quality, decode) of the degradation pipelines on NCHW fp32 RGB batches.  They share the
// frame (McuLane: one wavefront per 16 x 16 MCU = 4 luma blocks + Cb + Cr, four MCUs per 256-thread workgroup) and the standard
// quantisation tables.  The arithmetic of each is its own, and with it the LDS layout that arithmetic wants (fp32: luma as one 16 x 16 plane;
// int32: six blocks of row pitch 9).
//
// srganfd_jpeg_roundtrip: a real baseline JPEG, the integer pipeline of libjpeg's defaults (4:2:0, the slow-but-accurate integer DCT, fancy
// chroma upsampling), which BSRGAN's blind degradation runs per image on the host through cv2.imencode / cv2.imdecode
// (BSRGAN/imgproc.py:284-293).  Entropy coding is lossless, so it is not there; what is left is integer arithmetic in int32, and the
// result equals the library's byte for byte (tests/jpeg_oracle.py is the same restated in numpy).
//   jpeg_mcu_kernel     one wave per MCU: quantise to bytes, RGB -> YCbCr (16-bit fixed point), 2 x 2 chroma
//                       average (bias 1, 2, 1, 2 ... along a row), then for the four luma and two chroma blocks the forward DCT, the
//                       quantiser (|c| + 4 q) / (8 q), the product with q, the inverse DCT and the + 128 clamp, rows and columns through LDS;
//                       decoded Y (full size) and Cb / Cr (half size) go to a byte workspace.
//   jpeg_finish_kernel  one thread per pixel: the triangle-filter upsampling of the chroma planes cropped to ceil(h / 2) x ceil(w / 2), which
//                       needs the neighbouring MCUs' chroma (hence the second launch), YCbCr -> RGB, float(u8) / 255.
// Edges as the library pads them: columns are replicated before the chroma average, rows after it (an odd height's last row is doubled
// first), so the last chroma row of an even height is a true average of two rows, repeated downwards.
// quality[b] lives in device memory; 0 leaves that image's planes as they are (copied through, bit for bit).
//
// srganfd_diff_jpeg: Real-ESRGAN's DiffJPEG (Real_ESRGAN/imgproc.py:1198-1497), fp32 throughout; see diff_jpeg_kernel.
#include <math.h>
#include "elementwise.hpp"

namespace srganfd {

static constexpr int kJpgWaves = 4;          // MCUs per workgroup
static constexpr int kJpgPitch = 9;          // ints per block row in LDS: rows and columns of a block both fall in distinct banks
static constexpr int kJpgBlock = 8 * kJpgPitch;
static constexpr int kJpgMcuBytes = 384;     // 256 Y + 64 Cb + 64 Cr of workspace per MCU

// the standard luminance and chrominance quantisation tables (JPEG Annex K), in libjpeg's natural order: [frequency row][frequency column]
static constexpr unsigned char kJpgLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                               69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                               81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92, 95,  98,  112, 100, 103, 99};
static constexpr unsigned char kJpgChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                                 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// A lane's place in a grid of ceil(b * mcus_y * mcus_x / 4) workgroups of 256: wave -> MCU (img, my, mx), live = there is one; lane l owns the
// 2 x 2 pixel quad (qy, qx) = (l / 8, l % 8) of the MCU on the way in and out, and coefficient / sample (qy, qx) of each 8 x 8 block in between.
struct McuLane {
  int wave, lane, qy, qx, img, my, mx;
  long long per_img;
  bool live;
  __device__ __forceinline__ McuLane(int b, int mcus_x, int mcus_y)
      : wave(threadIdx.x >> 6), lane(threadIdx.x & 63), qy(lane >> 3), qx(lane & 7), img(0), my(0), mx(0), per_img((long long)mcus_x * mcus_y) {
    const long long mcu = (long long)blockIdx.x * kJpgWaves + wave;
    live = mcu < b * per_img;
    if (live) {
      img = (int)(mcu / per_img);
      const int rem = (int)(mcu % per_img);
      my = rem / mcus_x;
      mx = rem % mcus_x;
    }
  }
  // pixel j = 0 .. 3 of the quad (row-major): its row and column inside the MCU; + 16 * my / mx = in the image padded to whole MCUs
  __device__ __forceinline__ int quad_y(int j) const { return qy * 2 + (j >> 1); }
  __device__ __forceinline__ int quad_x(int j) const { return qx * 2 + (j & 1); }
  // the luma block (raster order, 0..3) that pixel (ly, lx) of the MCU falls in; Cb is block 4, Cr block 5
  __device__ static __forceinline__ int luma_block(int ly, int lx) { return (ly >> 3) * 2 + (lx >> 3); }
};

// 13-bit constants of the integer DCT
#define JF_0_298 2446
#define JF_0_390 3196
#define JF_0_541 4433
#define JF_0_765 6270
#define JF_0_899 7373
#define JF_1_175 9633
#define JF_1_501 12299
#define JF_1_847 15137
#define JF_1_961 16069
#define JF_2_053 16819
#define JF_2_562 20995
#define JF_3_072 25172

__device__ __forceinline__ int jdescale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 8-point forward pass on p[0], p[stride], ...: FIRST = the row pass (results scaled up by 4), else the column pass
template <bool FIRST>
__device__ __forceinline__ void jpeg_fdct8(int* p, int stride) {
  int d[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) d[i] = p[i * stride];
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int n = FIRST ? 11 : 15;
  p[0] = FIRST ? (t10 + t11) * 4 : jdescale(t10 + t11, 2);
  p[4 * stride] = FIRST ? (t10 - t11) * 4 : jdescale(t10 - t11, 2);
  int z1 = (t12 + t13) * JF_0_541;
  p[2 * stride] = jdescale(z1 + t13 * JF_0_765, n);
  p[6 * stride] = jdescale(z1 - t12 * JF_1_847, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * JF_1_175;
  const int a4 = t4 * JF_0_298, a5 = t5 * JF_2_053, a6 = t6 * JF_3_072, a7 = t7 * JF_1_501;
  z1 = -z1 * JF_0_899; z2 = -z2 * JF_2_562; z3 = -z3 * JF_1_961 + z5; z4 = -z4 * JF_0_390 + z5;
  p[7 * stride] = jdescale(a4 + z1 + z3, n);
  p[5 * stride] = jdescale(a5 + z2 + z4, n);
  p[3 * stride] = jdescale(a6 + z2 + z3, n);
  p[1 * stride] = jdescale(a7 + z1 + z4, n);
}

// one 8-point inverse pass: FIRST = the column pass, else the row pass, whose results are the samples (+ 128, clamped to a byte)
template <bool FIRST>
__device__ __forceinline__ void jpeg_idct8(int* p, int stride) {
  int d[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) d[i] = p[i * stride];
  int z1 = (d[2] + d[6]) * JF_0_541;
  const int e2 = z1 - d[6] * JF_1_847, e3 = z1 + d[2] * JF_0_765;
  const int e0 = (d[0] + d[4]) * 8192, e1 = (d[0] - d[4]) * 8192;
  const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  int t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * JF_1_175;
  t0 *= JF_0_298; t1 *= JF_2_053; t2 *= JF_3_072; t3 *= JF_1_501;
  z1 = -z1 * JF_0_899; z2 = -z2 * JF_2_562; z3 = -z3 * JF_1_961 + z5; z4 = -z4 * JF_0_390 + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  constexpr int n = FIRST ? 11 : 18;
  int o[8] = {t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int v = jdescale(o[i], n);
    p[i * stride] = FIRST ? v : min(max(v + 128, 0), 255);
  }
}

__device__ __forceinline__ int jpeg_u8(float v) { return (int)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }

__global__ __launch_bounds__(64 * kJpgWaves) void jpeg_mcu_kernel(const float* __restrict__ src, int b, int h, int w, int mcus_x, int mcus_y,
                                                                  const int* __restrict__ quality, unsigned char* __restrict__ ws) {
  __shared__ int lds[kJpgWaves][6 * kJpgBlock];
  const McuLane m(b, mcus_x, mcus_y);
  const int lane = m.lane, qy = m.qy, qx = m.qx, my = m.my, mx = m.mx;
  bool live = m.live;
  int q = 0;
  if (live) {
    q = quality[m.img];
    live = q != 0;                       // the whole image is copied through by jpeg_finish_kernel
    q = min(max(q, 1), 100);             // as the library clamps it; the host refuses such values where it sees them
  }
  int* blk = lds[m.wave];
  const size_t plane = (size_t)h * w;
  const float* ps = src + (size_t)m.img * 3 * plane;
  if (live) {
    // this lane's 2 x 2 quad: luma at the pixel itself (clamped into the image), chroma from the rows the library averages
    const int h2 = (h + 1) >> 1;
    const int cyc = min(my * 8 + qy, h2 - 1);
    int cbs = 0, crs = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ly = m.quad_y(j), lx = m.quad_x(j);
      const int y = min(my * 16 + ly, h - 1), yc = min(2 * cyc + (ly & 1), h - 1), x = min(mx * 16 + lx, w - 1);
      size_t o = (size_t)y * w + x;
      int r = jpeg_u8(ps[o]), g = jpeg_u8(ps[plane + o]), bl = jpeg_u8(ps[2 * plane + o]);
      blk[McuLane::luma_block(ly, lx) * kJpgBlock + (ly & 7) * kJpgPitch + (lx & 7)] = ((19595 * r + 38470 * g + 7471 * bl + 32768) >> 16) - 128;
      if (yc != y) {                     // below the last chroma row: its samples repeat that row's
        o = (size_t)yc * w + x;
        r = jpeg_u8(ps[o]); g = jpeg_u8(ps[plane + o]); bl = jpeg_u8(ps[2 * plane + o]);
      }
      cbs += (-11059 * r - 21709 * g + 32768 * bl + (128 << 16) + 32767) >> 16;
      crs += (32768 * r - 27439 * g - 5329 * bl + (128 << 16) + 32767) >> 16;
    }
    const int bias = 1 + (qx & 1);
    blk[4 * kJpgBlock + qy * kJpgPitch + qx] = ((cbs + bias) >> 2) - 128;
    blk[5 * kJpgBlock + qy * kJpgPitch + qx] = ((crs + bias) >> 2) - 128;
  }
  __syncthreads();
  const int pb = lane >> 3, pi = lane & 7;         // the passes: lane -> (block, row or column); 48 of the 64 lanes work
  const bool worker = live && pb < 6;
  if (worker) jpeg_fdct8<true>(blk + pb * kJpgBlock + pi * kJpgPitch, 1);
  __syncthreads();
  if (worker) jpeg_fdct8<false>(blk + pb * kJpgBlock + pi, kJpgPitch);
  __syncthreads();
  if (live) {
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    const int ql = min(max(((int)kJpgLuma[lane] * s + 50) / 100, 1), 255), qc = min(max(((int)kJpgChroma[lane] * s + 50) / 100, 1), 255);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      int* p = blk + k * kJpgBlock + qy * kJpgPitch + qx;
      const int qv = k < 4 ? ql : qc, c = *p;
      const int a = (abs(c) + 4 * qv) / (8 * qv);
      *p = (c < 0 ? -a : a) * qv;
    }
  }
  __syncthreads();
  if (worker) jpeg_idct8<true>(blk + pb * kJpgBlock + pi, kJpgPitch);
  __syncthreads();
  if (worker) jpeg_idct8<false>(blk + pb * kJpgBlock + pi * kJpgPitch, 1);
  __syncthreads();
  if (live) {
    const int hp = mcus_y * 16, wp = mcus_x * 16;
    unsigned char* base = ws + (size_t)m.img * m.per_img * kJpgMcuBytes;
    {                                    // Y: lane -> row lane / 4, columns 4 * (lane % 4) ..: one 4-byte store
      const int ly = lane >> 2, lx = (lane & 3) * 4;
      const int* p = blk + McuLane::luma_block(ly, lx) * kJpgBlock + (ly & 7) * kJpgPitch + (lx & 7);
      const unsigned v = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
      *(unsigned*)(base + (size_t)(my * 16 + ly) * wp + mx * 16 + lx) = v;
    }
    if (lane < 32) {                     // Cb (lanes 0..15) and Cr (16..31): row l / 2, columns 4 * (l % 2) ..
      const int k = lane >> 4, l = lane & 15, cy = l >> 1, cx = (l & 1) * 4;
      const int* p = blk + (4 + k) * kJpgBlock + cy * kJpgPitch + cx;
      const unsigned v = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
      unsigned char* cp = base + (size_t)hp * wp + (size_t)k * (hp / 2) * (wp / 2);
      *(unsigned*)(cp + (size_t)(my * 8 + cy) * (wp / 2) + mx * 8 + cx) = v;
    }
  }
}

__global__ __launch_bounds__(256) void jpeg_finish_kernel(const float* __restrict__ src, int b, int h, int w, int mcus_x, int mcus_y,
                                                          const int* __restrict__ quality, const unsigned char* __restrict__ ws,
                                                          float* __restrict__ dst) {
  const size_t plane = (size_t)h * w, total = (size_t)b * plane;
  const int hp = mcus_y * 16, wp = mcus_x * 16, wc = wp / 2;
  const int h2 = (h + 1) >> 1, w2 = (w + 1) >> 1;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int img = (int)(i / plane);
    const size_t o = i - (size_t)img * plane;
    const float* ps = src + (size_t)img * 3 * plane + o;
    float* pd = dst + (size_t)img * 3 * plane + o;
    if (quality[img] == 0) {
      pd[0] = ps[0]; pd[plane] = ps[plane]; pd[2 * plane] = ps[2 * plane];
      continue;
    }
    const int y = (int)(o / w), x = (int)(o - (size_t)y * w);
    const unsigned char* base = ws + (size_t)img * mcus_x * mcus_y * kJpgMcuBytes;
    const int yy = base[(size_t)y * wp + x];
    const int cy = y >> 1, cx = x >> 1;
    int c[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const unsigned char* cp = base + (size_t)hp * wp + (size_t)k * (hp / 2) * wc;
      if (w2 <= 2) {                     // the library repeats a chroma plane this narrow instead of filtering it
        c[k] = cp[(size_t)cy * wc + cx];
      } else {
        const int ny = (y & 1) ? min(cy + 1, h2 - 1) : max(cy - 1, 0);
        const int nx = (x & 1) ? min(cx + 1, w2 - 1) : max(cx - 1, 0);
        const int here = 3 * cp[(size_t)cy * wc + cx] + cp[(size_t)ny * wc + cx];
        const int side = 3 * cp[(size_t)cy * wc + nx] + cp[(size_t)ny * wc + nx];
        c[k] = (3 * here + side + ((x & 1) ? 7 : 8)) >> 4;
      }
      c[k] -= 128;
    }
    const int r = yy + ((91881 * c[1] + 32768) >> 16);
    const int g = yy + ((-22554 * c[0] + 32768 - 46802 * c[1]) >> 16);
    const int bl = yy + ((116130 * c[0] + 32768) >> 16);
    pd[0] = (float)min(max(r, 0), 255) / 255.0f;
    pd[plane] = (float)min(max(g, 0), 255) / 255.0f;
    pd[2 * plane] = (float)min(max(bl, 0), 255) / 255.0f;
  }
}

extern "C" int64_t srganfd_jpeg_workspace_bytes(int32_t b, int32_t h, int32_t w) {
  if (b <= 0 || h <= 0 || w <= 0) return -1;
  return (long long)b * ceil_div(h, 16) * ceil_div(w, 16) * kJpgMcuBytes;
}

extern "C" int srganfd_jpeg_roundtrip(const float* src, int32_t b, int32_t c, int32_t h, int32_t w, const int32_t* quality, const int32_t* quality_host,
                                      void* workspace, float* dst, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!src || !dst || !quality || !workspace) return set_err(SRGANFD_EINVAL, "jpeg_roundtrip: null pointer");
  if (c != 3) return set_err(SRGANFD_EINVAL, "jpeg_roundtrip: needs 3-channel RGB input, got %d channels", c);
  if (b <= 0 || h <= 0 || w <= 0) return set_err(SRGANFD_EINVAL, "jpeg_roundtrip: bad args (b %d, %d x %d: all must be positive)", b, h, w);
  if (src == dst) return set_err(SRGANFD_EINVAL, "jpeg_roundtrip: the output may not alias the input");
  if ((uintptr_t)workspace & 3) return set_err(SRGANFD_EINVAL, "jpeg_roundtrip: the workspace must be 4-byte aligned");
  if (quality_host)
    for (int i = 0; i < b; ++i)
      if (quality_host[i] < 0 || quality_host[i] > 100)
        return set_err(SRGANFD_EINVAL, "jpeg_roundtrip: quality[%d] = %d is outside 0..100 (0 leaves the image as it is)", i, quality_host[i]);
  const int mcus_x = ceil_div(w, 16), mcus_y = ceil_div(h, 16);
  const long long total = (long long)b * mcus_x * mcus_y;
  if ((total + kJpgWaves - 1) / kJpgWaves > 0x7fffffffLL) return set_err(SRGANFD_EINVAL, "jpeg_roundtrip: %lld MCUs exceed the grid", total);
  SRGANFD_LAUNCH(jpeg_mcu_kernel, dim3((unsigned)((total + kJpgWaves - 1) / kJpgWaves)), dim3(64 * kJpgWaves), 0, s, src, b, h, w, mcus_x, mcus_y,
                 quality, (unsigned char*)workspace);
  SRGANFD_LAUNCH(jpeg_finish_kernel, dim3(grid_for((size_t)b * h * w, 256, 65536)), dim3(256), 0, s, src, b, h, w, mcus_x, mcus_y, quality,
                 (const unsigned char*)workspace, dst);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// DiffJPEG (imgproc.py:1198-1497): x255, RGB -> YCbCr, 2x2 chroma average, per 8x8 block DCT -> divide by
// table * factor -> round (or the cubic "differentiable" rounding, :1183-1195) -> multiply back -> inverse DCT, chroma
// repeat, YCbCr -> RGB, clamp to [0, 255], /255; the image is zero-padded to multiples of 16 and cropped back
// (:1482-1495).  The wavefront owns its MCU from load to store; nothing but the RGB input and output touches HBM.
// The 4-D cosine tensors are the reference's fp32 products (:1250-1252, :1366-1368), summed over all 64 terms like its tensordot.
// tables: [dct 4096 | idct 4096 | dct scale 64 | idct alpha 64 | y_table 64 | c_table 64] floats.
// ---------------------------------------------------------------------------------------------------------------
static constexpr int kJpegTableFloats = 4096 * 2 + 64 * 4;
extern "C" int32_t srganfd_diff_jpeg_table_floats(void) { return kJpegTableFloats; }

static void diff_jpeg_tables_host(float* t) {
  const double pi = 3.14159265358979323846;
  float* dct = t;
  float* idct = t + 4096;
  float* scale = t + 8192;
  float* alpha = scale + 64;
  float* ytab = alpha + 64;
  float* ctab = ytab + 64;
  for (int x = 0; x < 8; ++x)
    for (int y = 0; y < 8; ++y)
      for (int u = 0; u < 8; ++u)
        for (int v = 0; v < 8; ++v) {
          dct[((x * 8 + y) * 8 + u) * 8 + v] = (float)(cos((2 * x + 1) * u * pi / 16) * cos((2 * y + 1) * v * pi / 16));
          idct[((x * 8 + y) * 8 + u) * 8 + v] = (float)(cos((2 * u + 1) * x * pi / 16) * cos((2 * v + 1) * y * pi / 16));
        }
  for (int u = 0; u < 8; ++u)
    for (int v = 0; v < 8; ++v) {
      const double au = u == 0 ? 1.0 / sqrt(2.0) : 1.0, av = v == 0 ? 1.0 / sqrt(2.0) : 1.0;
      scale[u * 8 + v] = (float)(au * av * 0.25);
      alpha[u * 8 + v] = (float)(au * av);
      ytab[u * 8 + v] = kJpgLuma[v * 8 + u];                                 // the reference transposes the standard tables (:43-48)
      ctab[u * 8 + v] = kJpgChroma[v * 8 + u];
    }
}
extern "C" int srganfd_diff_jpeg_tables(float* host_out) {
  if (!host_out) return set_err(SRGANFD_EINVAL, "diff_jpeg_tables: null output");
  diff_jpeg_tables_host(host_out);
  return SRGANFD_OK;
}

__global__ __launch_bounds__(64 * kJpgWaves) void diff_jpeg_kernel(const float* __restrict__ src, int b, int h, int w, int mcus_x, int mcus_y,
                                                                   const float* __restrict__ factor, int differentiable,
                                                                   const float* __restrict__ tables, float* __restrict__ dst) {
  __shared__ float sp_all[kJpgWaves][384], cf_all[kJpgWaves][384];
  const McuLane m(b, mcus_x, mcus_y);
  const int lane = m.lane, qy = m.qy, qx = m.qx;
  float* sp = sp_all[m.wave];
  float* cf = cf_all[m.wave];
  const float* dct = tables;
  const float* idct = tables + 4096;
  const float* scale = tables + 8192;
  const float* alpha = scale + 64;
  const float* ytab = alpha + 64;
  const float* ctab = ytab + 64;
  const size_t plane = (size_t)h * w;
  const float* ps = src + (size_t)m.img * 3 * plane;
  // ---- load the quad, x255, RGB -> YCbCr (tensordot with the transposed matrix + shift, :1201-1212), chroma average (:1219-1226)
  {
    float cbs = 0.f, crs = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ly = m.quad_y(j), lx = m.quad_x(j), y = m.my * 16 + ly, x = m.mx * 16 + lx;
      float r = 0.f, g = 0.f, bl = 0.f;
      if (m.live && y < h && x < w) {
        const size_t o = (size_t)y * w + x;
        r = ps[o] * 255.f; g = ps[plane + o] * 255.f; bl = ps[2 * plane + o] * 255.f;
      }
      float yy = r * 0.299f; yy = fmaf(g, 0.587f, yy); yy = fmaf(bl, 0.114f, yy);
      float cb = r * -0.168736f; cb = fmaf(g, -0.331264f, cb); cb = fmaf(bl, 0.5f, cb); cb += 128.f;
      float cr = r * 0.5f; cr = fmaf(g, -0.418688f, cr); cr = fmaf(bl, -0.081312f, cr); cr += 128.f;
      sp[ly * 16 + lx] = yy;
      cbs += cb; crs += cr;
    }
    sp[256 + qy * 8 + qx] = cbs * 0.25f;
    sp[320 + qy * 8 + qx] = crs * 0.25f;
  }
  __syncthreads();
  const float f = m.live ? factor[m.img] : 1.f;
  // ---- forward DCT of the six blocks, quantise, round, de-quantise, x alpha (:1254-1259, :1270-1278, :1183-1195, :1333-1340, :1371)
  {
#pragma unroll 1
    for (int blk = 0; blk < 6; ++blk) {
      const float* xb = blk < 4 ? sp + ((blk >> 1) * 8) * 16 + (blk & 1) * 8 : sp + 256 + (blk - 4) * 64;
      const int pitch = blk < 4 ? 16 : 8;
      float acc = 0.f;
#pragma unroll
      for (int x = 0; x < 8; ++x)
#pragma unroll
        for (int y = 0; y < 8; ++y) acc = fmaf(xb[x * pitch + y] - 128.f, dct[(x * 8 + y) * 64 + lane], acc);
      const float coef = scale[lane] * acc;
      const float tab = (blk < 4 ? ytab[lane] : ctab[lane]) * f;
      const float q = coef / tab;
      float rq = rintf(q);                                        // torch.round: half to even
      if (differentiable) { const float d = q - rq; rq = rq + d * d * d; }
      cf[blk * 64 + qy * 8 + qx] = (rq * tab) * alpha[lane];
    }
  }
  __syncthreads();
  // ---- inverse DCT (:1370-1374): pixel (qy, qx) of each block = 0.25 * sum_uv X[u,v] * idct[u,v,qy,qx] + 128
  {
#pragma unroll 1
    for (int blk = 0; blk < 6; ++blk) {
      const float* xb = cf + blk * 64;
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < 64; ++i) acc = fmaf(xb[i], idct[i * 64 + lane], acc);
      const float pv = 0.25f * acc + 128.f;
      if (blk < 4) sp[((blk >> 1) * 8 + qy) * 16 + (blk & 1) * 8 + qx] = pv;
      else sp[256 + (blk - 4) * 64 + qy * 8 + qx] = pv;
    }
  }
  __syncthreads();
  // ---- chroma repeat (:1396-1407), YCbCr -> RGB (:1414-1424), clamp and /255 (:1459-1460), crop (:1495)
  if (m.live) {
    const float cb = sp[256 + qy * 8 + qx] - 128.f, cr = sp[320 + qy * 8 + qx] - 128.f;
    float* pd = dst + (size_t)m.img * 3 * plane;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ly = m.quad_y(j), lx = m.quad_x(j), y = m.my * 16 + ly, x = m.mx * 16 + lx;
      if (y < h && x < w) {
        const float yy = sp[ly * 16 + lx];
        float r = yy * 1.f; r = fmaf(cb, 0.f, r); r = fmaf(cr, 1.402f, r);
        float g = yy * 1.f; g = fmaf(cb, -0.344136f, g); g = fmaf(cr, -0.714136f, g);
        float bl = yy * 1.f; bl = fmaf(cb, 1.772f, bl); bl = fmaf(cr, 0.f, bl);
        const size_t o = (size_t)y * w + x;
        pd[o] = fminf(255.f, fmaxf(0.f, r)) / 255.f;
        pd[plane + o] = fminf(255.f, fmaxf(0.f, g)) / 255.f;
        pd[2 * plane + o] = fminf(255.f, fmaxf(0.f, bl)) / 255.f;
      }
    }
  }
}

// quality -> factor in place, as DiffJPEG.forward does on the tensor it is given (:1476-1480, :1127-1144)
__global__ void jpeg_quality_factor_kernel(float* q, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float v = q[i];
    const float t = v < 50.f ? 5000.f / v : 200.f - v * 2.f;
    q[i] = t / 100.f;
  }
}

extern "C" int srganfd_diff_jpeg(const float* src, int32_t b, int32_t c, int32_t h, int32_t w, float* quality, int32_t quality_is_factor,
                                 int32_t differentiable, const float* tables, float* dst, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!src || !dst || !quality || !tables || b <= 0 || h <= 0 || w <= 0) return refuse_empty("diff_jpeg");
  if (c != 3) return set_err(SRGANFD_EINVAL, "diff_jpeg: needs 3-channel RGB input, got %d channels", c);
  const int mcus_x = ceil_div(w, 16), mcus_y = ceil_div(h, 16);
  const long long total = (long long)b * mcus_x * mcus_y;
  if (total > (1ll << 32)) return set_err(SRGANFD_EINVAL, "diff_jpeg: too many blocks");
  if (!quality_is_factor) SRGANFD_LAUNCH(jpeg_quality_factor_kernel, dim3(ceil_div(b, 256)), dim3(256), 0, s, quality, b);
  SRGANFD_LAUNCH(diff_jpeg_kernel, dim3((unsigned)((total + kJpgWaves - 1) / kJpgWaves)), dim3(64 * kJpgWaves), 0, s, src, b, h, w, mcus_x, mcus_y,
                 (const float*)quality, differentiable, tables, dst);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

}  // namespace srganfd
