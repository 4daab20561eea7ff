// imresize.hip -- MATLAB's imresize as the reference's data side runs it (ESRGAN/imgproc.py:202-288: cubic a = -0.5, stretched by 1/scale
// when it shrinks with antialiasing, symmetric padding, rows then columns, float32).  The weights and first source indices of every output
// row and column are tables the host builds (sr_gan_fd_amd/imgproc.py); this file applies them.
//   imresize_kernel  one workgroup per T x T output tile of one plane, one launch per call:
//     1. stage the tile's input footprint in LDS (16-byte row reads for tiles inside an image whose rows are aligned, the symmetric
//        rule at the borders; all of a thread's loads issued before its stores), together with the tile's rows of both weight tables;
//     2. vertical pass: T output rows x every staged column, four columns per thread -> a second LDS array (the intermediate never
//        goes to HBM and is rounded to float32 there, as the reference's out_1 is);
//     3. horizontal pass -> dst.
// Step 3 reads the intermediate at addresses about 1/scale floats apart for neighbouring output columns.  When the image shrinks,
// neighbouring lanes therefore take neighbouring output ROWS (the array's pitch is odd, so they fall in different banks) and the tile goes
// through LDS once more for row-contiguous stores; when it grows, neighbouring columns read the same or the next float and lanes follow them.
// When it shrinks, tiles are also renumbered so that the workgroups sharing an XCD's L2 walk neighbouring tiles (halos hit the L2).
// No MFMA: at most a few dozen taps per pass on 3-channel images; the kernel moves bytes.
#include "common.hpp"

namespace srganfd {

static constexpr int kImrThreads = 256;
static constexpr size_t kImrLdsMax = 64 * 1024;   // two workgroups or more per CU of the 160 KB
static constexpr int kImrWeightDepth = 2;         // rounds of weight loads kept in registers across the staging (T * taps is 256 at 1/4 and 1/8)
static constexpr int kImrStageDepth = 8;          // staging loads a thread keeps in flight (the 80 x 80 footprint at 1/4 is 1680 groups of 4: 7 per thread)

struct ImresizeArgs {
  const float* src;
  float* dst;
  const float* wt_h;
  const int* first_h;
  const float* wt_w;
  const int* first_w;
  int h, w, oh, ow, taps_h, taps_w;
  int tile;          // T
  int tiles_x, tiles_y;
  int cap_h, cap_w;  // rows / columns of the staged footprint the LDS plan has room for (cap_w a multiple of 4)
  int mid_pitch;     // odd, >= cap_w
  int stage_floats;  // cap_h * cap_w, at least T * T (the output tile reuses the array)
  int vec;           // rows of src are 16-byte aligned
};

// MATLAB symmetric padding (-1 -> 0, n -> n - 1); whatever lies further out than one reflection is clamped into the image: the host
// refuses such tables, and a tile overhanging the image stages columns no stored output reads
__device__ __forceinline__ int imr_reflect(int j, int n) {
  j = j < 0 ? -1 - j : (j >= n ? 2 * n - 1 - j : j);
  return min(max(j, 0), n - 1);
}

// grid (tiles_x * tiles_y * planes) when ROWS_FAST, else (tiles_x, tiles_y, planes); dynamic LDS: ImresizePlan::lds
template <bool ROWS_FAST>
__global__ __launch_bounds__(kImrThreads) void imresize_kernel(const ImresizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float imr_lds[];
  const int T = a.tile, SP = a.cap_w, MP = a.mid_pitch;
  float* stage = imr_lds;
  float* mid = stage + a.stage_floats;
  float* wh = mid + T * MP;
  float* ww = wh + T * a.taps_h;
  int* base_h = (int*)(ww + T * a.taps_w);
  int* base_w = base_h + T;
  const int tid = threadIdx.x;
  // Workgroups are handed to the 8 XCDs (each with its own L2) round robin, so with the plain order no two neighbouring tiles share an
  // L2 and every halo is fetched from beyond it again (measured: 1.9x the input bytes at 1/4, 1.0x with the remap).  When the image
  // shrinks, the grid is 1-D and the workgroups that share an XCD (id % 8: a label, not the XCD's number) get one contiguous run of
  // tiles, row by row, plane by plane; the remap is a bijection of 0 .. gridDim.x - 1 whatever the placement really is, so only the
  // speed depends on it.  When the image grows there is next to no halo, and the plain 3-D grid, which spreads neighbouring output
  // tiles over the XCDs, stores faster (measured both ways).
  int tile_x = blockIdx.x, tile_y = blockIdx.y, plane = blockIdx.z;
  if (ROWS_FAST) {
    const int nwg = gridDim.x, q = nwg >> 3, rem = nwg & 7, label = blockIdx.x & 7;
    const int tile_id = (label < rem ? label * (q + 1) : rem * (q + 1) + (label - rem) * q) + (blockIdx.x >> 3);
    const int rest = tile_id / a.tiles_x;
    tile_x = tile_id - rest * a.tiles_x;
    plane = rest / a.tiles_y;
    tile_y = rest - plane * a.tiles_y;
  }
  const int oy0 = tile_y * T, ox0 = tile_x * T;
  const int ty = min(T, a.oh - oy0), tx = min(T, a.ow - ox0);
  const int lo_y = a.first_h[oy0];
  const int lo_x = a.first_w[ox0] & ~3;      // rounded down to a multiple of 4 (also when negative): staged groups of 4 match aligned 16-byte reads
  // what this tile reads; never more than the plan holds (the host sized it from in / out, see imresize_cap)
  const int ny = min(max(a.first_h[oy0 + ty - 1] + a.taps_h - lo_y, a.taps_h), a.cap_h);
  const int nx = min(max(a.first_w[ox0 + tx - 1] + a.taps_w - lo_x, a.taps_w), a.cap_w);
  const int ngrp = (nx + 3) >> 2, nx4 = ngrp * 4;

  // The tile's rows of both weight tables and the first staged row / column of each of its outputs (kept inside what was staged
  // whatever the table holds) are loaded now and stored after the staging loads have been issued: one memory round trip, not two.
  const int nwh = ty * a.taps_h, nww = tx * a.taps_w;
  float wreg_h[kImrWeightDepth], wreg_w[kImrWeightDepth];
#pragma unroll
  for (int q = 0; q < kImrWeightDepth; ++q) {
    const int i = tid + q * kImrThreads;
    wreg_h[q] = i < nwh ? a.wt_h[(size_t)oy0 * a.taps_h + i] : 0.f;
    wreg_w[q] = i < nww ? a.wt_w[(size_t)ox0 * a.taps_w + i] : 0.f;
  }
  int first_reg = 0;
  if (tid < ty) first_reg = a.first_h[oy0 + tid];
  if (tid >= 64 && tid - 64 < tx) first_reg = a.first_w[ox0 + tid - 64];

  // Staging.  Every thread issues all its loads of a round before it stores any of them (kImrStageDepth 16-byte loads, or as many
  // scalar ones, in flight per thread): a load-store-load chain would pay the memory latency once per staged row group.
  const float* p = a.src + (size_t)plane * a.h * a.w;
  const int nitems = ny * ngrp;
  const bool interior = a.vec && lo_y >= 0 && lo_y + ny <= a.h && lo_x >= 0 && lo_x + nx4 <= a.w;     // the same for the whole workgroup
  if (interior) {
    for (int i0 = tid; i0 < nitems; i0 += kImrThreads * kImrStageDepth) {
      f32x4 v[kImrStageDepth];
#pragma unroll
      for (int u = 0; u < kImrStageDepth; ++u) {
        const int i = i0 + u * kImrThreads;
        if (i < nitems) {
          const int r = i / ngrp, g = i - r * ngrp;
          v[u] = *(const f32x4*)(p + (size_t)(lo_y + r) * a.w + lo_x + 4 * g);
        }
      }
#pragma unroll
      for (int u = 0; u < kImrStageDepth; ++u) {
        const int i = i0 + u * kImrThreads;
        if (i < nitems) {
          const int r = i / ngrp, g = i - r * ngrp;
          *(f32x4*)(stage + r * SP + 4 * g) = v[u];
        }
      }
    }
  } else {      // a tile at the image's border, or rows that are not 16-byte aligned: scalar reads through the symmetric rule
    for (int i0 = tid; i0 < nitems; i0 += kImrThreads * (kImrStageDepth / 2)) {
      f32x4 v[kImrStageDepth / 2];
#pragma unroll
      for (int u = 0; u < kImrStageDepth / 2; ++u) {
        const int i = i0 + u * kImrThreads;
        if (i < nitems) {
          const int r = i / ngrp, g = i - r * ngrp;
          const float* row = p + (size_t)imr_reflect(lo_y + r, a.h) * a.w;
          const int x0 = lo_x + 4 * g;
#pragma unroll
          for (int j = 0; j < 4; ++j) v[u][j] = row[imr_reflect(x0 + j, a.w)];
        }
      }
#pragma unroll
      for (int u = 0; u < kImrStageDepth / 2; ++u) {
        const int i = i0 + u * kImrThreads;
        if (i < nitems) {
          const int r = i / ngrp, g = i - r * ngrp;
          *(f32x4*)(stage + r * SP + 4 * g) = v[u];
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kImrWeightDepth; ++q) {
    const int i = tid + q * kImrThreads;
    if (i < nwh) wh[i] = wreg_h[q];
    if (i < nww) ww[i] = wreg_w[q];
  }
  for (int i = tid + kImrWeightDepth * kImrThreads; i < nwh; i += kImrThreads) wh[i] = a.wt_h[(size_t)oy0 * a.taps_h + i];   // very long kernels only
  for (int i = tid + kImrWeightDepth * kImrThreads; i < nww; i += kImrThreads) ww[i] = a.wt_w[(size_t)ox0 * a.taps_w + i];
  if (tid < ty) base_h[tid] = min(max(first_reg - lo_y, 0), ny - a.taps_h);
  if (tid >= 64 && tid - 64 < tx) base_w[tid - 64] = min(max(first_reg - lo_x, 0), nx - a.taps_w);
  __syncthreads();

  // rows (H) first: one thread per output row and group of 4 staged columns (one 16-byte LDS read and one weight per 4 multiply-adds)
  for (int i = tid; i < ty * ngrp; i += kImrThreads) {
    const int r = i / ngrp, g = i - r * ngrp;
    const float* s = stage + base_h[r] * SP + 4 * g;
    const float* wr = wh + r * a.taps_h;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k = 0; k < a.taps_h; ++k) {
      const float wk = wr[k];
      const f32x4 v = *(const f32x4*)(s + k * SP);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(wk, v[j], acc[j]);
    }
    float* m = mid + r * MP + 4 * g;       // odd pitch: four scalar stores
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = acc[j];
  }
  __syncthreads();

  float* dplane = a.dst + (size_t)plane * a.oh * a.ow;
  for (int i = tid; i < ty * tx; i += kImrThreads) {         // then columns (W)
    int r, c;
    if (ROWS_FAST) { c = i / ty; r = i - c * ty; } else { r = i / tx; c = i - r * tx; }
    const float* m = mid + r * MP + base_w[c];
    const float* wr = ww + c * a.taps_w;
    float acc = 0.f;
#pragma unroll 4
    for (int k = 0; k < a.taps_w; ++k) acc = fmaf(wr[k], m[k], acc);
    if (ROWS_FAST) stage[r * T + c] = acc;                   // the staged input is dead since the barrier above
    else dplane[(size_t)(oy0 + r) * a.ow + ox0 + c] = acc;
  }
  if (ROWS_FAST) {
    __syncthreads();
    for (int i = tid; i < ty * tx; i += kImrThreads) {
      const int r = i / tx, c = i - r * tx;
      dplane[(size_t)(oy0 + r) * a.ow + ox0 + c] = stage[r * T + c];
    }
  }
}

// Staged samples along one side that a tile of T outputs can need.  out = ceil(in * scale) gives 1 / scale < in / (out - 1), and the first
// source index floor(u - width / 2) advances by 1 / scale per output, so te = min(T, out) consecutive outputs span at most
// ceil((te - 1) * in / (out - 1)) + taps samples; one more for the float32 rounding of u at an integer boundary.
static long long imresize_cap(int T, int in, int out, int taps) {
  const int te = T < out ? T : out;
  if (te <= 1) return (long long)taps + 1;
  return ((long long)(te - 1) * in + (out - 2)) / (out - 1) + taps + 1;
}

struct ImresizePlan { int cap_h, cap_w, mid_pitch, stage_floats; size_t lds; };

static bool imresize_plan(int T, int h, int w, int oh, int ow, int taps_h, int taps_w, ImresizePlan* p) {
  const long long ch = imresize_cap(T, h, oh, taps_h);
  const long long cw = (imresize_cap(T, w, ow, taps_w) + 3 + 3) / 4 * 4;     // + 3: the first column is rounded down to a multiple of 4
  const long long mp = cw | 1;
  long long stage = ch * cw;
  if (stage < (long long)T * T) stage = (long long)T * T;
  const long long floats = stage + (long long)T * mp + (long long)T * (taps_h + taps_w) + 2 * T;
  if (floats * 4 > (long long)kImrLdsMax) return false;
  p->cap_h = (int)ch; p->cap_w = (int)cw; p->mid_pitch = (int)mp; p->stage_floats = (int)stage; p->lds = (size_t)floats * 4;
  return true;
}

extern "C" int srganfd_imresize(const float* src, int32_t planes, int32_t h, int32_t w, int32_t oh, int32_t ow, const float* wt_h, const int32_t* first_h,
                                int32_t taps_h, const float* wt_w, const int32_t* first_w, int32_t taps_w, float* dst, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!src || !dst || !wt_h || !first_h || !wt_w || !first_w) return set_err(SRGANFD_EINVAL, "imresize: null pointer");
  if (planes <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || taps_h < 1 || taps_w < 1)
    return set_err(SRGANFD_EINVAL, "imresize: bad args (planes %d, %d x %d -> %d x %d, taps %d / %d: all must be positive)", planes, h, w, oh, ow,
                   taps_h, taps_w);
  if (planes > 65535) return set_err(SRGANFD_EINVAL, "imresize: %d planes, at most 65535 per call", planes);
  // the largest tile whose footprint, intermediate and weights fit: 16 at 1/4, 8 at 1/8, 32 at 1/2 and when enlarging
  ImresizePlan plan;
  int T = 32;
  while (T >= 1 && !imresize_plan(T, h, w, oh, ow, taps_h, taps_w, &plan)) T >>= 1;
  if (T < 1)
    return set_err(SRGANFD_EINVAL, "imresize: %d x %d -> %d x %d with %d / %d taps: one output's footprint does not fit %zu bytes of LDS", h, w,
                   oh, ow, taps_h, taps_w, kImrLdsMax);
  const int tiles_x = ceil_div(ow, T), tiles_y = ceil_div(oh, T);
  if ((long long)tiles_x * tiles_y * planes > 0x7fffffffLL || tiles_y > 65535)
    return set_err(SRGANFD_EINVAL, "imresize: %d planes of %d x %d tiles exceed the grid", planes, tiles_y, tiles_x);
  const bool rows_fast = (long long)w > (long long)ow;     // shrinking along the width
  static unsigned long long attr_done = 0;   // one bit per device: the attribute belongs to the device's code object
  if (!g_dry_run) {
    int dev = 0;
    SRGANFD_HIP_CHECK(hipGetDevice(&dev));
    if (!(attr_done >> (dev & 63) & 1ULL)) {
      SRGANFD_HIP_CHECK(hipFuncSetAttribute((const void*)imresize_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kImrLdsMax));
      SRGANFD_HIP_CHECK(hipFuncSetAttribute((const void*)imresize_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kImrLdsMax));
      attr_done |= 1ULL << (dev & 63);
    }
  }
  ImresizeArgs a;
  a.src = src; a.dst = dst; a.wt_h = wt_h; a.first_h = first_h; a.wt_w = wt_w; a.first_w = first_w;
  a.h = h; a.w = w; a.oh = oh; a.ow = ow; a.taps_h = taps_h; a.taps_w = taps_w;
  a.tile = T; a.tiles_x = tiles_x; a.tiles_y = tiles_y; a.cap_h = plan.cap_h; a.cap_w = plan.cap_w; a.mid_pitch = plan.mid_pitch; a.stage_floats = plan.stage_floats;
  a.vec = ((w & 3) == 0 && ((uintptr_t)src & 15) == 0) ? 1 : 0;
  if (rows_fast) SRGANFD_LAUNCH(imresize_kernel<true>, dim3(tiles_x * tiles_y * planes), dim3(kImrThreads), plan.lds, s, a);
  else SRGANFD_LAUNCH(imresize_kernel<false>, dim3(tiles_x, tiles_y, planes), dim3(kImrThreads), plan.lds, s, a);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

}  // namespace srganfd
