// blur_kernels.hip -- the per-image filter kernels of Real-ESRGAN's degradation (Real_ESRGAN/dataset.py:64-133: random_mixed_kernels,
// imgproc.py:495-576, and generate_sinc_kernel, :579-606), synthesised on the device from their drawn parameters: one launch writes a bank
// of n kernels, kernel i being ksize[i] x ksize[i], centred in its kmax x kmax array with exact zeros around it.  The reference evaluates
// in numpy float64 and converts with torch.FloatTensor; here every element, the sum and the division are fp64 as well and the store is the
// one rounding to fp32.
// One 256-thread workgroup per kernel; a thread owns the slots tid, tid + 256, tid + 512 of the kmax x kmax array (at most 625), keeps
// their values in registers, and the sum is reduced in a fixed order: a thread's own slots in slot order, the 64 lanes by shuffle, then the
// four waves' partials through LDS in wave order -- identical bits on every run.
#include "common.hpp"

namespace srganfd {

static constexpr int kBankMaxK = 25, kBankThreads = 256, kBankWaves = kBankThreads / 64;
static constexpr int kBankSlots = (kBankMaxK * kBankMaxK + kBankThreads - 1) / kBankThreads;   // 3
static constexpr double kBankPi = 3.141592653589793238462643383279502884;

enum { kBankDelta = 0, kBankGaussian = 1, kBankGeneralized = 2, kBankPlateau = 3, kBankSinc = 4 };

// grid (n)
__global__ __launch_bounds__(kBankThreads) void blur_kernel_bank_kernel(const int* __restrict__ kind, const int* __restrict__ ksize,
                                                                        const double* __restrict__ params, int kmax, float* __restrict__ out) {
  __shared__ double red[kBankWaves];
  const int n = blockIdx.x;
  // the host refuses kinds and sizes outside their ranges where it can see them; here they are clamped into them
  const int kd = min(max(kind[n], 0), 4);
  const int k = min(max(ksize[n], 3), kmax) | 1;               // kmax is odd, so the | 1 of an even size stays <= kmax
  const double* p = params + (size_t)n * 5;
  const double sx = p[0], sy = p[1], theta = p[2], beta = p[3], omega = p[4];
  float* dst = out + (size_t)n * kmax * kmax;
  const int cells = kmax * kmax;
  if (kd == kBankDelta) {
    for (int i = threadIdx.x; i < cells; i += kBankThreads) dst[i] = i == (kmax / 2) * kmax + kmax / 2 ? 1.0f : 0.0f;
    return;
  }
  // Sigma = U diag(sx^2, sy^2) U^T, U the rotation by theta: [[a, b], [b, d]]; q = (x, y) Sigma^-1 (x, y)^T = (d x^2 - 2 b x y + a y^2) / det
  const double c = cos(theta), s = sin(theta), vx = sx * sx, vy = sy * sy;
  const double a = c * c * vx + s * s * vy, b = c * s * (vx - vy), d = s * s * vx + c * c * vy;
  const double det = a * d - b * b;
  const int off = (kmax - k) / 2, half = k / 2;
  double v[kBankSlots];
  double part = 0.0;
#pragma unroll
  for (int j = 0; j < kBankSlots; ++j) {
    const int i = threadIdx.x + j * kBankThreads;
    const int row = i / kmax - off, col = i % kmax - off;
    double val = 0.0;
    if (i < cells && row >= 0 && row < k && col >= 0 && col < k) {
      const double x = (double)(col - half), y = (double)(row - half);         // ax = arange(-k // 2 + 1, k // 2 + 1); x along columns
      if (kd == kBankSinc) {
        const double r = sqrt(x * x + y * y);
        val = (row == half && col == half) ? omega * omega / (4.0 * kBankPi) : omega * j1(omega * r) / (2.0 * kBankPi * r);
      } else {
        const double q = (d * x * x - 2.0 * b * x * y + a * y * y) / det;
        if (kd == kBankGaussian) val = exp(-0.5 * q);
        else if (kd == kBankGeneralized) val = exp(-0.5 * pow(q, beta));
        else val = 1.0 / (pow(q, beta) + 1.0);
      }
    }
    v[j] = val;
    part += val;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o, 64);
  if (lane == 0) red[wave] = part;
  __syncthreads();
  double sum = 0.0;
#pragma unroll
  for (int w = 0; w < kBankWaves; ++w) sum += red[w];
#pragma unroll
  for (int j = 0; j < kBankSlots; ++j) {
    const int i = threadIdx.x + j * kBankThreads;
    if (i < cells) dst[i] = (float)(v[j] / sum);                  // outside the k x k window v is 0.0: exact zeros around the kernel
  }
}

extern "C" int srganfd_blur_kernel_bank(const int32_t* kind, const int32_t* ksize, const double* params, const int32_t* kind_host,
                                        const int32_t* ksize_host, int32_t n, int32_t kmax, float* out, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!kind || !ksize || !params || !out) return set_err(SRGANFD_EINVAL, "blur_kernel_bank: null pointer");
  if (n <= 0) return set_err(SRGANFD_EINVAL, "blur_kernel_bank: n = %d kernels (must be positive)", n);
  if (kmax < 3 || kmax > kBankMaxK || kmax % 2 == 0) return set_err(SRGANFD_EINVAL, "blur_kernel_bank: kmax %d is not an odd size from 3 to %d", kmax, kBankMaxK);
  if (!kind_host != !ksize_host) return set_err(SRGANFD_EINVAL, "blur_kernel_bank: kind_host and ksize_host are given together or not at all");
  if (kind_host) {
    for (int i = 0; i < n; ++i) {
      const int kd = kind_host[i], k = ksize_host[i];
      if (kd < 0 || kd > 4) return set_err(SRGANFD_EINVAL, "blur_kernel_bank: kind[%d] = %d is not one of 0 (delta) .. 4 (sinc)", i, kd);
      if (kd != kBankDelta && (k < 3 || k > kmax || k % 2 == 0))
        return set_err(SRGANFD_EINVAL, "blur_kernel_bank: ksize[%d] = %d is not an odd size from 3 to kmax = %d", i, k, kmax);
    }
  }
  SRGANFD_LAUNCH(blur_kernel_bank_kernel, dim3(n), dim3(kBankThreads), 0, s, kind, ksize, params, kmax, out);
  SRGANFD_HIP_CHECK(hipGetLastError());
  return SRGANFD_OK;
}

}  // namespace srganfd
