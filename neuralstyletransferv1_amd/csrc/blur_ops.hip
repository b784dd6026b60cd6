// blur_ops.hip — one separable fp32 Gaussian blur of float planes (cv2.GaussianBlur on a float image;
// region_blend.py's F.pad(reflect) + conv2d with the outer product of the 1-D taps): a row pass into a scratch
// plane, then a column pass back, BORDER_REFLECT_101, the taps in a kernel argument.  Built with
// -ffp-contract=off: every product and sum rounds on its own, in ascending tap order.
#include <math.h>

#include <cmath>

#include "blur_internal.h"
#include "border_common.h"

namespace nst {

struct BlurTaps {
  int n;
  float t[BLUR_MAX_TAPS];
};

// row tiles of 256 pixels + halo staged in LDS
__global__ __launch_bounds__(256) void blur_rows_kernel(const float* __restrict__ in, int h, int w, BlurTaps tp,
                                                        float* __restrict__ out) {
  extern __shared__ float row[];  // 256 + n - 1 entries
  const int pad = tp.n / 2;
  const size_t plane = (size_t)blockIdx.z * h * w;
  const int y = blockIdx.y, x0 = blockIdx.x * 256;
  const float* src = in + plane + (size_t)y * w;
  for (int j = threadIdx.x; j < 256 + tp.n - 1; j += 256) {
    const int xs = x0 + j - pad;
    row[j] = (xs < w + pad) ? src[border_reflect101(xs, w)] : 0.f;
  }
  __syncthreads();
  const int x = x0 + threadIdx.x;
  if (x >= w) return;
  float acc = 0.f;
  for (int j = 0; j < tp.n; ++j) acc = acc + tp.t[j] * row[threadIdx.x + j];
  out[plane + (size_t)y * w + x] = acc;
}

__global__ __launch_bounds__(256) void blur_cols_kernel(const float* __restrict__ in, int h, int w, BlurTaps tp,
                                                        float* __restrict__ out) {
  const int pad = tp.n / 2;
  const size_t plane = (size_t)blockIdx.z * h * w;
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= w) return;
  const float* col = in + plane + x;
  float acc = 0.f;
  if (y >= pad && y + pad < h) {  // an interior row (y is the block's): the same samples without the border rule
    const float* p = col + (size_t)(y - pad) * w;
    for (int j = 0; j < tp.n; ++j) acc = acc + tp.t[j] * p[(size_t)j * w];
  } else {
    for (int j = 0; j < tp.n; ++j) acc = acc + tp.t[j] * col[(size_t)border_reflect101(y + j - pad, h) * w];
  }
  out[plane + (size_t)y * w + x] = acc;
}

hipError_t launch_sep_blur_f32(float* planes, int k, int h, int w, const float* taps, int n, float* tmp,
                               hipStream_t st) {
  if (n < 1 || n > BLUR_MAX_TAPS || (n & 1) == 0) return hipErrorInvalidValue;
  BlurTaps tp;
  tp.n = n;
  for (int i = 0; i < BLUR_MAX_TAPS; ++i) tp.t[i] = i < n ? taps[i] : 0.f;
  const dim3 grid((unsigned)((w + 255) / 256), (unsigned)h, (unsigned)k);
  hipLaunchKernelGGL(blur_rows_kernel, grid, dim3(256), (256 + n - 1) * sizeof(float), st, planes, h, w, tp, tmp);
  hipLaunchKernelGGL(blur_cols_kernel, grid, dim3(256), 0, st, tmp, h, w, tp, planes);
  return hipGetLastError();
}

void gaussian_taps_f32(int n, double sigma, float* t) {
  if (sigma <= 0 && n == 3) {
    t[0] = 0.25f; t[1] = 0.5f; t[2] = 0.25f;
    return;
  }
  if (sigma <= 0) sigma = ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
  const double s2 = -0.5 / (sigma * sigma);
  double sum = 0;
  double v[BLUR_MAX_TAPS];
  for (int i = 0; i < n; ++i) {
    const double x = i - (n - 1) * 0.5;
    v[i] = std::exp(s2 * x * x);
    sum += v[i];
  }
  for (int i = 0; i < n; ++i) t[i] = (float)(v[i] / sum);
}

}  // namespace nst
