// blur_internal.h — the separable fp32 Gaussian blur of float planes (blur_ops.hip) that the Farneback pre-blur,
// the motion-adaptive alpha and the region feather share, and the tap generator.
#pragma once

#include <hip/hip_runtime.h>

namespace nst {

constexpr int BLUR_MAX_TAPS = 511;  // the tap table travels as a kernel argument (2 KiB)

// cv2.getGaussianKernel(n, sigma, CV_32F) into t[n] (n <= BLUR_MAX_TAPS): sigma <= 0 takes the fixed 3-tap table
// at n = 3 and OpenCV's default sigma otherwise
void gaussian_taps_f32(int n, double sigma, float* t);
// k planes [h][w] blurred in place through tmp (k planes): rows into tmp, then columns back, BORDER_REFLECT_101,
// each sum acc = acc + taps[j] * v from 0.f in ascending tap order; odd n <= BLUR_MAX_TAPS
hipError_t launch_sep_blur_f32(float* planes, int k, int h, int w, const float* taps, int n, float* tmp,
                               hipStream_t st);

}  // namespace nst
