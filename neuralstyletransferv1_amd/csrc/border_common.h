// border_common.h — OpenCV's two mirrored border rules as device helpers, each valid for any integer position
// (a position further out than the frame is wide reflects more than once).
#pragma once

#include <hip/hip_runtime.h>

namespace nst {

// BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba; torch's F.pad(mode='reflect')): the edge sample is not repeated
__device__ __forceinline__ int border_reflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
  return p;
}

// BORDER_REFLECT (fedcba|abcdefgh|hgfedcba): the edge sample is repeated
__device__ __forceinline__ int border_reflect(int p, int n) {
  const int n2 = 2 * n;
  int r = p % n2;
  if (r < 0) r += n2;
  return r < n ? r : n2 - 1 - r;
}

}  // namespace nst
