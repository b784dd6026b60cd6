// hsv_common.h — cv2.cvtColor's 8-bit RGB <-> HSV on one pixel, shared by camera_ops.hip (apply_hue_shift),
// style_morph_ops.hip (boost_saturation, vibrance) and multi_model_ops.hip (adjust_saturation).  Restated from
// OpenCV's sources (cv2 absent, parity unpinned);
// tests/camera_ref.py rgb_to_hsv8 / hsv8_to_rgb is the yardstick, byte for byte.  Include from translation units
// built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace nst {

// rint(num / den) half-to-even for positive integers: what rint of the double quotient gives (a quotient that is
// not a tie is at least 1 / (2 den) away from one)
__device__ __forceinline__ int hsv_div_rint(int num, int den) {
  int q = num / den;
  const int r2 = 2 * (num - q * den);
  if (r2 > den || (r2 == den && (q & 1))) ++q;
  return q;
}

__device__ __forceinline__ int hsv_sat_u8f(float v) { return (int)fminf(fmaxf(rintf(v), 0.f), 255.f); }

// 8-bit BGR2HSV (fixed point, sdiv / hdiv tables in 12 bits): h 0..180 saturated to u8, s wrapped to u8 as the cast
__device__ __forceinline__ void rgb_to_hsv8(int r, int g, int b, int* h8, int* s8, int* v8) {
  const int v = max(r, max(g, b)), vmin = min(r, min(g, b));
  const int diff = v - vmin;
  const int sdiv = v ? hsv_div_rint(255 << 12, v) : 0;
  const int hdiv = diff ? hsv_div_rint(122880, diff) : 0;  // (180 << 12) / (6 diff)
  const int s = (diff * sdiv + 2048) >> 12;
  int hn = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
  int hh = (hn * hdiv + 2048) >> 12;
  if (hh < 0) hh += 180;
  *h8 = min(max(hh, 0), 255);
  *s8 = s & 255;
  *v8 = v;
}

// 8-bit HSV2BGR: the float path, sat_u8(rint(x * 255.f)); h8, s8, v8 in 0..255
__device__ __forceinline__ void hsv8_to_rgb(int h8, int s8, int v, int* rgb) {
  const float vf = (float)v * (1.f / 255.f);
  float bo, go, ro;
  if (s8 == 0) {
    bo = go = ro = vf;
  } else {
    const float sf = (float)s8 * (1.f / 255.f);
    float h = (float)h8 * (6.f / 180.f);
    h = fmodf(h, 6.f);
    int sector = (int)floorf(h);
    h -= (float)sector;
    if ((unsigned)sector >= 6u) {
      sector = 0;
      h = 0.f;
    }
    float tab[4];
    tab[0] = vf;
    tab[1] = vf * (1.f - sf);
    tab[2] = vf * (1.f - sf * h);
    tab[3] = vf * (1.f - sf * (1.f - h));
    // sector_data {1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}: the (b, g, r) picks
    const int pb = sector == 0 || sector == 1 ? 1 : (sector == 2 ? 3 : (sector == 5 ? 2 : 0));
    const int pg = sector == 0 ? 3 : (sector == 1 || sector == 2 ? 0 : (sector == 3 ? 2 : 1));
    const int pr = sector == 0 || sector == 5 ? 0 : (sector == 1 ? 2 : (sector == 4 ? 3 : 1));
    bo = tab[pb];
    go = tab[pg];
    ro = tab[pr];
  }
  rgb[0] = hsv_sat_u8f(ro * 255.f);
  rgb[1] = hsv_sat_u8f(go * 255.f);
  rgb[2] = hsv_sat_u8f(bo * 255.f);
}

}  // namespace nst
