// camera_ops.hip — the camera stage of the morph slideshow (scripts/morph_v2.py:624-999, create_morph_video with
// --pan_zoom): what the reference does to every morph frame between optical_flow_morph and the video writer, on the
// GPU and batched over frames (include/nst_hip.h "Camera stage"):
//   (a) zoom pulse     cv2.resize(frame, (nw, nh), INTER_LINEAR) + centre crop back, 8-bit fixed point (11-bit taps);
//   (b) getRectSubPix  u8 -> u8, 16-bit fixed-point weights, replicated right column / bottom row;
//   (c) zoom phase     cv2.resize(crop, target, INTER_LANCZOS4): 8 x 8 taps from host-built tables, int64 vertical sum;
//   (d) hue rotation   8-bit BGR2HSV (fixed point), fp32 remainder, HSV2BGR (float path);
//   (e) temporal_smooth_frames with NumPy >= 2 promotion (double products, fp32 accumulator, double quotient);
//   (f) the fused launch pair the CLI uses: zoom-phase patches go through scratch, pan-phase frames are one gather
//       pass over the morph frame (pulse taps recomputed under the sub-pixel taps) and one store, the run and its store
//       from the compositor core (u8run_common.h).
// cv2 is not installed here: all of it is restated from OpenCV's sources and the script, parity unpinned; the
// yardstick is tests/camera_ref.py, byte for byte.  Built with -ffp-contract=off: every product and sum rounds alone.
#include <hip/hip_runtime.h>
#include <math.h>

#include <cstdint>
#include <string>

#include "hsv_common.h"
#include "nst_hip.h"
#include "nst_internal.h"
#include "u8run_common.h"

namespace nst {
namespace {

struct CamFrame {
  double scx, scy;                   // pulse: W / nw, H / nh
  size_t scr_off;                    // zoom phase: byte offset of this frame's patch in the scratch
  int pulse, ox, oy;                 // pulse on; (nw - W) / 2, (nh - H) / 2
  int zoom, pw, ph;                  // phase; patch size (lanczos stage: the crop's size)
  int ipx, ipy;                      // floor of the patch's corner
  int a11, a12, a21, a22, b1, b2;    // getRectSubPix weights, 16 fraction bits
  int hue_on;
  float hue_half;
  int table;
};
struct CamBatch {
  CamFrame f[NST_CAMERA_MAX_FRAMES];
};
struct LancTab {
  const int32_t* xofs;   // [slots, tw]     floor(fx) of every output column
  const int16_t* xcoef;  // [slots, tw, 8]
  const int32_t* yofs;   // [slots, th]
  const int16_t* ycoef;  // [slots, th, 8]
};

struct LinTap {
  int i0, i1, c0, c1;
};

// cv2.resize INTER_LINEAR, 8-bit: the source column of resized column d, taps in 11 bits
__device__ __forceinline__ LinTap lin_tap_x(int d, double scale, int n) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= n - 1) { s = n - 1; f = 0.f; }
  LinTap t;
  t.i0 = s;
  t.i1 = min(s + 1, n - 1);
  t.c0 = (int)(short)rintf((1.f - f) * 2048.f);
  t.c1 = (int)(short)rintf(f * 2048.f);
  return t;
}

// rows: the fraction is kept, the two rows are clipped one by one
__device__ __forceinline__ LinTap lin_tap_y(int d, double scale, int n) {
  float f = (float)((d + 0.5) * scale - 0.5);
  const int s = (int)floorf(f);
  f -= (float)s;
  LinTap t;
  t.i0 = min(max(s, 0), n - 1);
  t.i1 = min(max(s + 1, 0), n - 1);
  t.c0 = (int)(short)rintf((1.f - f) * 2048.f);
  t.c1 = (int)(short)rintf(f * 2048.f);
  return t;
}

__device__ __forceinline__ void pulse_px(const uint8_t* __restrict__ src, int w, const LinTap& tx, const LinTap& ty,
                                         int* rgb) {
  const uint8_t* r0 = src + (size_t)ty.i0 * w * 3;
  const uint8_t* r1 = src + (size_t)ty.i1 * w * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int s0 = (int)r0[tx.i0 * 3 + c] * tx.c0 + (int)r0[tx.i1 * 3 + c] * tx.c1;
    const int s1 = (int)r1[tx.i0 * 3 + c] * tx.c0 + (int)r1[tx.i1 * 3 + c] * tx.c1;
    rgb[c] = ((((ty.c0 * (s0 >> 4)) >> 16) + ((ty.c1 * (s1 >> 4)) >> 16) + 2) >> 2) & 255;
  }
}

__device__ __forceinline__ void load_px(const uint8_t* __restrict__ src, int w, int x, int y, int* rgb) {
  const uint8_t* p = src + ((size_t)y * w + x) * 3;
  rgb[0] = p[0];
  rgb[1] = p[1];
  rgb[2] = p[2];
}

// pixel (j, i) of getRectSubPix's patch, taken from the (pulsed) frame: 0 <= ip and ip + patch <= size hold, so the
// only border is the replicated column w - 1 / row h - 1
__device__ __forceinline__ void subpix_px(const uint8_t* __restrict__ src, int h, int w, const CamFrame& f, int j, int i,
                                          int* rgb) {
  const int x0 = f.ipx + j, y0 = f.ipy + i;
  const bool xin = x0 + 1 <= w - 1;
  const int y1 = y0 + 1 <= h - 1 ? y0 + 1 : y0;
  int p00[3], p01[3] = {0, 0, 0}, p10[3], p11[3] = {0, 0, 0};
  if (f.pulse) {
    const LinTap tx0 = lin_tap_x(x0 + f.ox, f.scx, w);
    const LinTap ty0 = lin_tap_y(y0 + f.oy, f.scy, h), ty1 = lin_tap_y(y1 + f.oy, f.scy, h);
    pulse_px(src, w, tx0, ty0, p00);
    pulse_px(src, w, tx0, ty1, p10);
    if (xin) {
      const LinTap tx1 = lin_tap_x(x0 + 1 + f.ox, f.scx, w);
      pulse_px(src, w, tx1, ty0, p01);
      pulse_px(src, w, tx1, ty1, p11);
    }
  } else {
    load_px(src, w, x0, y0, p00);
    load_px(src, w, x0, y1, p10);
    if (xin) {
      load_px(src, w, x0 + 1, y0, p01);
      load_px(src, w, x0 + 1, y1, p11);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    rgb[c] = (xin ? (f.a11 * p00[c] + f.a12 * p01[c] + f.a21 * p10[c] + f.a22 * p11[c] + 32768) >> 16
                  : (f.b1 * p00[c] + f.b2 * p10[c] + 32768) >> 16) & 255;
}

// cv2.resize INTER_LANCZOS4 of the cw x ch image at `img` (row pitch `pitch` pixels): output pixel (x, y).  Every tap
// index is clamped here, so no table content can index outside the image.
__device__ __forceinline__ void lanczos_px(const uint8_t* __restrict__ img, int pitch, int cw, int ch, const LancTab& tab,
                                           int slot, int tw, int th, int x, int y, int* rgb) {
  const int sx = tab.xofs[(size_t)slot * tw + x], sy = tab.yofs[(size_t)slot * th + y];
  const int16_t* cx = tab.xcoef + ((size_t)slot * tw + x) * 8;
  const int16_t* cy = tab.ycoef + ((size_t)slot * th + y) * 8;
  int col[8], kx[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    col[k] = min(max(sx - 3 + k, 0), cw - 1) * 3;
    kx[k] = cx[k];
  }
  long long v[3] = {0, 0, 0};
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint8_t* row = img + (size_t)min(max(sy - 3 + r, 0), ch - 1) * pitch * 3;
    int hs[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      hs[0] += (int)row[col[k]] * kx[k];
      hs[1] += (int)row[col[k] + 1] * kx[k];
      hs[2] += (int)row[col[k] + 2] * kx[k];
    }
    const long long ky = cy[r];
    v[0] += hs[0] * ky;
    v[1] += hs[1] * ky;
    v[2] += hs[2] * ky;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long long q = (v[c] + (1ll << 21)) >> 22;
    rgb[c] = (int)(q < 0 ? 0 : (q > 255 ? 255 : q));
  }
}

// apply_hue_shift on one RGB pixel: cv2's 8-bit BGR2HSV, the fp32 remainder numpy takes, HSV2BGR's float path
// (both conversions in hsv_common.h)
__device__ __forceinline__ void hue_px(int* rgb, float half) {
  int hh, s8, v;
  rgb_to_hsv8(rgb[0], rgb[1], rgb[2], &hh, &s8, &v);
  // np.remainder(float32(h) + half, 180): fmod, then the divisor's sign
  float m = fmodf((float)hh + half, 180.f);
  if (m != 0.f) {
    if (m < 0.f) m += 180.f;
  } else {
    m = 0.f;
  }
  hsv8_to_rgb((int)m, s8, v, rgb);  // (int)m: 0 .. 180
}

// ---- the single stages (a) - (d), one thread per output pixel: what the tests and camera.py's wrappers call ----
enum { STAGE_PULSE = 0, STAGE_SUBPIX = 1, STAGE_LANCZOS = 2, STAGE_HUE = 3 };

template <int STAGE>
__global__ __launch_bounds__(256) void camera_stage_kernel(const uint8_t* __restrict__ in, int h, int w, CamBatch cb,
                                                           int oh, int ow, LancTab tab, uint8_t* __restrict__ out) {
  const size_t opix = (size_t)oh * ow;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= opix) return;
  const CamFrame& f = cb.f[blockIdx.z];
  const uint8_t* src = in + (size_t)blockIdx.z * h * w * 3;
  const int x = (int)(i % ow), y = (int)(i / ow);
  int rgb[3];
  if (STAGE == STAGE_PULSE) {
    pulse_px(src, w, lin_tap_x(x + f.ox, f.scx, w), lin_tap_y(y + f.oy, f.scy, h), rgb);
  } else if (STAGE == STAGE_SUBPIX) {
    subpix_px(src, h, w, f, x, y, rgb);
  } else if (STAGE == STAGE_LANCZOS) {
    lanczos_px(src, w, f.pw, f.ph, tab, f.table, ow, oh, x, y, rgb);
  } else {
    load_px(src, w, x, y, rgb);
    if (f.hue_on) hue_px(rgb, f.hue_half);
  }
  uint8_t* o = out + ((size_t)blockIdx.z * opix + i) * 3;
  o[0] = (uint8_t)rgb[0];
  o[1] = (uint8_t)rgb[1];
  o[2] = (uint8_t)rgb[2];
}

// ---- (f) ----
// zoom-phase frames: the (pulsed) frame's centred patch into the scratch, rows packed (pitch = patch width)
__global__ __launch_bounds__(256) void camera_crop_kernel(const uint8_t* __restrict__ in, int h, int w, CamBatch cb,
                                                          uint8_t* __restrict__ scratch) {
  const CamFrame& f = cb.f[blockIdx.z];
  if (!f.zoom) return;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)f.pw * f.ph) return;
  int rgb[3];
  subpix_px(in + (size_t)blockIdx.z * h * w * 3, h, w, f, (int)(i % f.pw), (int)(i / f.pw), rgb);
  uint8_t* o = scratch + f.scr_off + i * 3;
  o[0] = (uint8_t)rgb[0];
  o[1] = (uint8_t)rgb[1];
  o[2] = (uint8_t)rgb[2];
}

// every frame's output: one run of U8_RUN consecutive pixels per thread (u8run_common.h); zoom phase = Lanczos of its
// patch, pan phase = the sub-pixel gather from the morph frame; then the hue rotation and store_run.
template <bool VEC>
__global__ __launch_bounds__(256) void camera_out_kernel(const uint8_t* __restrict__ in, int h, int w, CamBatch cb, int th,
                                                         int tw, LancTab tab, const uint8_t* __restrict__ scratch,
                                                         uint8_t* __restrict__ out) {
  const size_t opix = (size_t)th * tw;
  const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * U8_RUN;
  if (i0 >= opix) return;
  const CamFrame& f = cb.f[blockIdx.z];
  const uint8_t* src = in + (size_t)blockIdx.z * h * w * 3;
  RunBytes rb;
#pragma unroll
  for (int j = 0; j < U8_RUN; ++j) {
    const size_t i = min(i0 + j, opix - 1);
    const int x = (int)(i % tw), y = (int)(i / tw);
    int rgb[3];
    if (f.zoom)
      lanczos_px(scratch + f.scr_off, f.pw, f.pw, f.ph, tab, f.table, tw, th, x, y, rgb);
    else
      subpix_px(src, h, w, f, x, y, rgb);
    if (f.hue_on) hue_px(rgb, f.hue_half);
    rb.b[j * 3] = (uint32_t)rgb[0];
    rb.b[j * 3 + 1] = (uint32_t)rgb[1];
    rb.b[j * 3 + 2] = (uint32_t)rgb[2];
  }
  store_run<VEC>(out + ((size_t)blockIdx.z * opix + i0) * 3, rb, run_count<VEC>(i0, opix));
}

// ---- (e) ----
struct SmoothW {
  int k, half;
  double w[NST_CAMERA_MAX_SMOOTH];
};

__device__ __forceinline__ uint32_t smooth_byte(const uint8_t* __restrict__ win, size_t fbytes, size_t e, int g, int first,
                                                int seq_len, const SmoothW& sw) {
  float acc = 0.f;
  double total = 0.0;
  for (int j = 0; j < sw.k; ++j) {
    const int idx = g + j - sw.half;
    if (idx >= 0 && idx < seq_len) {
      acc = (float)((double)acc + (double)(float)win[(size_t)(idx - first) * fbytes + e] * sw.w[j]);
      total += sw.w[j];
    }
  }
  return (uint32_t)(int)((double)acc / total) & 255u;
}

template <bool VEC>
__global__ __launch_bounds__(256) void camera_smooth_kernel(const uint8_t* __restrict__ win, size_t fbytes, int first,
                                                            int seq_len, int out_first, SmoothW sw,
                                                            uint8_t* __restrict__ out) {
  const size_t e0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e0 >= fbytes) return;
  const int g = out_first + (int)blockIdx.z;
  uint8_t* o = out + (size_t)blockIdx.z * fbytes + e0;
  if (VEC) {
    uint32_t v = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) v |= smooth_byte(win, fbytes, e0 + q, g, first, seq_len, sw) << (8 * q);
    *(uint32_t*)o = v;
  } else {
    for (int q = 0; q < 4 && e0 + q < fbytes; ++q) o[q] = (uint8_t)smooth_byte(win, fbytes, e0 + q, g, first, seq_len, sw);
  }
}

// ---- host side: argument checks and the device descriptors ----
bool bad_dims(const char* who, int n, int h, int w, int* rc) {
  if (n < 1 || n > NST_CAMERA_MAX_FRAMES) {
    set_error(std::string(who) + ": 1 <= n <= " + std::to_string(NST_CAMERA_MAX_FRAMES) + " frames per call");
    *rc = NST_E_INVALID;
    return true;
  }
  if (bad_frame_shape(who, h, w)) {
    *rc = NST_E_SHAPE;
    return true;
  }
  return false;
}

bool set_pulse(CamFrame& f, int h, int w, int nw, int nh) {
  if (nw < w || nh < h || nw > (1 << 20) || nh > (1 << 20)) return false;
  f.pulse = (nw != w || nh != h) ? 1 : 0;  // (w, h) is the identity
  f.ox = (nw - w) / 2;
  f.oy = (nh - h) / 2;
  f.scx = (double)w / (double)nw;
  f.scy = (double)h / (double)nh;
  return true;
}

// getRectSubPix's corner and weights; false unless 0 <= ip and ip + patch <= size
bool set_subpix(CamFrame& f, int h, int w, int pw, int ph, float cx, float cy) {
  if (pw < 1 || ph < 1 || pw > w || ph > h || !(cx >= 0.f) || !(cy >= 0.f) || !(cx <= 65536.f) || !(cy <= 65536.f))
    return false;
  cx -= (float)(pw - 1) * 0.5f;
  cy -= (float)(ph - 1) * 0.5f;
  if (!(cx >= 0.f) || !(cy >= 0.f)) return false;
  const int ix = (int)floorf(cx), iy = (int)floorf(cy);
  if (ix + pw > w || iy + ph > h) return false;
  const float a = cx - (float)ix, b = cy - (float)iy;
  f.pw = pw;
  f.ph = ph;
  f.ipx = ix;
  f.ipy = iy;
  f.a11 = (int)rintf((1.f - a) * (1.f - b) * 65536.f);
  f.a12 = (int)rintf(a * (1.f - b) * 65536.f);
  f.a21 = (int)rintf((1.f - a) * b * 65536.f);
  f.a22 = (int)rintf(a * b * 65536.f);
  f.b1 = (int)rintf((1.f - b) * 65536.f);
  f.b2 = (int)rintf(b * 65536.f);
  return true;
}

bool set_hue(CamFrame& f, int on, float half) {
  if (!(fabsf(half) <= 1.0e6f)) return false;
  f.hue_on = on ? 1 : 0;
  f.hue_half = half;
  return true;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

dim3 px_grid(size_t pixels, int per_thread, int n) {
  const size_t threads = (pixels + per_thread - 1) / per_thread;
  return dim3((unsigned)((threads + 255) / 256), 1, (unsigned)n);
}

#define CAM_LAUNCHED(what)                                                              \
  do {                                                                                  \
    hipError_t _e = hipGetLastError();                                                  \
    if (_e != hipSuccess) {                                                             \
      set_error(std::string(what) + " launch: " + hipGetErrorString(_e));               \
      return NST_E_HIP;                                                                 \
    }                                                                                   \
  } while (0)

}  // namespace
}  // namespace nst

using namespace nst;

extern "C" {

int nst_camera_pulse_u8(const uint8_t* in, int n, int h, int w, const int* nw, const int* nh, uint8_t* out,
                        void* stream) {
  int rc;
  if (!in || !out || in == out || !nw || !nh) { set_error("nst_camera_pulse_u8: invalid arguments (out != in)"); return NST_E_INVALID; }
  if (bad_dims("nst_camera_pulse_u8", n, h, w, &rc)) return rc;
  CamBatch cb = {};
  for (int i = 0; i < n; ++i)
    if (!set_pulse(cb.f[i], h, w, nw[i], nh[i])) {
      set_error("nst_camera_pulse_u8: frame " + std::to_string(i) + ": the resized size must be at least the frame's");
      return NST_E_INVALID;
    }
  for (int i = 0; i < n; ++i) cb.f[i].pulse = 1;
  hipLaunchKernelGGL(camera_stage_kernel<STAGE_PULSE>, px_grid((size_t)h * w, 1, n), dim3(256), 0, (hipStream_t)stream, in,
                     h, w, cb, h, w, LancTab{}, out);
  CAM_LAUNCHED("camera_pulse");
  return NST_OK;
}

int nst_camera_rect_subpix_u8(const uint8_t* in, int n, int h, int w, int pw, int ph, const float* cx, const float* cy,
                              uint8_t* out, void* stream) {
  int rc;
  if (!in || !out || in == out || !cx || !cy) { set_error("nst_camera_rect_subpix_u8: invalid arguments (out != in)"); return NST_E_INVALID; }
  if (bad_dims("nst_camera_rect_subpix_u8", n, h, w, &rc)) return rc;
  CamBatch cb = {};
  for (int i = 0; i < n; ++i)
    if (!set_subpix(cb.f[i], h, w, pw, ph, cx[i], cy[i])) {
      set_error("nst_camera_rect_subpix_u8: frame " + std::to_string(i) + ": the patch must lie inside the frame (its " +
                "corner's floor >= 0, floor + patch <= size); the left and top borders are not built");
      return NST_E_INVALID;
    }
  hipLaunchKernelGGL(camera_stage_kernel<STAGE_SUBPIX>, px_grid((size_t)ph * pw, 1, n), dim3(256), 0, (hipStream_t)stream,
                     in, h, w, cb, ph, pw, LancTab{}, out);
  CAM_LAUNCHED("camera_rect_subpix");
  return NST_OK;
}

int nst_camera_lanczos_u8(const uint8_t* in, int n, int h, int w, const int* cw, const int* ch, int tw, int th,
                          const int32_t* xofs, const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef,
                          uint8_t* out, void* stream) {
  int rc;
  if (!in || !out || in == out || !cw || !ch || !xofs || !xcoef || !yofs || !ycoef) {
    set_error("nst_camera_lanczos_u8: invalid arguments (out != in)");
    return NST_E_INVALID;
  }
  if (bad_dims("nst_camera_lanczos_u8", n, h, w, &rc)) return rc;
  if (tw < 1 || th < 1 || tw > 32768 || th > 32768) {
    set_error("nst_camera_lanczos_u8: target " + std::to_string(tw) + "x" + std::to_string(th) + " outside 1..32768");
    return NST_E_SHAPE;
  }
  CamBatch cb = {};
  for (int i = 0; i < n; ++i) {
    if (cw[i] < 1 || ch[i] < 1 || cw[i] > w || ch[i] > h) {
      set_error("nst_camera_lanczos_u8: frame " + std::to_string(i) + ": the crop must lie inside the frame");
      return NST_E_INVALID;
    }
    cb.f[i].pw = cw[i];
    cb.f[i].ph = ch[i];
    cb.f[i].table = i;
  }
  hipLaunchKernelGGL(camera_stage_kernel<STAGE_LANCZOS>, px_grid((size_t)th * tw, 1, n), dim3(256), 0, (hipStream_t)stream,
                     in, h, w, cb, th, tw, LancTab{xofs, xcoef, yofs, ycoef}, out);
  CAM_LAUNCHED("camera_lanczos");
  return NST_OK;
}

int nst_camera_hue_u8(const uint8_t* in, int n, int h, int w, const int* hue_on, const float* hue_half, uint8_t* out,
                      void* stream) {
  int rc;
  if (!in || !out || !hue_on || !hue_half) { set_error("nst_camera_hue_u8: invalid arguments"); return NST_E_INVALID; }
  if (bad_dims("nst_camera_hue_u8", n, h, w, &rc)) return rc;
  CamBatch cb = {};
  for (int i = 0; i < n; ++i)
    if (!set_hue(cb.f[i], hue_on[i], hue_half[i])) {
      set_error("nst_camera_hue_u8: frame " + std::to_string(i) + ": the half shift must be finite, at most 1e6");
      return NST_E_INVALID;
    }
  hipLaunchKernelGGL(camera_stage_kernel<STAGE_HUE>, px_grid((size_t)h * w, 1, n), dim3(256), 0, (hipStream_t)stream, in, h,
                     w, cb, h, w, LancTab{}, out);
  CAM_LAUNCHED("camera_hue");
  return NST_OK;
}

int nst_camera_smooth_u8(const uint8_t* window, int win_n, int h, int w, int first, int seq_len, int out_first,
                         int out_count, int kernel_size, const double* weights, uint8_t* out, void* stream) {
  if (!window || !out || !weights || win_n < 1 || first < 0 || seq_len < 1 || out_first < 0 || out_count < 1 ||
      out_count > 65535 || (long long)first + win_n > seq_len || (long long)out_first + out_count > seq_len) {
    set_error("nst_camera_smooth_u8: invalid arguments (window and outputs inside the sequence)");
    return NST_E_INVALID;
  }
  if (kernel_size < 1 || kernel_size > NST_CAMERA_MAX_SMOOTH) {
    set_error("nst_camera_smooth_u8: kernel_size " + std::to_string(kernel_size) + " outside 1.." +
              std::to_string(NST_CAMERA_MAX_SMOOTH));
    return NST_E_INVALID;
  }
  if (bad_frame_shape("nst_camera_smooth_u8", h, w)) return NST_E_SHAPE;
  const bool plain = seq_len <= kernel_size;  // the call site's condition: such a sequence is returned unchanged
  const int half = kernel_size / 2;
  const int lo = plain ? out_first : (out_first - half < 0 ? 0 : out_first - half);
  const long long hi_tap = (long long)out_first + out_count - 1 + (plain ? 0 : kernel_size - 1 - half);
  const int hi = (int)(hi_tap > seq_len - 1 ? seq_len - 1 : hi_tap);
  if (lo < first || hi >= first + win_n) {
    set_error("nst_camera_smooth_u8: the outputs need frames " + std::to_string(lo) + ".." + std::to_string(hi) +
              ", the window holds " + std::to_string(first) + ".." + std::to_string(first + win_n - 1));
    return NST_E_INVALID;
  }
  const size_t fbytes = (size_t)h * w * 3;
  if (out == window || (out > window && out < window + (size_t)win_n * fbytes) ||
      (window > out && window < out + (size_t)out_count * fbytes)) {
    set_error("nst_camera_smooth_u8: out overlaps the window");
    return NST_E_INVALID;
  }
  if (plain) {
    hipError_t e = hipMemcpyAsync(out, window + (size_t)(out_first - first) * fbytes, (size_t)out_count * fbytes,
                                  hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) { set_error(std::string("nst_camera_smooth_u8 copy: ") + hipGetErrorString(e)); return NST_E_HIP; }
    return NST_OK;
  }
  SmoothW sw = {};
  sw.k = kernel_size;
  sw.half = half;
  for (int j = 0; j < kernel_size; ++j) {
    if (!(weights[j] > 0.0) || !(weights[j] <= 1.0e6)) {
      set_error("nst_camera_smooth_u8: weights must be positive and finite");
      return NST_E_INVALID;
    }
    sw.w[j] = weights[j];
  }
  const bool vec = (fbytes % 4) == 0 && ((uintptr_t)out & 3) == 0;
  const dim3 g = px_grid(fbytes, 4, out_count);
  if (vec)
    hipLaunchKernelGGL(camera_smooth_kernel<true>, g, dim3(256), 0, (hipStream_t)stream, window, fbytes, first, seq_len,
                       out_first, sw, out);
  else
    hipLaunchKernelGGL(camera_smooth_kernel<false>, g, dim3(256), 0, (hipStream_t)stream, window, fbytes, first, seq_len,
                       out_first, sw, out);
  CAM_LAUNCHED("camera_smooth");
  return NST_OK;
}

int nst_camera_scratch_bytes(const nst_camera_frame* frames, int n, size_t* out) {
  if (!frames || !out || n < 1 || n > NST_CAMERA_MAX_FRAMES) {
    set_error("nst_camera_scratch_bytes: invalid arguments (1 <= n <= " + std::to_string(NST_CAMERA_MAX_FRAMES) + ")");
    return NST_E_INVALID;
  }
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    const nst_camera_frame& d = frames[i];
    if (!d.zoom) continue;
    if (d.patch_w < 1 || d.patch_h < 1 || d.patch_w > 32768 || d.patch_h > 32768) {
      set_error("nst_camera_scratch_bytes: frame " + std::to_string(i) + ": patch outside 1..32768");
      return NST_E_INVALID;
    }
    total += align16((size_t)d.patch_w * d.patch_h * 3);
  }
  *out = total;
  return NST_OK;
}

int nst_camera_frames_u8(const uint8_t* in, int n, int h, int w, const nst_camera_frame* frames, int tw, int th,
                         const int32_t* xofs, const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef,
                         int table_slots, uint8_t* out, void* scratch, size_t scratch_bytes, void* stream) {
  int rc;
  if (!in || !out || in == out || !frames) { set_error("nst_camera_frames_u8: invalid arguments (out != in)"); return NST_E_INVALID; }
  if (bad_dims("nst_camera_frames_u8", n, h, w, &rc)) return rc;
  if (tw < 1 || th < 1 || tw > w || th > h) {
    set_error("nst_camera_frames_u8: target " + std::to_string(tw) + "x" + std::to_string(th) + " must fit the " +
              std::to_string(w) + "x" + std::to_string(h) + " frame");
    return NST_E_SHAPE;
  }
  CamBatch cb = {};
  size_t need = 0, max_patch = 0;
  for (int i = 0; i < n; ++i) {
    const nst_camera_frame& d = frames[i];
    CamFrame& f = cb.f[i];
    const std::string who = "nst_camera_frames_u8: frame " + std::to_string(i) + ": ";
    if (!set_pulse(f, h, w, d.pulse_w, d.pulse_h)) { set_error(who + "the pulse size must be at least the frame's"); return NST_E_INVALID; }
    if (!set_subpix(f, h, w, d.patch_w, d.patch_h, d.cx, d.cy)) {
      set_error(who + "the patch must lie inside the frame (corner's floor >= 0, floor + patch <= size)");
      return NST_E_INVALID;
    }
    if (!set_hue(f, d.hue_on, d.hue_half)) { set_error(who + "the half shift must be finite, at most 1e6"); return NST_E_INVALID; }
    f.zoom = d.zoom ? 1 : 0;
    if (f.zoom) {
      if (!xofs || !xcoef || !yofs || !ycoef || d.table < 0 || d.table >= table_slots) {
        set_error(who + "a zoom-phase frame needs the Lanczos tables and a slot below table_slots");
        return NST_E_INVALID;
      }
      f.table = d.table;
      f.scr_off = need;
      const size_t pb = (size_t)d.patch_w * d.patch_h;
      need += align16(pb * 3);
      if (pb > max_patch) max_patch = pb;
    } else if (d.patch_w != tw || d.patch_h != th) {
      set_error(who + "a pan-phase patch is the target's size");
      return NST_E_INVALID;
    }
  }
  if (need > 0 && (!scratch || scratch_bytes < need)) {
    set_error("nst_camera_frames_u8: scratch smaller than nst_camera_scratch_bytes");
    return NST_E_WORKSPACE;
  }
  const hipStream_t st = (hipStream_t)stream;
  const LancTab tab{xofs, xcoef, yofs, ycoef};
  if (need > 0) {
    hipLaunchKernelGGL(camera_crop_kernel, px_grid(max_patch, 1, n), dim3(256), 0, st, in, h, w, cb, (uint8_t*)scratch);
    CAM_LAUNCHED("camera_crop");
  }
  const size_t opix = (size_t)th * tw;
  const bool vec = (opix % 4) == 0 && ((uintptr_t)out & 3) == 0;
  if (vec)
    hipLaunchKernelGGL(camera_out_kernel<true>, px_grid(opix, U8_RUN, n), dim3(256), 0, st, in, h, w, cb, th, tw, tab,
                       (const uint8_t*)scratch, out);
  else
    hipLaunchKernelGGL(camera_out_kernel<false>, px_grid(opix, U8_RUN, n), dim3(256), 0, st, in, h, w, cb, th, tw, tab,
                       (const uint8_t*)scratch, out);
  CAM_LAUNCHED("camera_out");
  return NST_OK;
}

}  // extern "C"
