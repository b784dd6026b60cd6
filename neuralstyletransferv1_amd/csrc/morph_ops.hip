// morph_ops.hip — the optical-flow morph between two stills (the reference's optical_flow_morph:
// scripts/optical_flow_slideshow.py:17-70, scripts/morph_v2.py:365-468) on the GPU, beside the Farneback flows of
// flow_ops.hip (launch_farneback_ex):
//   * cv2.cvtColor(COLOR_BGR2GRAY) of 8-bit images: (R*9798 + G*19235 + B*3735 + 16384) >> 15;
//   * morph_v2's pre-blur cv2.GaussianBlur(gray, (5, 5), 1.0) in fp32 (see gauss_u8_kernel);
//   * morph_v2's flow post-processing: GaussianBlur((15, 15), 3.0) of each component, then the radial term where
//     the blurred flow is shorter than 2 px;
//   * every frame of a transition in one launch: two cv2.remap(INTER_LINEAR, BORDER_REFLECT) warps in OpenCV's
//     1/32-pixel fixed point and cv2.addWeighted, per pixel over all k frames; the run of pixels a thread owns, its
//     store and add_weighted are the compositor core's (u8run_common.h).
// cv2 is not installed here: all of it is restated from OpenCV's sources and the scripts, parity unpinned.  The
// translation unit is built with -ffp-contract=off: every fp32 product and sum rounds on its own, in the order written.
#include <math.h>

#include "blur_internal.h"
#include "border_common.h"
#include "flow_internal.h"
#include "u8run_common.h"

namespace nst {

__global__ __launch_bounds__(256) void gray_cv_kernel(const uint8_t* __restrict__ rgb, size_t npix, uint8_t* __restrict__ g) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const uint32_t r = rgb[3 * i], gg = rgb[3 * i + 1], b = rgb[3 * i + 2];
  g[i] = (uint8_t)((r * 9798u + gg * 19235u + b * 3735u + 16384u) >> 15);
}

hipError_t launch_gray_cv(const uint8_t* rgb, size_t npix, uint8_t* gray, hipStream_t st) {
  hipLaunchKernelGGL(gray_cv_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, rgb, npix, gray);
  return hipGetLastError();
}

struct Taps5 {
  float t[5];
};
struct Taps15 {
  float t[15];
};

// cv2.GaussianBlur(u8, (5, 5), 1.0) as the float path would do it: the rows' 5-tap sums (BORDER_REFLECT_101), then
// the columns' over those, each acc = acc + t[j] * v in tap order as blur_rows_kernel / blur_cols_kernel, then
// rounded half-to-even to u8.  One thread per output pixel recomputes the 5 row sums it needs (the same values a
// row pass would have stored).  OpenCV >= 4 blurs 8-bit images in 8.8 fixed point instead, so cv2's own result may
// differ from this one by 1 grey level; that difference is unmeasured (cv2 absent).
__global__ __launch_bounds__(256) void gauss_u8_kernel(const uint8_t* __restrict__ in, int h, int w, Taps5 tp,
                                                       uint8_t* __restrict__ out) {
  const size_t hw = (size_t)h * w;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const uint8_t* src = in + (size_t)blockIdx.z * hw;
  const int x = (int)(i % w), y = (int)(i / w);
  int xs[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) xs[j] = border_reflect101(x + j - 2, w);
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const uint8_t* row = src + (size_t)border_reflect101(y + r - 2, h) * w;
    float ra = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) ra = ra + tp.t[j] * (float)row[xs[j]];
    acc = acc + tp.t[r] * ra;
  }
  out[(size_t)blockIdx.z * hw + i] = (uint8_t)fminf(fmaxf(rintf(acc), 0.f), 255.f);
}

hipError_t launch_gauss_u8(const uint8_t* in, int n, int h, int w, uint8_t* out, hipStream_t st) {
  Taps5 tp;
  gaussian_taps_f32(5, 1.0, tp.t);
  const size_t hw = (size_t)h * w;
  hipLaunchKernelGGL(gauss_u8_kernel, dim3((unsigned)((hw + 255) / 256), 1, (unsigned)n), dim3(256), 0, st, in, h, w, tp,
                     out);
  return hipGetLastError();
}

// ---- morph_v2.py:405-432: blur both flow components 15 x 15 (sigma 3, REFLECT_101; rows then columns, the
// accumulation order of blur_rows_kernel / blur_cols_kernel), then add the radial term where the blurred flow
// is shorter than 2 px.  numpy adds the float64 term to the float32 flow and rounds once. ----
__global__ __launch_bounds__(256) void flow_blur_rows_kernel(const float2* __restrict__ in, int h, int w, Taps15 tp,
                                                             float2* __restrict__ out) {
  const size_t hw = (size_t)h * w;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const int x = (int)(i % w), y = (int)(i / w);
  const float2* row = in + (size_t)blockIdx.z * hw + (size_t)y * w;
  float ax = 0.f, ay = 0.f;
#pragma unroll
  for (int j = 0; j < 15; ++j) {
    const float2 v = row[border_reflect101(x + j - 7, w)];
    ax = ax + tp.t[j] * v.x;
    ay = ay + tp.t[j] * v.y;
  }
  out[(size_t)blockIdx.z * hw + i] = make_float2(ax, ay);
}

struct Signs {
  float s[16];
};

__global__ __launch_bounds__(256) void flow_blur_cols_radial_kernel(const float2* __restrict__ in, int h, int w, Taps15 tp,
                                                                    Signs sg, float2* __restrict__ out) {
  const size_t hw = (size_t)h * w;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const int x = (int)(i % w), y = (int)(i / w);
  const float2* pl = in + (size_t)blockIdx.z * hw;
  float dx = 0.f, dy = 0.f;
#pragma unroll
  for (int j = 0; j < 15; ++j) {
    const float2 v = pl[(size_t)border_reflect101(y + j - 7, h) * w + x];
    dx = dx + tp.t[j] * v.x;
    dy = dy + tp.t[j] * v.y;
  }
  const float mag = sqrtf(dx * dx + dy * dy);
  if (mag < 2.0f) {
    const double s = (double)sg.s[blockIdx.z];
    dx = (float)((double)dx + s * (((double)x - w / 2.0) / w) * 4.0);
    dy = (float)((double)dy + s * (((double)y - h / 2.0) / h) * 4.0);
  }
  out[(size_t)blockIdx.z * hw + i] = make_float2(dx, dy);
}

hipError_t launch_morph_flow_post(float* flow, int n, int h, int w, const float* sign, float* scratch, hipStream_t st) {
  Taps15 tp;
  gaussian_taps_f32(15, 3.0, tp.t);
  Signs sg;
  for (int i = 0; i < 16; ++i) sg.s[i] = i < n ? sign[i] : 0.f;
  const size_t hw = (size_t)h * w;
  const dim3 g((unsigned)((hw + 255) / 256), 1, (unsigned)n);
  hipLaunchKernelGGL(flow_blur_rows_kernel, g, dim3(256), 0, st, (const float2*)flow, h, w, tp, (float2*)scratch);
  hipLaunchKernelGGL(flow_blur_cols_radial_kernel, g, dim3(256), 0, st, (const float2*)scratch, h, w, tp, sg,
                     (float2*)flow);
  return hipGetLastError();
}

// ---- all frames of a transition in one launch ----
struct MorphSched {
  int k;
  float t[128], omt[128], wa[128], wb[128];  // NST_MORPH_MAX_FRAMES
};

// cv2.remap(INTER_LINEAR, BORDER_REFLECT) of one u8 RGB pixel at the fp32 map position (mx, my): the position is
// clamped far outside the frame first (NaN to the low end; cv2's saturate_cast<int>(map * 32) saturates), which
// keeps the int conversion defined and reflects to the same sample; then 5 fraction bits, the four taps reflected
// one by one, integer weights (32 - fx) * (32 - fy) * 32 ... (sum 32768), (sum + 16384) >> 15
__device__ __forceinline__ void remap_reflect(const uint8_t* __restrict__ img, int h, int w, float mx, float my, int* rgb) {
  mx = fminf(fmaxf(mx, -2.f * w), 3.f * w);
  my = fminf(fmaxf(my, -2.f * h), 3.f * h);
  const int X = (int)rintf(mx * 32.f), Y = (int)rintf(my * 32.f);
  const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
  const int x0 = border_reflect(sx, w), x1 = border_reflect(sx + 1, w);
  const int y0 = border_reflect(sy, h), y1 = border_reflect(sy + 1, h);
  const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
  const uint8_t* p00 = img + ((size_t)y0 * w + x0) * 3;
  const uint8_t* p01 = img + ((size_t)y0 * w + x1) * 3;
  const uint8_t* p10 = img + ((size_t)y1 * w + x0) * 3;
  const uint8_t* p11 = img + ((size_t)y1 * w + x1) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    rgb[c] = (w00 * (int)p00[c] + w01 * (int)p01[c] + w10 * (int)p10[c] + w11 * (int)p11[c] + 16384) >> 15;
}

// Each thread owns one run of U8_RUN consecutive pixels (u8run_common.h), loads their forward and backward flow
// vectors once and loops over the k frames: the 16 B of flow per pixel are read once per transition, not once per
// frame.  Every frame's 12 output bytes leave through store_run.  The run's pixel count stays the computed one under
// VEC too (run_count<false>): with it folded to the constant the compiler schedules the gathers differently and the
// kernel measured 5 to 25 % slower (profiles/compositor_core_ab.txt).
template <bool VEC>
__global__ __launch_bounds__(256) void morph_frames_kernel(const uint8_t* __restrict__ img1, const uint8_t* __restrict__ img2,
                                                           const float2* __restrict__ fwd, const float2* __restrict__ bwd,
                                                           int h, int w, MorphSched sc, uint8_t* __restrict__ out) {
  const size_t hw = (size_t)h * w;
  const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * U8_RUN;
  if (i0 >= hw) return;
  const int cnt = run_count<false>(i0, hw);
  float2 ff[U8_RUN], fb[U8_RUN];
  float px[U8_RUN], py[U8_RUN];
#pragma unroll
  for (int j = 0; j < U8_RUN; ++j) {
    const size_t i = min(i0 + j, hw - 1);
    ff[j] = fwd[i];
    fb[j] = bwd[i];
    px[j] = (float)(int)(i % w);
    py[j] = (float)(int)(i / w);
  }
  for (int f = 0; f < sc.k; ++f) {
    const float t = sc.t[f], omt = sc.omt[f], wa = sc.wa[f], wb = sc.wb[f];
    RunBytes rb;
#pragma unroll
    for (int j = 0; j < U8_RUN; ++j) {
      int a[3], c[3];
      remap_reflect(img1, h, w, px[j] + t * ff[j].x, py[j] + t * ff[j].y, a);
      remap_reflect(img2, h, w, px[j] + omt * fb[j].x, py[j] + omt * fb[j].y, c);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) rb.b[j * 3 + ch] = add_weighted(a[ch], c[ch], wa, wb);
    }
    store_run<VEC>(out + ((size_t)f * hw + i0) * 3, rb, cnt);
  }
}

hipError_t launch_morph_frames(const uint8_t* img1, const uint8_t* img2, const float* fwd, const float* bwd, int h,
                               int w, int k, const float* t, const float* omt, const float* wa, const float* wb,
                               uint8_t* out, hipStream_t st) {
  MorphSched sc;
  sc.k = k;
  for (int f = 0; f < 128; ++f) {
    const bool in = f < k;
    sc.t[f] = in ? t[f] : 0.f;
    sc.omt[f] = in ? omt[f] : 0.f;
    sc.wa[f] = in ? wa[f] : 0.f;
    sc.wb[f] = in ? wb[f] : 0.f;
  }
  const size_t hw = (size_t)h * w;
  const size_t threads = (hw + U8_RUN - 1) / U8_RUN;
  const dim3 g((unsigned)((threads + 255) / 256));
  const bool vec = (hw % 4) == 0 && ((uintptr_t)out & 3) == 0;
  if (vec)
    hipLaunchKernelGGL(morph_frames_kernel<true>, g, dim3(256), 0, st, img1, img2, (const float2*)fwd, (const float2*)bwd,
                       h, w, sc, out);
  else
    hipLaunchKernelGGL(morph_frames_kernel<false>, g, dim3(256), 0, st, img1, img2, (const float2*)fwd,
                       (const float2*)bwd, h, w, sc, out);
  return hipGetLastError();
}

}  // namespace nst
