// style_morph_ops.hip — the frame loop of the reference's weight-ladder style flow (scripts/style_morph.py:216-298,
// create_video; interpolate_ladder :105-118; the gentle filters :42-59) on the GPU: per output frame one pass over
// the u8 ladder stills it blends (the original, per family the two neighbouring rungs, the same again for the next
// still inside a cross-fade), the clip and truncation to u8, and the still's colour filter, in one launch per group
// of frames (include/nst_hip.h "Style morph").
// The blend is the reference's own numpy float32 arithmetic: every Python scalar is rounded to fp32 once (the host
// does that), every product and sum rounds alone, in the script's order (built with -ffp-contract=off).  Only the
// two cvtColor calls of the saturation filters are restated (hsv_common.h; cv2 absent, parity unpinned); the
// yardstick is tests/style_morph_ref.py, byte for byte.
#include <hip/hip_runtime.h>
#include <math.h>

#include <cstdint>
#include <string>

#include "hsv_common.h"
#include "nst_hip.h"
#include "nst_internal.h"

namespace nst {
namespace {

// Each thread owns SM_RUN consecutive pixels (12 bytes) of the flattened frame, as nst_morph_frames; the frame is
// blockIdx.z of the launch's group.  The descriptors travel by value: SM_GROUP of them fit the 4 KB argument block.
constexpr int SM_RUN = 4;
constexpr int SM_BYTES = SM_RUN * 3;
constexpr int SM_GROUP = 8;
struct SmBatch {
  nst_style_morph_frame f[SM_GROUP];
};
static_assert(sizeof(SmBatch) + 64 <= 4096, "the descriptors of one launch must fit the kernel-argument block");

// the run's 12 bytes of one bank image as floats.  VEC: every image and every run starts on a dword boundary (h*w a
// multiple of 4, the bank aligned); otherwise byte loads, the index clamped to the image (the tail is not stored)
template <bool VEC>
__device__ __forceinline__ void load_run(const uint8_t* __restrict__ img, size_t e0, size_t fbytes, float* v) {
  if (VEC) {
    const uint32_t* p = (const uint32_t*)(img + e0);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const uint32_t d = p[q];
      v[4 * q] = (float)(d & 255u);
      v[4 * q + 1] = (float)((d >> 8) & 255u);
      v[4 * q + 2] = (float)((d >> 16) & 255u);
      v[4 * q + 3] = (float)(d >> 24);
    }
  } else {
#pragma unroll
    for (int e = 0; e < SM_BYTES; ++e) v[e] = (float)img[min(e0 + e, fbytes - 1)];
  }
}

// frame = orig * ORIG_AMOUNT; frame += style_frame * weight per family, style_frame = the ladder image itself (one
// rung) or images[lo] * (1 - blend) + images[hi] * blend
template <bool VEC>
__device__ __forceinline__ void side_sum(const uint8_t* __restrict__ bank, size_t fbytes, size_t e0,
                                         const nst_style_morph_side& sd, float* S) {
  float a[SM_BYTES], b[SM_BYTES];
  load_run<VEC>(bank + (size_t)sd.orig * fbytes, e0, fbytes, a);
  const float ow = sd.orig_w;
#pragma unroll
  for (int e = 0; e < SM_BYTES; ++e) S[e] = a[e] * ow;
  for (int t = 0; t < sd.n_terms; ++t) {
    const nst_style_morph_term& tm = sd.term[t];
    const float wgt = tm.weight;
    load_run<VEC>(bank + (size_t)tm.lo * fbytes, e0, fbytes, a);
    if (tm.hi < 0) {
#pragma unroll
      for (int e = 0; e < SM_BYTES; ++e) S[e] = S[e] + a[e] * wgt;
    } else {
      load_run<VEC>(bank + (size_t)tm.hi * fbytes, e0, fbytes, b);
      const float wl = tm.w_lo, wh = tm.w_hi;
#pragma unroll
      for (int e = 0; e < SM_BYTES; ++e) {
        const float sf = a[e] * wl + b[e] * wh;
        S[e] = S[e] + sf * wgt;
      }
    }
  }
}

// np.clip(x, 0, 255).astype(np.uint8): truncation
__device__ __forceinline__ int clip_u8(float v) { return (int)fminf(fmaxf(v, 0.f), 255.f); }

__device__ __forceinline__ void filter_px(int filter, float p0, float p1, float p2, int* rgb) {
  if (filter == NST_SM_FILTER_WARM) {
    rgb[0] = clip_u8((float)rgb[0] * p0);
    rgb[1] = clip_u8((float)rgb[1] * p1);
    rgb[2] = clip_u8((float)rgb[2] * p2);
  } else if (filter != NST_SM_FILTER_NONE) {
    int h8, s8, v8;
    rgb_to_hsv8(rgb[0], rgb[1], rgb[2], &h8, &s8, &v8);
    const float sat = (float)s8;
    // vibrance: factor + (1 - factor) * (sat / 255), the quotient a true fp32 division
    const float boost = filter == NST_SM_FILTER_VIBRANCE ? p0 + p1 * (sat / 255.f) : p0;
    hsv8_to_rgb(h8, clip_u8(sat * boost), v8, rgb);
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void style_morph_kernel(const uint8_t* __restrict__ bank, size_t hw, SmBatch sb,
                                                          uint8_t* __restrict__ out) {
  const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * SM_RUN;
  if (i0 >= hw) return;
  const nst_style_morph_frame& f = sb.f[blockIdx.z];
  const size_t fbytes = hw * 3, e0 = i0 * 3;
  const int cnt = (int)min((size_t)SM_RUN, hw - i0);
  float S[SM_BYTES];
  side_sum<VEC>(bank, fbytes, e0, f.side[0], S);
  if (f.n_sides == 2) {
    float T[SM_BYTES];
    side_sum<VEC>(bank, fbytes, e0, f.side[1], T);
    const float f0 = f.fade[0], f1 = f.fade[1];
#pragma unroll
    for (int e = 0; e < SM_BYTES; ++e) S[e] = S[e] * f0 + T[e] * f1;
  }
  uint32_t b[SM_BYTES];
  const int filter = f.filter;
  const float p0 = f.fparam[0], p1 = f.fparam[1], p2 = f.fparam[2];
#pragma unroll
  for (int j = 0; j < SM_RUN; ++j) {
    int rgb[3] = {clip_u8(S[j * 3]), clip_u8(S[j * 3 + 1]), clip_u8(S[j * 3 + 2])};
    filter_px(filter, p0, p1, p2, rgb);
    b[j * 3] = (uint32_t)rgb[0];
    b[j * 3 + 1] = (uint32_t)rgb[1];
    b[j * 3 + 2] = (uint32_t)rgb[2];
  }
  uint8_t* o = out + (size_t)blockIdx.z * fbytes + e0;
  if (VEC && cnt == SM_RUN) {
    uint32_t* o4 = (uint32_t*)o;
#pragma unroll
    for (int q = 0; q < 3; ++q) o4[q] = b[4 * q] | (b[4 * q + 1] << 8) | (b[4 * q + 2] << 16) | (b[4 * q + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < SM_RUN; ++j)
      if (j < cnt) {
        o[j * 3] = (uint8_t)b[j * 3];
        o[j * 3 + 1] = (uint8_t)b[j * 3 + 1];
        o[j * 3 + 2] = (uint8_t)b[j * 3 + 2];
      }
  }
}

bool bad_index(int i, int n_bank) { return i < 0 || i >= n_bank; }

}  // namespace
}  // namespace nst

using namespace nst;

extern "C" int nst_style_morph_frames(const uint8_t* bank, int n_bank, int h, int w, const nst_style_morph_frame* frames,
                                      int n, uint8_t* out, void* stream) {
  if (!bank || !out || !frames || n < 1 || n_bank < 1) {
    set_error("nst_style_morph_frames: invalid arguments (bank, frames, out non-null; n >= 1; n_bank >= 1)");
    return NST_E_INVALID;
  }
  if (h < 1 || w < 1 || h > 32768 || w > 32768) {
    set_error("nst_style_morph_frames: frame " + std::to_string(w) + "x" + std::to_string(h) + " outside 1..32768");
    return NST_E_SHAPE;
  }
  for (int i = 0; i < n; ++i) {
    const nst_style_morph_frame& d = frames[i];
    const std::string who = "nst_style_morph_frames: frame " + std::to_string(i) + ": ";
    if (d.n_sides < 1 || d.n_sides > 2) { set_error(who + "n_sides must be 1 or 2"); return NST_E_INVALID; }
    if (d.filter < NST_SM_FILTER_NONE || d.filter > NST_SM_FILTER_WARM) {
      set_error(who + "unknown filter " + std::to_string(d.filter));
      return NST_E_INVALID;
    }
    for (int s = 0; s < d.n_sides; ++s) {
      const nst_style_morph_side& sd = d.side[s];
      if (sd.n_terms < 0 || sd.n_terms > NST_STYLE_MORPH_MAX_STYLES) {
        set_error(who + "n_terms outside 0.." + std::to_string(NST_STYLE_MORPH_MAX_STYLES));
        return NST_E_INVALID;
      }
      bool bad = bad_index(sd.orig, n_bank);
      for (int t = 0; t < sd.n_terms; ++t)
        bad = bad || bad_index(sd.term[t].lo, n_bank) || (sd.term[t].hi >= 0 && bad_index(sd.term[t].hi, n_bank));
      if (bad) {
        set_error(who + "a bank index outside 0.." + std::to_string(n_bank - 1));
        return NST_E_INVALID;
      }
    }
  }
  const size_t hw = (size_t)h * w, fbytes = hw * 3;
  const uint8_t* bank_end = bank + (size_t)n_bank * fbytes;
  const uint8_t* out_end = out + (size_t)n * fbytes;
  if (out < bank_end && bank < out_end) {
    set_error("nst_style_morph_frames: out overlaps the bank");
    return NST_E_INVALID;
  }
  const bool vec = (hw % 4) == 0 && ((uintptr_t)bank & 3) == 0 && ((uintptr_t)out & 3) == 0;
  const size_t threads = (hw + SM_RUN - 1) / SM_RUN;
  for (int first = 0; first < n; first += SM_GROUP) {
    const int g = n - first < SM_GROUP ? n - first : SM_GROUP;
    SmBatch sb = {};
    for (int i = 0; i < g; ++i) sb.f[i] = frames[first + i];
    const dim3 grid((unsigned)((threads + 255) / 256), 1, (unsigned)g);
    uint8_t* o = out + (size_t)first * fbytes;
    if (vec)
      hipLaunchKernelGGL(style_morph_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, bank, hw, sb, o);
    else
      hipLaunchKernelGGL(style_morph_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, bank, hw, sb, o);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      set_error(std::string("style_morph launch: ") + hipGetErrorString(e));
      return NST_E_HIP;
    }
  }
  return NST_OK;
}
