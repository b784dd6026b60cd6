// style_morph_ops.hip — the frame loop of the reference's weight-ladder style flow (scripts/style_morph.py:216-298,
// create_video; interpolate_ladder :105-118; the gentle filters :42-59) on the GPU: per output frame one pass over
// the u8 ladder stills it blends (the original, per family the two neighbouring rungs, the same again for the next
// still inside a cross-fade), the clip and truncation to u8, and the still's colour filter, in one launch per group
// of frames (include/nst_hip.h "Style morph").  The run of pixels a thread owns, its load and store, the shared
// refusals and the launch loop are the compositor core's (u8run_common.h); this file is the blend and the descriptor
// check.
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
#include "u8run_common.h"

namespace nst {
namespace {

// The run, its load and store and the launch frame are the compositor core's (u8run_common.h).  This kernel converts a
// run to floats as it loads it (DESIGN.md §7.5 says why).
template <bool VEC>
__device__ __forceinline__ void load_run_f(const uint8_t* __restrict__ img, size_t e0, size_t fbytes, float* v) {
  const RunRaw r = load_run<VEC>(img, e0, fbytes);
#pragma unroll
  for (int e = 0; e < U8_RUN_BYTES; ++e) v[e] = byte_of(r, e);
}

// frame = orig * ORIG_AMOUNT; frame += style_frame * weight per family, style_frame = the ladder image itself (one
// rung) or images[lo] * (1 - blend) + images[hi] * blend
template <bool VEC>
__device__ __forceinline__ void side_sum(const uint8_t* __restrict__ bank, size_t fbytes, size_t e0,
                                         const nst_style_morph_side& sd, float* S) {
  float a[U8_RUN_BYTES], b[U8_RUN_BYTES];
  load_run_f<VEC>(bank + (size_t)sd.orig * fbytes, e0, fbytes, a);
  const float ow = sd.orig_w;
#pragma unroll
  for (int e = 0; e < U8_RUN_BYTES; ++e) S[e] = a[e] * ow;
  for (int t = 0; t < sd.n_terms; ++t) {
    const nst_style_morph_term& tm = sd.term[t];
    const float wgt = tm.weight;
    load_run_f<VEC>(bank + (size_t)tm.lo * fbytes, e0, fbytes, a);
    if (tm.hi < 0) {
#pragma unroll
      for (int e = 0; e < U8_RUN_BYTES; ++e) S[e] = S[e] + a[e] * wgt;
    } else {
      load_run_f<VEC>(bank + (size_t)tm.hi * fbytes, e0, fbytes, b);
      const float wl = tm.w_lo, wh = tm.w_hi;
#pragma unroll
      for (int e = 0; e < U8_RUN_BYTES; ++e) {
        const float sf = a[e] * wl + b[e] * wh;
        S[e] = S[e] + sf * wgt;
      }
    }
  }
}

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
__global__ __launch_bounds__(256) void style_morph_kernel(const uint8_t* __restrict__ bank, size_t hw,
                                                          BankBatch<nst_style_morph_frame> sb,
                                                          uint8_t* __restrict__ out) {
  const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * U8_RUN;
  if (i0 >= hw) return;
  const nst_style_morph_frame& f = sb.f[blockIdx.z];
  const size_t fbytes = hw * 3, e0 = i0 * 3;
  float S[U8_RUN_BYTES];
  side_sum<VEC>(bank, fbytes, e0, f.side[0], S);
  if (f.n_sides == 2) {
    float T[U8_RUN_BYTES];
    side_sum<VEC>(bank, fbytes, e0, f.side[1], T);
    const float f0 = f.fade[0], f1 = f.fade[1];
#pragma unroll
    for (int e = 0; e < U8_RUN_BYTES; ++e) S[e] = S[e] * f0 + T[e] * f1;
  }
  RunBytes rb;
  const int filter = f.filter;
  const float p0 = f.fparam[0], p1 = f.fparam[1], p2 = f.fparam[2];
#pragma unroll
  for (int j = 0; j < U8_RUN; ++j) {
    int rgb[3] = {clip_u8(S[j * 3]), clip_u8(S[j * 3 + 1]), clip_u8(S[j * 3 + 2])};
    filter_px(filter, p0, p1, p2, rgb);
    rb.b[j * 3] = (uint32_t)rgb[0];
    rb.b[j * 3 + 1] = (uint32_t)rgb[1];
    rb.b[j * 3 + 2] = (uint32_t)rgb[2];
  }
  store_run<VEC>(out + (size_t)blockIdx.z * fbytes + e0, rb, run_count<VEC>(i0, hw));
}

}  // namespace
}  // namespace nst

using namespace nst;

extern "C" int nst_style_morph_frames(const uint8_t* bank, int n_bank, int h, int w, const nst_style_morph_frame* frames,
                                      int n, uint8_t* out, void* stream) {
  const std::string me = "nst_style_morph_frames";
  if (const int rc = bank_call_refused(me, bank, n_bank, h, w, frames, n, out)) return rc;
  for (int i = 0; i < n; ++i) {
    const nst_style_morph_frame& d = frames[i];
    const std::string who = me + ": frame " + std::to_string(i) + ": ";
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
  return launch_bank_frames(me, "style_morph", style_morph_kernel<true>, style_morph_kernel<false>, bank, n_bank, h, w,
                            frames, n, out, stream);
}
