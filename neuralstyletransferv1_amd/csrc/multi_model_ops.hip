// multi_model_ops.hip — the frame loop of the reference's pulsed multi-style compositor (scripts/multi_model_video.py:
// create_multi_model_video :239-353, get_styled_frame :60-107, adjust_saturation :113-122) on the GPU: per output
// frame one pass over the u8 stills it names (the ramped base, up to two pulsed overlays, the fade-in original, the
// cross-fade's next image), every truncation to u8 the script makes between its stages, and the saturation boost, in
// one launch per group of frames (include/nst_hip.h "Multi-model video").  The run of pixels a thread owns, its load
// and store, the shared refusals and the launch loop are the compositor core's (u8run_common.h); this file is the
// stages and the descriptor check.
// The arithmetic is the reference's own numpy float32 code: every Python scalar is rounded to fp32 once (the host
// does that), every product and sum rounds alone, in the script's order (built with -ffp-contract=off).  Only the
// two cvtColor calls of the saturation boost are restated (hsv_common.h; cv2 absent, parity unpinned); the yardstick
// is tests/multi_model_ref.py, byte for byte.
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

// The run, its load and store and the launch frame are the compositor core's (u8run_common.h); a run stays in its
// raw dwords until a stage consumes it (byte_of).

// ST(s) or a plain image, in two halves so that a stage's loads are all issued before the first is consumed
struct StillRaw {
  RunRaw o, a, b;
};

template <bool VEC>
__device__ __forceinline__ void still_load(const uint8_t* __restrict__ bank, size_t fbytes, size_t e0,
                                           const nst_multi_model_still& s, bool styled, StillRaw& r) {
  r.o = load_run<VEC>(bank + (size_t)s.orig * fbytes, e0, fbytes);
  if (styled && s.lo >= 0) {
    r.a = load_run<VEC>(bank + (size_t)s.lo * fbytes, e0, fbytes);
    if (s.hi >= 0) r.b = load_run<VEC>(bank + (size_t)s.hi * fbytes, e0, fbytes);
  }
}

// the image's u8 values as floats: bank[orig] itself (plain, or lo < 0), or
// trunc(orig * orig_w + (lo [* w_lo + hi * w_hi]) * style_w)
__device__ __forceinline__ void still_value(const nst_multi_model_still& s, bool styled, const StillRaw& r, float* v) {
  if (!(styled && s.lo >= 0)) {
#pragma unroll
    for (int e = 0; e < U8_RUN_BYTES; ++e) v[e] = byte_of(r.o, e);
  } else {
    const float ow = s.orig_w, sw = s.style_w;
    if (s.hi < 0) {
#pragma unroll
      for (int e = 0; e < U8_RUN_BYTES; ++e) v[e] = trunc_u8f(byte_of(r.o, e) * ow + byte_of(r.a, e) * sw);
    } else {
      const float wl = s.w_lo, wh = s.w_hi;
#pragma unroll
      for (int e = 0; e < U8_RUN_BYTES; ++e) {
        const float sf = byte_of(r.a, e) * wl + byte_of(r.b, e) * wh;
        v[e] = trunc_u8f(byte_of(r.o, e) * ow + sf * sw);
      }
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void multi_model_kernel(const uint8_t* __restrict__ bank, size_t hw,
                                                          BankBatch<nst_multi_model_frame> mb,
                                                          uint8_t* __restrict__ out) {
  const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * U8_RUN;
  if (i0 >= hw) return;
  const nst_multi_model_frame& f = mb.f[blockIdx.z];
  const size_t fbytes = hw * 3, e0 = i0 * 3;
  float F[U8_RUN_BYTES], T[U8_RUN_BYTES];
  StillRaw sr;
  // base
  still_load<VEC>(bank, fbytes, e0, f.base, f.base_kind == NST_MM_STYLED, sr);
  still_value(f.base, f.base_kind == NST_MM_STYLED, sr, F);
  // overlays: each ST truncated to u8 before it enters the sum, the sum truncated after the last
  for (int k = 0; k < f.n_over; ++k) {
    still_load<VEC>(bank, fbytes, e0, f.over[k], true, sr);
    still_value(f.over[k], true, sr, T);
    const float keep = f.keep[k], wk = f.over_w[k];
#pragma unroll
    for (int e = 0; e < U8_RUN_BYTES; ++e) F[e] = F[e] * keep + T[e] * wk;
  }
  // the loads of the two fades, issued ahead of the saturation arithmetic
  RunRaw fin;
  const bool fade_in = f.fin >= 0, cross = f.cross_kind != NST_MM_NONE;
  if (fade_in) fin = load_run<VEC>(bank + (size_t)f.fin * fbytes, e0, fbytes);
  if (cross) still_load<VEC>(bank, fbytes, e0, f.next, f.cross_kind == NST_MM_STYLED, sr);
  if (f.n_over > 0) {
#pragma unroll
    for (int e = 0; e < U8_RUN_BYTES; ++e) F[e] = trunc_u8f(F[e]);
  }
  if (f.sat_on) {
    const float factor = f.sat;
#pragma unroll
    for (int j = 0; j < U8_RUN; ++j) {
      int h8, s8, v8, rgb[3];
      rgb_to_hsv8((int)F[j * 3], (int)F[j * 3 + 1], (int)F[j * 3 + 2], &h8, &s8, &v8);
      hsv8_to_rgb(h8, clip_u8((float)s8 * factor), v8, rgb);
      F[j * 3] = (float)rgb[0];
      F[j * 3 + 1] = (float)rgb[1];
      F[j * 3 + 2] = (float)rgb[2];
    }
  }
  if (fade_in) {
    const float a0 = f.fin_w[0], a1 = f.fin_w[1];
#pragma unroll
    for (int e = 0; e < U8_RUN_BYTES; ++e) F[e] = byte_of(fin, e) * a0 + F[e] * a1;
  }
  if (cross) {
    still_value(f.next, f.cross_kind == NST_MM_STYLED, sr, T);
    const float c0 = f.cross_w[0], c1 = f.cross_w[1];
#pragma unroll
    for (int e = 0; e < U8_RUN_BYTES; ++e) F[e] = F[e] * c0 + T[e] * c1;
  }
  RunBytes rb;
#pragma unroll
  for (int e = 0; e < U8_RUN_BYTES; ++e) rb.b[e] = (uint32_t)clip_u8(F[e]);
  store_run<VEC>(out + (size_t)blockIdx.z * fbytes + e0, rb, run_count<VEC>(i0, hw));
}

// a still's indices: orig always; lo and hi only where ST reads them (styled; lo < 0: the original alone; hi < 0: one
// rung)
bool bad_still(const nst_multi_model_still& s, bool styled, int n_bank) {
  if (bad_index(s.orig, n_bank)) return true;
  if (!styled || s.lo < 0) return false;
  return bad_index(s.lo, n_bank) || (s.hi >= 0 && bad_index(s.hi, n_bank));
}

}  // namespace
}  // namespace nst

using namespace nst;

extern "C" int nst_multi_model_frames(const uint8_t* bank, int n_bank, int h, int w, const nst_multi_model_frame* frames,
                                      int n, uint8_t* out, void* stream) {
  const std::string me = "nst_multi_model_frames";
  if (const int rc = bank_call_refused(me, bank, n_bank, h, w, frames, n, out)) return rc;
  for (int i = 0; i < n; ++i) {
    const nst_multi_model_frame& d = frames[i];
    const std::string who = me + ": frame " + std::to_string(i) + ": ";
    if (d.base_kind != NST_MM_PLAIN && d.base_kind != NST_MM_STYLED) {
      set_error(who + "unknown base kind " + std::to_string(d.base_kind));
      return NST_E_INVALID;
    }
    if (d.cross_kind != NST_MM_NONE && d.cross_kind != NST_MM_PLAIN && d.cross_kind != NST_MM_STYLED) {
      set_error(who + "unknown cross kind " + std::to_string(d.cross_kind));
      return NST_E_INVALID;
    }
    if (d.n_over < 0 || d.n_over > 2) { set_error(who + "n_over outside 0..2"); return NST_E_INVALID; }
    bool bad = bad_still(d.base, d.base_kind == NST_MM_STYLED, n_bank);
    for (int k = 0; k < d.n_over; ++k) bad = bad || bad_still(d.over[k], true, n_bank);
    bad = bad || (d.fin >= 0 && bad_index(d.fin, n_bank));
    bad = bad || (d.cross_kind != NST_MM_NONE && bad_still(d.next, d.cross_kind == NST_MM_STYLED, n_bank));
    if (bad) {
      set_error(who + "a bank index outside 0.." + std::to_string(n_bank - 1));
      return NST_E_INVALID;
    }
  }
  return launch_bank_frames(me, "multi_model", multi_model_kernel<true>, multi_model_kernel<false>, bank, n_bank, h, w,
                            frames, n, out, stream);
}
