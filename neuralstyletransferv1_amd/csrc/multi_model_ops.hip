// multi_model_ops.hip — the frame loop of the reference's pulsed multi-style compositor (scripts/multi_model_video.py:
// create_multi_model_video :239-353, get_styled_frame :60-107, adjust_saturation :113-122) on the GPU: per output
// frame one pass over the u8 stills it names (the ramped base, up to two pulsed overlays, the fade-in original, the
// cross-fade's next image), every truncation to u8 the script makes between its stages, and the saturation boost, in
// one launch per group of frames (include/nst_hip.h "Multi-model video").
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

namespace nst {
namespace {

// Each thread owns MM_RUN consecutive pixels (12 bytes) of the flattened frame, as nst_style_morph_frames; the frame is
// blockIdx.z of the launch's group.  The descriptors travel by value: MM_GROUP of them fit the 4 KB argument block.
constexpr int MM_RUN = 4;
constexpr int MM_BYTES = MM_RUN * 3;
constexpr int MM_GROUP = 8;
struct MmBatch {
  nst_multi_model_frame f[MM_GROUP];
};
static_assert(sizeof(MmBatch) + 64 <= 4096, "the descriptors of one launch must fit the kernel-argument block");

// a run of one bank image as it lies in memory, four channel bytes per dword
struct Raw {
  uint32_t d[MM_BYTES / 4];
};

__device__ __forceinline__ float byte_of(const Raw& r, int e) { return (float)((r.d[e / 4] >> (8 * (e % 4))) & 255u); }

// VEC: every image and every run starts on a dword boundary (h*w a multiple of 4, the bank aligned); otherwise byte
// loads, the index clamped to the image (the tail is not stored)
template <bool VEC>
__device__ __forceinline__ void load_raw(const uint8_t* __restrict__ img, size_t e0, size_t fbytes, Raw& r) {
  if (VEC) {
    const uint32_t* p = (const uint32_t*)(img + e0);
#pragma unroll
    for (int q = 0; q < MM_BYTES / 4; ++q) r.d[q] = p[q];
  } else {
#pragma unroll
    for (int q = 0; q < MM_BYTES / 4; ++q) {
      uint32_t d = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) d |= (uint32_t)img[min(e0 + 4 * q + k, fbytes - 1)] << (8 * k);
      r.d[q] = d;
    }
  }
}

// np.clip(x, 0, 255).astype(np.uint8): truncation
__device__ __forceinline__ int clip_u8(float v) { return (int)fminf(fmaxf(v, 0.f), 255.f); }
// the same value kept as a float (what .astype(np.float32) then gives)
__device__ __forceinline__ float trunc_u8f(float v) { return truncf(fminf(fmaxf(v, 0.f), 255.f)); }

// ST(s) or a plain image, in two halves so that a stage's loads are all issued before the first is consumed
struct StillRaw {
  Raw o, a, b;
};

template <bool VEC>
__device__ __forceinline__ void still_load(const uint8_t* __restrict__ bank, size_t fbytes, size_t e0,
                                           const nst_multi_model_still& s, bool styled, StillRaw& r) {
  load_raw<VEC>(bank + (size_t)s.orig * fbytes, e0, fbytes, r.o);
  if (styled && s.lo >= 0) {
    load_raw<VEC>(bank + (size_t)s.lo * fbytes, e0, fbytes, r.a);
    if (s.hi >= 0) load_raw<VEC>(bank + (size_t)s.hi * fbytes, e0, fbytes, r.b);
  }
}

// the image's u8 values as floats: bank[orig] itself (plain, or lo < 0), or
// trunc(orig * orig_w + (lo [* w_lo + hi * w_hi]) * style_w)
__device__ __forceinline__ void still_value(const nst_multi_model_still& s, bool styled, const StillRaw& r, float* v) {
  if (!(styled && s.lo >= 0)) {
#pragma unroll
    for (int e = 0; e < MM_BYTES; ++e) v[e] = byte_of(r.o, e);
  } else {
    const float ow = s.orig_w, sw = s.style_w;
    if (s.hi < 0) {
#pragma unroll
      for (int e = 0; e < MM_BYTES; ++e) v[e] = trunc_u8f(byte_of(r.o, e) * ow + byte_of(r.a, e) * sw);
    } else {
      const float wl = s.w_lo, wh = s.w_hi;
#pragma unroll
      for (int e = 0; e < MM_BYTES; ++e) {
        const float sf = byte_of(r.a, e) * wl + byte_of(r.b, e) * wh;
        v[e] = trunc_u8f(byte_of(r.o, e) * ow + sf * sw);
      }
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void multi_model_kernel(const uint8_t* __restrict__ bank, size_t hw, MmBatch mb,
                                                          uint8_t* __restrict__ out) {
  const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * MM_RUN;
  if (i0 >= hw) return;
  const nst_multi_model_frame& f = mb.f[blockIdx.z];
  const size_t fbytes = hw * 3, e0 = i0 * 3;
  const int cnt = (int)min((size_t)MM_RUN, hw - i0);
  float F[MM_BYTES], T[MM_BYTES];
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
    for (int e = 0; e < MM_BYTES; ++e) F[e] = F[e] * keep + T[e] * wk;
  }
  // the loads of the two fades, issued ahead of the saturation arithmetic
  Raw fin;
  const bool fade_in = f.fin >= 0, cross = f.cross_kind != NST_MM_NONE;
  if (fade_in) load_raw<VEC>(bank + (size_t)f.fin * fbytes, e0, fbytes, fin);
  if (cross) still_load<VEC>(bank, fbytes, e0, f.next, f.cross_kind == NST_MM_STYLED, sr);
  if (f.n_over > 0) {
#pragma unroll
    for (int e = 0; e < MM_BYTES; ++e) F[e] = trunc_u8f(F[e]);
  }
  if (f.sat_on) {
    const float factor = f.sat;
#pragma unroll
    for (int j = 0; j < MM_RUN; ++j) {
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
    for (int e = 0; e < MM_BYTES; ++e) F[e] = byte_of(fin, e) * a0 + F[e] * a1;
  }
  if (cross) {
    still_value(f.next, f.cross_kind == NST_MM_STYLED, sr, T);
    const float c0 = f.cross_w[0], c1 = f.cross_w[1];
#pragma unroll
    for (int e = 0; e < MM_BYTES; ++e) F[e] = F[e] * c0 + T[e] * c1;
  }
  uint32_t b[MM_BYTES];
#pragma unroll
  for (int e = 0; e < MM_BYTES; ++e) b[e] = (uint32_t)clip_u8(F[e]);
  uint8_t* o = out + (size_t)blockIdx.z * fbytes + e0;
  if (VEC) {  // h*w is a multiple of MM_RUN: every run is whole
    uint32_t* o4 = (uint32_t*)o;
#pragma unroll
    for (int q = 0; q < 3; ++q) o4[q] = b[4 * q] | (b[4 * q + 1] << 8) | (b[4 * q + 2] << 16) | (b[4 * q + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < MM_RUN; ++j)
      if (j < cnt) {
        o[j * 3] = (uint8_t)b[j * 3];
        o[j * 3 + 1] = (uint8_t)b[j * 3 + 1];
        o[j * 3 + 2] = (uint8_t)b[j * 3 + 2];
      }
  }
}

bool bad_index(int i, int n_bank) { return i < 0 || i >= n_bank; }

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
  if (!bank || !out || !frames || n < 1 || n_bank < 1) {
    set_error("nst_multi_model_frames: invalid arguments (bank, frames, out non-null; n >= 1; n_bank >= 1)");
    return NST_E_INVALID;
  }
  if (h < 1 || w < 1 || h > 32768 || w > 32768) {
    set_error("nst_multi_model_frames: frame " + std::to_string(w) + "x" + std::to_string(h) + " outside 1..32768");
    return NST_E_SHAPE;
  }
  for (int i = 0; i < n; ++i) {
    const nst_multi_model_frame& d = frames[i];
    const std::string who = "nst_multi_model_frames: frame " + std::to_string(i) + ": ";
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
  const size_t hw = (size_t)h * w, fbytes = hw * 3;
  const uint8_t* bank_end = bank + (size_t)n_bank * fbytes;
  const uint8_t* out_end = out + (size_t)n * fbytes;
  if (out < bank_end && bank < out_end) {
    set_error("nst_multi_model_frames: out overlaps the bank");
    return NST_E_INVALID;
  }
  const bool vec = (hw % 4) == 0 && ((uintptr_t)bank & 3) == 0 && ((uintptr_t)out & 3) == 0;
  const size_t threads = (hw + MM_RUN - 1) / MM_RUN;
  for (int first = 0; first < n; first += MM_GROUP) {
    const int g = n - first < MM_GROUP ? n - first : MM_GROUP;
    MmBatch mb = {};
    for (int i = 0; i < g; ++i) mb.f[i] = frames[first + i];
    const dim3 grid((unsigned)((threads + 255) / 256), 1, (unsigned)g);
    uint8_t* o = out + (size_t)first * fbytes;
    if (vec)
      hipLaunchKernelGGL(multi_model_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, bank, hw, mb, o);
    else
      hipLaunchKernelGGL(multi_model_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, bank, hw, mb, o);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      set_error(std::string("multi_model launch: ") + hipGetErrorString(e));
      return NST_E_HIP;
    }
  }
  return NST_OK;
}
