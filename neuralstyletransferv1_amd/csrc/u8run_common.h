// u8run_common.h — what the u8 frame compositors share (morph_frames_kernel, camera_out_kernel, style_morph_kernel,
// multi_model_kernel, blob_frames_kernel and their entry points; DESIGN.md §7.4 "The compositor core").
// Device: each thread owns U8_RUN consecutive pixels (12 bytes) of the flattened RGB frame.  A run of a source image
// is loaded as three dwords (RunRaw), the 12 result bytes leave through store_run.  VEC: every image and every run
// starts on a dword boundary (h*w a multiple of 4, the buffers 4-byte aligned), so every run is whole and moves as
// dwords; otherwise bytes, loads clamped to the image and stores masked by the run's pixel count.
// Host: the 1..32768 shape refusal of every frame entry point, and the frame of a bank call (a u8 bank of stills, a
// table of by-value frame descriptors, one launch per group of BANK_GROUP frames).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include <cstdint>
#include <string>

#include "nst_hip.h"
#include "nst_internal.h"

namespace nst {

constexpr int U8_RUN = 4;
constexpr int U8_RUN_BYTES = U8_RUN * 3;

// a run of one image as it lies in memory, four channel bytes per dword
struct RunRaw {
  uint32_t d[U8_RUN_BYTES / 4];
};

__device__ __forceinline__ float byte_of(const RunRaw& r, int e) { return (float)((r.d[e / 4] >> (8 * (e % 4))) & 255u); }

// the pixels of the run at pixel i0 of an hw-pixel frame: the tail run of a frame is short only without VEC
template <bool VEC>
__device__ __forceinline__ int run_count(size_t i0, size_t hw) {
  return VEC ? U8_RUN : (int)min((size_t)U8_RUN, hw - i0);
}

// the run at byte e0 of the fbytes-byte image `img`; without VEC the index is clamped to the image (the tail is not
// stored)
template <bool VEC>
__device__ __forceinline__ RunRaw load_run(const uint8_t* __restrict__ img, size_t e0, size_t fbytes) {
  RunRaw r;
  if (VEC) {
    const uint32_t* p = (const uint32_t*)(img + e0);
#pragma unroll
    for (int q = 0; q < U8_RUN_BYTES / 4; ++q) r.d[q] = p[q];
  } else {
#pragma unroll
    for (int q = 0; q < U8_RUN_BYTES / 4; ++q) {
      uint32_t d = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) d |= (uint32_t)img[min(e0 + 4 * q + k, fbytes - 1)] << (8 * k);
      r.d[q] = d;
    }
  }
  return r;
}

// np.clip(x, 0, 255).astype(np.uint8): truncation
__device__ __forceinline__ int clip_u8(float v) { return (int)fminf(fmaxf(v, 0.f), 255.f); }
// the same value kept as a float (what .astype(np.float32) then gives)
__device__ __forceinline__ float trunc_u8f(float v) { return truncf(fminf(fmaxf(v, 0.f), 255.f)); }

// cv2.addWeighted on 8-bit images: saturate(rint_half_even(p1 * wa + p2 * wb)) in fp32
__device__ __forceinline__ uint32_t add_weighted(int p1, int p2, float wa, float wb) {
  const float v = (float)p1 * wa + (float)p2 * wb;
  return (uint32_t)fminf(fmaxf(rintf(v), 0.f), 255.f);
}

// a run's 12 result bytes, each 0..255 in a register of its own
struct RunBytes {
  uint32_t b[U8_RUN_BYTES];
};

// the run's result bytes to dst: three dword stores, or the first cnt pixels byte by byte.  The bytes travel by value:
// through a pointer the compiler keeps morph_frames_kernel at 107 VGPRs (4 waves) where the value form gives 70
template <bool VEC>
__device__ __forceinline__ void store_run(uint8_t* dst, const RunBytes rb, int cnt) {
  const uint32_t* b = rb.b;
  if (VEC && cnt == U8_RUN) {
    uint32_t* o4 = (uint32_t*)dst;
#pragma unroll
    for (int q = 0; q < 3; ++q) o4[q] = b[4 * q] | (b[4 * q + 1] << 8) | (b[4 * q + 2] << 16) | (b[4 * q + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < U8_RUN; ++j)
      if (j < cnt) {
        dst[j * 3] = (uint8_t)b[j * 3];
        dst[j * 3 + 1] = (uint8_t)b[j * 3 + 1];
        dst[j * 3 + 2] = (uint8_t)b[j * 3 + 2];
      }
  }
}

// ---- host ----
// the shape every frame entry point takes; the caller returns NST_E_SHAPE
inline bool bad_frame_shape(const std::string& who, int h, int w) {
  if (h >= 1 && w >= 1 && h <= 32768 && w <= 32768) return false;
  set_error(who + ": frame " + std::to_string(w) + "x" + std::to_string(h) + " outside 1..32768");
  return true;
}

// A bank call: nst_<who>(bank [n_bank,h,w,3], frames[n], out [n,h,w,3]).  Its refusals come in this order: arguments
// and shape (bank_call_refused), every descriptor of every frame (the entry point's own loop, bad_index for the bank
// indices), overlap (launch_bank_frames, before its first launch).
inline int bank_call_refused(const std::string& who, const void* bank, int n_bank, int h, int w, const void* frames,
                             int n, const void* out) {
  if (!bank || !out || !frames || n < 1 || n_bank < 1) {
    set_error(who + ": invalid arguments (bank, frames, out non-null; n >= 1; n_bank >= 1)");
    return NST_E_INVALID;
  }
  return bad_frame_shape(who, h, w) ? NST_E_SHAPE : NST_OK;
}

inline bool bad_index(int i, int n_bank) { return i < 0 || i >= n_bank; }

// the last refusal of a bank call: n output frames of fbytes bytes may not overlap the bank
inline bool out_overlaps_bank(const std::string& who, const uint8_t* bank, int n_bank, size_t fbytes, const uint8_t* out,
                              int n) {
  const uint8_t* bank_end = bank + (size_t)n_bank * fbytes;
  const uint8_t* out_end = out + (size_t)n * fbytes;
  if (!(out < bank_end && bank < out_end)) return false;
  set_error(who + ": out overlaps the bank");
  return true;
}

// The descriptors travel by value, the frame is blockIdx.z of the launch's group: BANK_GROUP of them fit the 4 KB
// argument block.
constexpr int BANK_GROUP = 8;
template <class Frame>
struct BankBatch {
  Frame f[BANK_GROUP];
};
template <class Frame>
using BankKernel = void (*)(const uint8_t*, size_t, BankBatch<Frame>, uint8_t*);

// kernel(bank, h * w, group, out of the group's first frame) over 256-thread blocks of runs, grid.z = the group's
// frames; `what` names the kernel in a launch error
template <class Frame>
int launch_bank_frames(const std::string& who, const char* what, BankKernel<Frame> kernel_vec,
                       BankKernel<Frame> kernel_bytes, const uint8_t* bank, int n_bank, int h, int w,
                       const Frame* frames, int n, uint8_t* out, void* stream) {
  static_assert(sizeof(BankBatch<Frame>) + 64 <= 4096, "the descriptors of one launch must fit the kernel-argument block");
  const size_t hw = (size_t)h * w, fbytes = hw * 3;
  if (out_overlaps_bank(who, bank, n_bank, fbytes, out, n)) return NST_E_INVALID;
  const bool vec = (hw % 4) == 0 && ((uintptr_t)bank & 3) == 0 && ((uintptr_t)out & 3) == 0;
  const size_t threads = (hw + U8_RUN - 1) / U8_RUN;
  for (int first = 0; first < n; first += BANK_GROUP) {
    const int g = n - first < BANK_GROUP ? n - first : BANK_GROUP;
    BankBatch<Frame> batch = {};
    for (int i = 0; i < g; ++i) batch.f[i] = frames[first + i];
    const dim3 grid((unsigned)((threads + 255) / 256), 1, (unsigned)g);
    hipLaunchKernelGGL(vec ? kernel_vec : kernel_bytes, grid, dim3(256), 0, (hipStream_t)stream, bank, hw, batch,
                       out + (size_t)first * fbytes);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      set_error(std::string(what) + " launch: " + hipGetErrorString(e));
      return NST_E_HIP;
    }
  }
  return NST_OK;
}

}  // namespace nst
