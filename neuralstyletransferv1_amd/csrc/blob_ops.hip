// blob_ops.hip — the reference's animated soft-blob compositor (scripts/selfstyle_blob.py:
// create_soft_multi_blob_masks :238-274, get_blended_image :277-292, the frame loop of generate_blob_video :401-434;
// the same masks in scripts/morph_faces.py and scripts/gen_pytorch_only_videos.py) on the GPU: per output frame the
// softmax weights of up to NST_BLOB_MAX sine-noise fields and the weighted sum of as many cross-faded u8 stills, in
// one pass (include/nst_hip.h "Soft-blob compositor"); nst_blob_masks gives the weights alone, nst_add_weighted_u8 is
// the loader's cv2.addWeighted.  The run of pixels a thread owns, its load and store, add_weighted and the refusals
// are the compositor core's (u8run_common.h); this file is the noise field, the softmax and its own launch loop.
//
// The arithmetic is the reference's numpy float32 code under the NumPy it pins (every Python scalar rounded to fp32
// once, by the host; every product, sum and quotient rounded alone, in the script's order: built with
// -ffp-contract=off, sinf / expf the accurate library functions, IEEE division).  The arguments of sinf reach about
// 170 rad: no fast intrinsic anywhere.
//
// Cost shape.  The row term depends on y alone and the column term on x alone, so a workgroup evaluates them once for
// the rows and columns it covers and keeps them in LDS; only the diagonal term is one sine per pixel, octave and
// blob.  For that a workgroup owns a rectangle, not 1024 consecutive pixels: BLOB_ROWS rows by BLOB_SLOTS run slots,
// slot k of row y being the k-th run that STARTS in row y (runs stay the flat 4-pixel runs of the core, so a run may
// straddle a row end; every run starts in exactly one row).  Its pixels then lie in rows y .. y + 3 and either in
// columns c0 .. c0 + BLOB_TCOLS - 1 of the block (not wrapped) or in columns 0 .. 2 (wrapped into a following row).
// A block's tables are (19 + 67 + 3) x n_blobs float4 (one component per octave) against 1024 x n_blobs x 4 diagonal
// sines: under 9 % on top.  The weights of the thread's four pixels wait in LDS too (indexed by blob at run time,
// which registers cannot be), n_blobs x 4 KB; the blob loops stay rolled, one inlined sinf per octave.
#include <hip/hip_runtime.h>
#include <math.h>

#include <cstdint>
#include <string>

#include "nst_hip.h"
#include "nst_internal.h"
#include "u8run_common.h"

namespace nst {
namespace {

constexpr int BLOB_ROWS = 16, BLOB_SLOTS = 16;
constexpr int BLOB_THREADS = BLOB_ROWS * BLOB_SLOTS;
static_assert(BLOB_THREADS == 256, "one run per thread of a 256-thread block");
constexpr int BLOB_TROWS = BLOB_ROWS + U8_RUN - 1;                // a run reaches at most U8_RUN - 1 rows further (w = 1)
constexpr int BLOB_TCOLS = BLOB_SLOTS * U8_RUN + U8_RUN - 1;      // slot k starts in column c0 + 4k .. c0 + 4k + 3
constexpr int BLOB_WRAP = U8_RUN - 1;                             // a wrapped pixel lies in column 0 .. 2
constexpr int BLOB_TAB = BLOB_TROWS + BLOB_TCOLS + BLOB_WRAP;     // table entries per blob
constexpr float PI32 = 3.14159274101257324f;                      // np.float32(np.pi)

// dynamic LDS of a block: float4 tab[n_blobs][BLOB_TAB], then float wts[n_blobs][U8_RUN][BLOB_THREADS]
inline size_t blob_lds_bytes(int nb) { return (size_t)nb * (BLOB_TAB * sizeof(float4) + U8_RUN * BLOB_THREADS * sizeof(float)); }

// amp[o] * sinf((((v * freq[o]) * pi32 + phase[o]) + t[o]) + bp) for the four octaves
__device__ __forceinline__ float4 axis_terms(float v, const nst_blob_field& fd, const float* phase, const float* t, float bp) {
  float r[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const float a = (((v * fd.freq[o]) * PI32 + phase[o]) + t[o]) + bp;
    r[o] = fd.amp[o] * sinf(a);
  }
  return make_float4(r[0], r[1], r[2], r[3]);
}

// where the calling thread's run lies
struct BlobRun {
  bool valid;   // the thread owns a run of the frame
  size_t i0;    // its first pixel
  int y, xs;    // the row it starts in, its first column
};

// slot (blockIdx.x, threadIdx.x % BLOB_SLOTS) of row (blockIdx.y, threadIdx.x / BLOB_SLOTS)
__device__ __forceinline__ BlobRun blob_run(int h, int w) {
  BlobRun br;
  br.y = (int)blockIdx.y * BLOB_ROWS + (int)threadIdx.x / BLOB_SLOTS;
  const int k = (int)blockIdx.x * BLOB_SLOTS + (int)threadIdx.x % BLOB_SLOTS;
  const size_t row0 = (size_t)br.y * w;
  const size_t r = (row0 + U8_RUN - 1) / U8_RUN + k;                 // the k-th run that starts at or after the row's start
  br.valid = br.y < h && r < (row0 + w + U8_RUN - 1) / U8_RUN;      // ... and before the next row's
  br.i0 = r * U8_RUN;
  br.xs = br.valid ? (int)(br.i0 - row0) : 0;
  return br;
}

// The softmax weights of the run's four pixels, for every blob, into wts[(b * U8_RUN + j) * BLOB_THREADS + thread]
// (pixels past the frame's end get the values of clamped positions; they are not stored).  Every thread of the block
// must call it (one barrier, behind the tables); a thread reads its own weights only, so none is needed after it.
__device__ __forceinline__ void blob_weights(const nst_blob_field& fd, const nst_blob_frame& fr, int h, int w,
                                             const float* __restrict__ yn, const float* __restrict__ xn,
                                             const BlobRun& br, float4* tab, float* wts) {
  const int nb = fd.n_blobs, tid = (int)threadIdx.x;
  const int y_blk = (int)blockIdx.y * BLOB_ROWS, c0 = (int)blockIdx.x * BLOB_SLOTS * U8_RUN;
  // the block's row and column terms
  for (int idx = tid; idx < nb * BLOB_TAB; idx += BLOB_THREADS) {
    const int b = idx / BLOB_TAB, e = idx % BLOB_TAB;
    const bool row = e < BLOB_TROWS;
    const int col = e < BLOB_TROWS + BLOB_TCOLS ? c0 + (e - BLOB_TROWS) : e - (BLOB_TROWS + BLOB_TCOLS);
    const float v = row ? yn[min(y_blk + e, h - 1)] : xn[min(col, w - 1)];
    tab[idx] = axis_terms(v, fd, row ? fd.phase_y[b] : fd.phase_x[b], row ? fr.t_y : fr.t_x, fd.blob_phase[b]);
  }
  __syncthreads();
  if (!br.valid) return;
  const int ty = tid / BLOB_SLOTS;
#pragma unroll 1
  for (int j = 0; j < U8_RUN; ++j) {
    int xx = br.xs + j, dy = 0;
    while (xx >= w) {  // at most U8_RUN - 1 times
      xx -= w;
      ++dy;
    }
    const int ce = BLOB_TROWS + (dy == 0 ? xx - c0 : BLOB_TCOLS + xx);
    const float xy = xn[xx] + yn[min(br.y + dy, h - 1)];
    float* wj = wts + (size_t)j * BLOB_THREADS + tid;
    float m = 0.f;
#pragma unroll 1
    for (int b = 0; b < nb; ++b) {
      const float4 rt = tab[b * BLOB_TAB + ty + dy], ct = tab[b * BLOB_TAB + ce];
      const float r[4] = {rt.x, rt.y, rt.z, rt.w}, c[4] = {ct.x, ct.y, ct.z, ct.w};
      const float bp = fd.blob_phase[b];
      float noise = 0.f;
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const float a = ((((xy * fd.freq[o]) * PI32) + fd.phase_t[b][o]) + fr.t_t) + bp;
        const float d = fd.amp_half[o] * sinf(a);
        noise = ((noise + r[o]) + c[o]) + d;
      }
      wj[b * U8_RUN * BLOB_THREADS] = noise;
      m = b == 0 ? noise : fmaxf(m, noise);
    }
    float s = 0.f;
#pragma unroll 1
    for (int b = 0; b < nb; ++b) {
      const float e = expf((wj[b * U8_RUN * BLOB_THREADS] - m) / fd.T);
      wj[b * U8_RUN * BLOB_THREADS] = e;
      s = b == 0 ? e : s + e;
    }
    const float den = s + 1e-6f;
#pragma unroll 1
    for (int b = 0; b < nb; ++b) wj[b * U8_RUN * BLOB_THREADS] = wj[b * U8_RUN * BLOB_THREADS] / den;
  }
}

__device__ __forceinline__ int int_of(const RunRaw& r, int e) { return (int)((r.d[e / 4] >> (8 * (e % 4))) & 255u); }

template <bool VEC>
__global__ __launch_bounds__(BLOB_THREADS) void blob_frames_kernel(const uint8_t* __restrict__ bank, int h, int w,
                                                                   const float* __restrict__ yn,
                                                                   const float* __restrict__ xn, nst_blob_field fd,
                                                                   BankBatch<nst_blob_frame> fb, uint8_t* __restrict__ out) {
  extern __shared__ float4 blob_lds[];
  float* wts = (float*)(blob_lds + fd.n_blobs * BLOB_TAB);
  const nst_blob_frame& fr = fb.f[blockIdx.z];
  const BlobRun br = blob_run(h, w);
  blob_weights(fd, fr, h, w, yn, xn, br, blob_lds, wts);
  if (!br.valid) return;
  const size_t hw = (size_t)h * w, fbytes = hw * 3, e0 = br.i0 * 3;
  float F[U8_RUN_BYTES];
#pragma unroll
  for (int e = 0; e < U8_RUN_BYTES; ++e) F[e] = 0.f;
#pragma unroll 1
  for (int b = 0; b < fd.n_blobs; ++b) {
    const nst_blob_still st = fr.blob[b];
    const RunRaw lo = load_run<VEC>(bank + (size_t)st.lo * fbytes, e0, fbytes);
    const RunRaw hi = load_run<VEC>(bank + (size_t)st.hi * fbytes, e0, fbytes);
    float wb[U8_RUN];
#pragma unroll
    for (int j = 0; j < U8_RUN; ++j) wb[j] = wts[(size_t)(b * U8_RUN + j) * BLOB_THREADS + threadIdx.x];
#pragma unroll
    for (int e = 0; e < U8_RUN_BYTES; ++e)
      F[e] = F[e] + (float)add_weighted(int_of(lo, e), int_of(hi, e), st.w_lo, st.w_hi) * wb[e / 3];
  }
  RunBytes rb;
#pragma unroll
  for (int e = 0; e < U8_RUN_BYTES; ++e) rb.b[e] = (uint32_t)clip_u8(F[e]);
  store_run<VEC>(out + (size_t)blockIdx.z * fbytes + e0, rb, run_count<VEC>(br.i0, hw));
}

__global__ __launch_bounds__(BLOB_THREADS) void blob_masks_kernel(int h, int w, const float* __restrict__ yn,
                                                                  const float* __restrict__ xn, nst_blob_field fd,
                                                                  BankBatch<nst_blob_frame> fb, float* __restrict__ out) {
  extern __shared__ float4 blob_lds[];
  float* wts = (float*)(blob_lds + fd.n_blobs * BLOB_TAB);
  const BlobRun br = blob_run(h, w);
  blob_weights(fd, fb.f[blockIdx.z], h, w, yn, xn, br, blob_lds, wts);
  if (!br.valid) return;
  const size_t hw = (size_t)h * w;
  const int cnt = run_count<false>(br.i0, hw);
  for (int b = 0; b < fd.n_blobs; ++b) {
    float* o = out + ((size_t)blockIdx.z * fd.n_blobs + b) * hw + br.i0;
    for (int j = 0; j < cnt; ++j) o[j] = wts[(size_t)(b * U8_RUN + j) * BLOB_THREADS + threadIdx.x];
  }
}

__global__ __launch_bounds__(256) void add_weighted_u8_kernel(const uint8_t* __restrict__ a, float wa,
                                                              const uint8_t* __restrict__ b, float wb, size_t n,
                                                              bool vec, uint8_t* __restrict__ out) {
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  if (vec && n - i >= 4) {
    const uint32_t pa = *(const uint32_t*)(a + i), pb = *(const uint32_t*)(b + i);
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      r |= add_weighted((int)((pa >> (8 * k)) & 255u), (int)((pb >> (8 * k)) & 255u), wa, wb) << (8 * k);
    *(uint32_t*)(out + i) = r;
  } else {
    const int cnt = (int)min((size_t)4, n - i);
    for (int k = 0; k < cnt; ++k) out[i + k] = (uint8_t)add_weighted(a[i + k], b[i + k], wa, wb);
  }
}

// what both blob entry points refuse about the tables and the field
int field_refused(const std::string& who, const float* yn, const float* xn, const nst_blob_field* fd) {
  if (!yn || !xn || !fd) {
    set_error(who + ": invalid arguments (yn, xn, field non-null)");
    return NST_E_INVALID;
  }
  if (fd->n_blobs < 1 || fd->n_blobs > NST_BLOB_MAX) {
    set_error(who + ": n_blobs " + std::to_string(fd->n_blobs) + " outside 1.." + std::to_string(NST_BLOB_MAX));
    return NST_E_INVALID;
  }
  if (!std::isfinite(fd->T) || !(fd->T > 0.f)) {
    set_error(who + ": T must be finite and > 0");
    return NST_E_INVALID;
  }
  return NST_OK;
}

dim3 blob_grid(int h, int w, int g) {
  const int slots = w / U8_RUN + 1;  // no row has more runs starting in it
  return dim3((unsigned)((slots + BLOB_SLOTS - 1) / BLOB_SLOTS), (unsigned)((h + BLOB_ROWS - 1) / BLOB_ROWS), (unsigned)g);
}

static_assert(sizeof(nst_blob_field) + sizeof(BankBatch<nst_blob_frame>) + 64 <= 4096,
              "the field and the descriptors of one launch must fit the kernel-argument block");

}  // namespace
}  // namespace nst

using namespace nst;

extern "C" int nst_blob_frames(const uint8_t* bank, int n_bank, int h, int w, const float* yn, const float* xn,
                               const nst_blob_field* field, const nst_blob_frame* frames, int n, uint8_t* out,
                               void* stream) {
  const std::string me = "nst_blob_frames";
  if (const int rc = bank_call_refused(me, bank, n_bank, h, w, frames, n, out)) return rc;
  if (const int rc = field_refused(me, yn, xn, field)) return rc;
  for (int i = 0; i < n; ++i)
    for (int b = 0; b < field->n_blobs; ++b)
      if (bad_index(frames[i].blob[b].lo, n_bank) || bad_index(frames[i].blob[b].hi, n_bank)) {
        set_error(me + ": frame " + std::to_string(i) + ": a bank index outside 0.." + std::to_string(n_bank - 1));
        return NST_E_INVALID;
      }
  const size_t hw = (size_t)h * w, fbytes = hw * 3;
  if (out_overlaps_bank(me, bank, n_bank, fbytes, out, n)) return NST_E_INVALID;
  const bool vec = (hw % 4) == 0 && ((uintptr_t)bank & 3) == 0 && ((uintptr_t)out & 3) == 0;
  const size_t lds = blob_lds_bytes(field->n_blobs);
  for (int first = 0; first < n; first += BANK_GROUP) {
    const int g = n - first < BANK_GROUP ? n - first : BANK_GROUP;
    BankBatch<nst_blob_frame> batch = {};
    for (int i = 0; i < g; ++i) batch.f[i] = frames[first + i];
    hipLaunchKernelGGL(vec ? blob_frames_kernel<true> : blob_frames_kernel<false>, blob_grid(h, w, g), dim3(BLOB_THREADS),
                       lds, (hipStream_t)stream, bank, h, w, yn, xn, *field, batch, out + (size_t)first * fbytes);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      set_error(std::string("blob_frames launch: ") + hipGetErrorString(e));
      return NST_E_HIP;
    }
  }
  return NST_OK;
}

extern "C" int nst_blob_masks(int h, int w, const float* yn, const float* xn, const nst_blob_field* field,
                              const nst_blob_frame* frames, int n, float* out, void* stream) {
  const std::string me = "nst_blob_masks";
  if (!frames || !out || n < 1) {
    set_error(me + ": invalid arguments (frames, out non-null; n >= 1)");
    return NST_E_INVALID;
  }
  if (bad_frame_shape(me, h, w)) return NST_E_SHAPE;
  if (const int rc = field_refused(me, yn, xn, field)) return rc;
  const size_t hw = (size_t)h * w, lds = blob_lds_bytes(field->n_blobs);
  for (int first = 0; first < n; first += BANK_GROUP) {
    const int g = n - first < BANK_GROUP ? n - first : BANK_GROUP;
    BankBatch<nst_blob_frame> batch = {};
    for (int i = 0; i < g; ++i) batch.f[i] = frames[first + i];
    hipLaunchKernelGGL(blob_masks_kernel, blob_grid(h, w, g), dim3(BLOB_THREADS), lds, (hipStream_t)stream, h, w, yn, xn,
                       *field, batch, out + (size_t)first * field->n_blobs * hw);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      set_error(std::string("blob_masks launch: ") + hipGetErrorString(e));
      return NST_E_HIP;
    }
  }
  return NST_OK;
}

extern "C" int nst_add_weighted_u8(const uint8_t* a, double wa, const uint8_t* b, double wb, size_t n_bytes,
                                   uint8_t* out, void* stream) {
  const std::string me = "nst_add_weighted_u8";
  const size_t blocks = (n_bytes + 1023) / 1024;
  if (!a || !b || !out || n_bytes < 1 || blocks > 0x7fffffffu) {
    set_error(me + ": invalid arguments (a, b, out non-null; n_bytes in 1..(2^31 - 1) * 1024)");
    return NST_E_INVALID;
  }
  if ((out < a + n_bytes && a < out + n_bytes) || (out < b + n_bytes && b < out + n_bytes)) {
    set_error(me + ": out overlaps an input");
    return NST_E_INVALID;
  }
  const bool vec = (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 3) == 0;
  hipLaunchKernelGGL(add_weighted_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, (float)wa, b,
                     (float)wb, n_bytes, vec, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(std::string("add_weighted_u8 launch: ") + hipGetErrorString(e));
    return NST_E_HIP;
  }
  return NST_OK;
}
