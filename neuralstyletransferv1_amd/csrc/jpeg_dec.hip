// jpeg_dec.hip — device half of the baseline JPEG reader (include/nst_hip.h "JPEG decode"; replaces the host's
// Image.open(frame).convert("RGB"), pipeline.py:1086, for --jpeg_reader gpu).  The host entropy-decodes each frame
// into a coefficient record (jpeg_entropy.cpp, layout in jpeg_common.h); two launches rebuild the pixels exactly as
// libjpeg-turbo's defaults do (islow IDCT, fancy upsampling), so the frames equal Pillow's byte for byte:
//   1 jpeg_idct   one lane per 8x8 block: dequantise, jidctint's islow inverse DCT (CONST_BITS 13, PASS1_BITS 2;
//                 columns descaled by 11, rows by 18), range limit, 8 rows of 8 bytes into the planar u8 workspace
//                 (neighbouring lanes hold neighbouring blocks of a block row, so each row store is contiguous);
//   2 jpeg_color  one lane per 4 consecutive pixels of the flat [n*h*w] pixel stream (12 bytes = 3 aligned dwords
//                 whatever the width): h2v1 / h2v2 "fancy" triangle upsampling of the chroma planes (plain
//                 replication when a chroma plane is at most 2 samples wide), YCbCr -> RGB in 16-bit fixed point,
//                 clamp, NHWC store.  Only the planes' real samples are read, never the MCU grid's padding.
// No atomics, no data-dependent loops: every trip count comes from (n, h, w, components, sampling).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "jpeg_common.h"
#include "nst_hip.h"
#include "nst_internal.h"

namespace nst {
namespace {

struct JpegDims {
  int h, w, comps, sampling;
  int bw[3];              // blocks per block row of each plane (row pitch = bw * 8 bytes)
  int cw, ch;             // real chroma samples per row / rows
  unsigned blk_off[3];    // first block of each plane
  unsigned blocks;        // blocks per frame
  size_t record_bytes;
};

__device__ __forceinline__ int range_limit(int v) {
  const int i = v & 1023;
  return i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896));
}

// jidctint.c's 1-D islow pass: 8 inputs -> 8 outputs, each descaled by SHIFT with round-half-up
template <int SHIFT>
__device__ __forceinline__ void idct8(const int* in, int stride, int* out, int ostride) {
  int z2 = in[2 * stride], z3 = in[6 * stride];
  int z1 = (z2 + z3) * 4433;
  int tmp2 = z1 + z3 * (-15137);
  int tmp3 = z1 + z2 * 6270;
  z2 = in[0];
  z3 = in[4 * stride];
  int tmp0 = (int)((unsigned)(z2 + z3) << 13);
  int tmp1 = (int)((unsigned)(z2 - z3) << 13);
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7 * stride];
  tmp1 = in[5 * stride];
  tmp2 = in[3 * stride];
  tmp3 = in[1 * stride];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * 9633;
  tmp0 *= 2446;
  tmp1 *= 16819;
  tmp2 *= 25172;
  tmp3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 *= -16069;
  z4 *= -3196;
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  constexpr int R = 1 << (SHIFT - 1);
  out[0 * ostride] = (tmp10 + tmp3 + R) >> SHIFT;
  out[7 * ostride] = (tmp10 - tmp3 + R) >> SHIFT;
  out[1 * ostride] = (tmp11 + tmp2 + R) >> SHIFT;
  out[6 * ostride] = (tmp11 - tmp2 + R) >> SHIFT;
  out[2 * ostride] = (tmp12 + tmp1 + R) >> SHIFT;
  out[5 * ostride] = (tmp12 - tmp1 + R) >> SHIFT;
  out[3 * ostride] = (tmp13 + tmp0 + R) >> SHIFT;
  out[4 * ostride] = (tmp13 - tmp0 + R) >> SHIFT;
}

__global__ __launch_bounds__(256) void jpeg_idct(const uint8_t* __restrict__ records, JpegDims d, unsigned total,
                                                 uint8_t* __restrict__ ws) {
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  if (t >= total) return;
  const unsigned f = t / d.blocks, b = t - f * d.blocks;
  const int c = (d.comps == 3 && b >= d.blk_off[1]) ? (b >= d.blk_off[2] ? 2 : 1) : 0;
  const unsigned lb = b - d.blk_off[c];
  const unsigned bw = (unsigned)d.bw[c];
  const unsigned by = lb / bw, bx = lb - by * bw;
  const uint8_t* rec = records + (size_t)f * d.record_bytes;
  const uint4* qv = (const uint4*)(rec + c * 128);
  const uint4* cv = (const uint4*)(rec + NST_JPEG_QT_BYTES + (size_t)b * 128);
  int v[64], m[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint4 q = qv[r], k = cv[r];
    const unsigned qq[4] = {q.x, q.y, q.z, q.w}, kk[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[r * 8 + 2 * j] = (int)(short)(kk[j] & 0xffffu) * (int)(qq[j] & 0xffffu);
      v[r * 8 + 2 * j + 1] = (int)(short)(kk[j] >> 16) * (int)(qq[j] >> 16);
    }
  }
#pragma unroll
  for (int col = 0; col < 8; ++col) idct8<11>(v + col, 8, m + col, 8);
  uint8_t* dst = ws + (size_t)f * d.blocks * 64 + (size_t)d.blk_off[c] * 64 + ((size_t)by * 8 * bw + bx) * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int o[8];
    idct8<18>(m + r * 8, 1, o, 1);
    uint2 px;
    px.x = (unsigned)range_limit(o[0]) | ((unsigned)range_limit(o[1]) << 8) | ((unsigned)range_limit(o[2]) << 16) |
           ((unsigned)range_limit(o[3]) << 24);
    px.y = (unsigned)range_limit(o[4]) | ((unsigned)range_limit(o[5]) << 8) | ((unsigned)range_limit(o[6]) << 16) |
           ((unsigned)range_limit(o[7]) << 24);
    *(uint2*)(dst + (size_t)r * bw * 8) = px;
  }
}

// one chroma sample at full resolution (jdsample.c: h2v1_fancy_upsample / h2v2_fancy_upsample restated per output
// sample; a neighbour index clamped to the plane turns the interior formulas into the edge ones)
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int pitch, const JpegDims& d, int y, int x) {
  if (d.sampling == 0) return p[(size_t)y * pitch + x];
  const int cx = x >> 1;
  if (d.cw <= 2) return p[(size_t)(d.sampling == 2 ? y >> 1 : y) * pitch + cx];
  const int nx = (x & 1) ? min(cx + 1, d.cw - 1) : max(cx - 1, 0);
  if (d.sampling == 1) {
    const uint8_t* row = p + (size_t)y * pitch;
    return (3 * row[cx] + row[nx] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int cy = y >> 1;
  const int fy = (y & 1) ? min(cy + 1, d.ch - 1) : max(cy - 1, 0);
  const uint8_t* near = p + (size_t)cy * pitch;
  const uint8_t* far = p + (size_t)fy * pitch;
  const int cs = 3 * near[cx] + far[cx], ns = 3 * near[nx] + far[nx];
  return (3 * cs + ns + ((x & 1) ? 7 : 8)) >> 4;
}

__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)min(max(v, 0), 255); }

__device__ __forceinline__ void pixel_rgb(const uint8_t* __restrict__ fw, const JpegDims& d, int y, int x,
                                          unsigned* rgb) {
  const int Y = fw[(size_t)y * (d.bw[0] * 8) + x];
  if (d.comps == 1) {
    rgb[0] = rgb[1] = rgb[2] = (unsigned)Y;
    return;
  }
  const int cb = chroma_at(fw + (size_t)d.blk_off[1] * 64, d.bw[1] * 8, d, y, x) - 128;
  const int cr = chroma_at(fw + (size_t)d.blk_off[2] * 64, d.bw[2] * 8, d, y, x) - 128;
  rgb[0] = clamp255(Y + ((91881 * cr + 32768) >> 16));
  rgb[1] = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  rgb[2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
}

__global__ __launch_bounds__(256) void jpeg_color(const uint8_t* __restrict__ ws, JpegDims d, unsigned pixels,
                                                  uint8_t* __restrict__ out) {
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  const unsigned p0 = t * 4u;
  if (p0 >= pixels) return;
  const unsigned hw = (unsigned)d.h * (unsigned)d.w;
  unsigned f = p0 / hw;
  const unsigned rem = p0 - f * hw;
  int y = (int)(rem / (unsigned)d.w), x = (int)(rem - (unsigned)y * (unsigned)d.w);
  const unsigned cnt = min(4u, pixels - p0);
  unsigned px[4][3] = {};
#pragma unroll
  for (unsigned j = 0; j < 4; ++j) {
    if (j < cnt) {
      pixel_rgb(ws + (size_t)f * d.blocks * 64, d, y, x, px[j]);
      if (++x == d.w) {
        x = 0;
        if (++y == d.h) {
          y = 0;
          ++f;
        }
      }
    }
  }
  uint8_t* o = out + (size_t)p0 * 3;
  if (cnt == 4) {
    uint3 v;
    v.x = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
    v.y = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
    v.z = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
    *(uint3*)o = v;
  } else {  // the stream's last 1-3 pixels
    for (unsigned j = 0; j < cnt; ++j) {
      o[3 * j] = (uint8_t)px[j][0];
      o[3 * j + 1] = (uint8_t)px[j][1];
      o[3 * j + 2] = (uint8_t)px[j][2];
    }
  }
}

// geometry + the 32-bit index budget of the kernels
bool jpeg_dims(int n, int h, int w, int comps, int sampling, JpegDims* d, JpegGeom* g) {
  if (n <= 0 || !jpeg_geom(h, w, comps, sampling, g)) return false;
  if ((unsigned long long)n * g->blocks >= (1ull << 31) || (unsigned long long)n * h * w >= (1ull << 31)) return false;
  d->h = h;
  d->w = w;
  d->comps = comps;
  d->sampling = sampling;
  for (int c = 0; c < 3; ++c) {
    d->bw[c] = g->bw[c];
    d->blk_off[c] = (unsigned)g->blk_off[c];
  }
  d->cw = g->pw[1];
  d->ch = g->ph[1];
  d->blocks = (unsigned)g->blocks;
  d->record_bytes = jpeg_record_bytes(*g);
  return true;
}

}  // namespace
}  // namespace nst

using namespace nst;

extern "C" {

int nst_jpeg_workspace_bytes(int n, int h, int w, int comps, int sampling, size_t* out) {
  JpegDims d;
  JpegGeom g;
  if (!out || !jpeg_dims(n, h, w, comps, sampling, &d, &g)) {
    set_error("nst_jpeg_workspace_bytes: invalid arguments (comps 1 or 3, sampling 0..2, n*h*w < 2^31)");
    return NST_E_INVALID;
  }
  *out = (size_t)n * g.blocks * 64;
  return NST_OK;
}

int nst_jpeg_reconstruct_u8(const void* records, size_t record_bytes, int n, int h, int w, int comps, int sampling,
                            uint8_t* out, void* workspace, size_t workspace_bytes, void* stream) {
  JpegDims d;
  JpegGeom g;
  if (!records || !out || !workspace || !jpeg_dims(n, h, w, comps, sampling, &d, &g) ||
      record_bytes != d.record_bytes || (uintptr_t)records % 16 || (uintptr_t)workspace % 16 || (uintptr_t)out % 4) {
    set_error("nst_jpeg_reconstruct_u8: invalid arguments (record_bytes as nst_jpeg_probe reports for this geometry; "
              "records and workspace 16-byte aligned, out 4-byte aligned)");
    return NST_E_INVALID;
  }
  if (workspace_bytes < (size_t)n * g.blocks * 64) {
    set_error("nst_jpeg_reconstruct_u8: workspace smaller than nst_jpeg_workspace_bytes");
    return NST_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const unsigned total = (unsigned)n * d.blocks, pixels = (unsigned)n * (unsigned)h * (unsigned)w;
  hipLaunchKernelGGL(jpeg_idct, dim3((total + 255) / 256), dim3(256), 0, st, (const uint8_t*)records, d, total,
                     (uint8_t*)workspace);
  hipLaunchKernelGGL(jpeg_color, dim3((pixels / 4 + 1 + 255) / 256), dim3(256), 0, st, (const uint8_t*)workspace, d,
                     pixels, out);
  NST_HIP_CHECK(hipGetLastError());
  return NST_OK;
}

}  // extern "C"
