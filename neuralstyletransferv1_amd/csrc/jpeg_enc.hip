// jpeg_enc.hip — baseline JPEG files built on the GPU (include/nst_hip.h "JPEG encode"; replaces the host's
// out_img.save(out_path, format="JPEG", quality=int(jpeg_quality)), pipeline.py:2099-2113, for --image_ext jpg).
//
// Every file equals Pillow's (libjpeg-turbo defaults: 4:2:0, islow FDCT, standard Huffman tables, no restart
// markers) byte for byte; tests/jpeg_enc_ref.py restates the arithmetic in numpy and is pinned to Pillow on the host.
// Block geometry as csrc/jpeg_common.h (sampling 2); blocks are kept in the scan's order: MCU by MCU,
// Y00 Y01 Y10 Y11 Cb Cr, 64 int16 each in zigzag order.
//   1 jpeg_enc_blocks   one lane per block: RGB -> Y / Cb / Cr (edge replication and the h2v2 downsample by clamped
//                       coordinates), islow FDCT on sample - 128 (rows, then columns), quantise, zigzag store.  The MCU
//                       grid's dummy luma blocks are stored as zeros; their DC is the DC of the block coded before
//                       them in the MCU, resolved where the DC is read (dc_at).
//   2 jpeg_enc_len      one lane per block: its DC difference and the bit count of its Huffman codes;
//   3 jpeg_enc_scan     per frame: exclusive prefix sum of the bit counts (block bit offsets) and the total;
//   4 jpeg_enc_put      one lane per block: the same walk writing bits, MSB first, into the frame's unstuffed stream
//                       (32-bit words; the first and the last word of a block are shared with its neighbours and
//                       OR-ed atomically into the zeroed stream -- OR commutes, so the bytes are deterministic);
//   5 jpeg_enc_ffcount  one lane per 32 stream bytes: how many of them are 0xFF (the last byte padded with 1-bits);
//   6 jpeg_enc_scan     per frame: exclusive prefix sum of those counts and the total;
//   7 jpeg_enc_scatter  one lane per 32 stream bytes: the bytes, a 0x00 after every 0xFF, at their file offset;
//   8 jpeg_enc_head     per frame: the fixed header (built on the host per call, a kernel argument), EOI, sizes[j].
// A frame whose file exceeds out_stride gets sizes[j] = -1 and launches 7 and 8 write nothing for it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "jpeg_common.h"
#include "nst_hip.h"
#include "nst_internal.h"

namespace nst {
namespace {

constexpr int CH = 32;               // stream bytes per lane in the stuffing passes
constexpr int HDR_BYTES = 623;       // SOI 2, APP0 18, DQT 2*69, SOF0 19, DHT 33 + 183 + 33 + 183, SOS 14
constexpr int HDR_WORDS = (HDR_BYTES + 3) / 4;
// The longest block: a DC code of at most 11 bits (chrominance, category 11) and 11 value bits, then 63 AC terms
// each with a 16-bit code (the longest in either standard table) and 10 value bits (category 10, the largest an
// 8-bit baseline coefficient reaches): 22 + 63 * 26 = 1660 bits, no ZRL or EOB (no zero among the 63).
constexpr int MAX_BLOCK_BITS = 1660;
constexpr size_t MAX_BLOCKS = (size_t)1 << 21;  // keeps a frame's bit count below 2^32

// libjpeg jcparam.c, natural (row-major) order
constexpr uint8_t kStdQt[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
     69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
     81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
     99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
constexpr uint8_t kZig[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ITU-T T.81 Annex K.3: BITS[1..16] and HUFFVAL of the DC and AC tables, luminance then chrominance
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVal[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

struct HuffConst {     // code | length << 16 per symbol (T.81 Annex C); unused symbols 0
  uint32_t dc[2][16];  // DC category 0..11 (HUFFVAL of both DC tables is 0..11 in order)
  uint32_t ac[2][256];
};

constexpr HuffConst make_huff() {
  HuffConst t{};
  for (int k = 0; k < 2; ++k) {
    uint32_t code = 0;
    int i = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int j = 0; j < kDcBits[k][len - 1]; ++j) t.dc[k][i++] = code++ | ((uint32_t)len << 16);
      code <<= 1;
    }
    code = 0;
    i = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int j = 0; j < kAcBits[k][len - 1]; ++j) t.ac[k][kAcVal[k][i++]] = code++ | ((uint32_t)len << 16);
      code <<= 1;
    }
  }
  return t;
}

__constant__ HuffConst kHuff = make_huff();

struct QuantArg {       // natural order, [0] luminance, [1] chrominance (kernel argument)
  uint16_t half[2][64];  // divisor / 2, divisor = 8 * table entry
  uint32_t recip[2][64]; // ceil(2^32 / divisor): (t * recip) >> 32 == t / divisor for t * divisor < 2^32
};

struct HeaderArg {
  uint32_t w[HDR_WORDS];  // the header's bytes in memory order
};

struct Geo {  // what the kernels need of JpegGeom (sampling 2)
  int h, w;
  int mcux, mcuy;  // MCU grid; luma blocks 2*mcux x 2*mcuy, chroma mcux x mcuy
  int rbw, rbh;    // real luma blocks per row / block rows: ceil(w/8), ceil(h/8)
  int ph;          // real chroma rows: ceil(h/2)
  uint32_t blocks;  // 6 * mcux * mcuy
};

// ---- 1: samples -> quantised blocks ----
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c (islow) over d[0], d[S], ..., d[7*S]; kFirst: the row pass (results scaled up by PASS1_BITS = 2)
template <bool kFirst, int S>
__device__ __forceinline__ void fdct8(int* d) {
  constexpr int SH = kFirst ? 11 : 15;  // CONST_BITS -/+ PASS1_BITS
  int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S], t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
  int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S], t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = kFirst ? (t10 + t11) << 2 : descale(t10 + t11, 2);
  d[4 * S] = kFirst ? (t10 - t11) << 2 : descale(t10 - t11, 2);
  int z1 = (t12 + t13) * 4433;
  d[2 * S] = descale(z1 + t13 * 6270, SH);
  d[6 * S] = descale(z1 - t12 * 15137, SH);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7 * S] = descale(t4 + z1 + z3, SH);
  d[5 * S] = descale(t5 + z2 + z4, SH);
  d[3 * S] = descale(t6 + z2 + z3, SH);
  d[S] = descale(t7 + z1 + z4, SH);
}

// grid.x: luma workgroups, then Cb's, then Cr's (the component is uniform over a workgroup, so the quantisation
// table is read with scalar loads); lanes in each plane's raster order, so a wave reads neighbouring pixels
__global__ __launch_bounds__(64) void jpeg_enc_blocks(const uint8_t* frames, Geo g, int wgs_y, int wgs_c, QuantArg qa,
                                                     int16_t* coef) {
  const int bx0 = blockIdx.x;
  const int comp = bx0 < wgs_y ? 0 : (bx0 < wgs_y + wgs_c ? 1 : 2);
  const int p = (bx0 - (comp == 0 ? 0 : comp == 1 ? wgs_y : wgs_y + wgs_c)) * 64 + (int)threadIdx.x;
  const int bw = comp ? g.mcux : 2 * g.mcux, bh = comp ? g.mcuy : 2 * g.mcuy;
  if (p >= bw * bh) return;
  const int by = p / bw, bx = p % bw;
  const uint32_t idx = comp ? (uint32_t)(by * g.mcux + bx) * 6u + 3u + comp
                            : (uint32_t)((by >> 1) * g.mcux + (bx >> 1)) * 6u + (by & 1) * 2 + (bx & 1);
  uint4* o = reinterpret_cast<uint4*>(coef + ((size_t)blockIdx.y * g.blocks + idx) * 64);
  if (comp == 0 && (bx >= g.rbw || by >= g.rbh)) {  // dummy block of the MCU grid
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = make_uint4(0, 0, 0, 0);
    return;
  }
  const uint8_t* fr = frames + (size_t)blockIdx.y * g.h * g.w * 3;
  const size_t pitch = (size_t)g.w * 3;
  int d[64];
  if (comp == 0) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int y = min(by * 8 + r, g.h - 1);
      const uint8_t* row = fr + y * pitch;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint8_t* px = row + 3 * min(bx * 8 + c, g.w - 1);
        d[r * 8 + c] = ((19595 * px[0] + 38470 * px[1] + 7471 * px[2] + 32768) >> 16) - 128;
      }
    }
  } else {
    // Cb / Cr of one pixel, 16 fractional bits kept until after the shift (jccolor.c)
    const int cr_ = comp == 1 ? -11059 : 32768, cg = comp == 1 ? -21709 : -27439, cb_ = comp == 1 ? 32768 : -5329;
    constexpr int OFF = (128 << 16) + 32767;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int cy = min(by * 8 + r, g.ph - 1);  // rows past the plane repeat the last downsampled row
      const uint8_t* r0 = fr + (size_t)(2 * cy) * pitch;
      const uint8_t* r1 = fr + (size_t)min(2 * cy + 1, g.h - 1) * pitch;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int cx = bx * 8 + c;
        const int x0 = 3 * min(2 * cx, g.w - 1), x1 = 3 * min(2 * cx + 1, g.w - 1);
        int s = 0;
        s += (cr_ * r0[x0] + cg * r0[x0 + 1] + cb_ * r0[x0 + 2] + OFF) >> 16;
        s += (cr_ * r0[x1] + cg * r0[x1 + 1] + cb_ * r0[x1 + 2] + OFF) >> 16;
        s += (cr_ * r1[x0] + cg * r1[x0 + 1] + cb_ * r1[x0 + 2] + OFF) >> 16;
        s += (cr_ * r1[x1] + cg * r1[x1 + 1] + cb_ * r1[x1 + 2] + OFF) >> 16;
        d[r * 8 + c] = ((s + 1 + (c & 1)) >> 2) - 128;  // h2v2 bias 1, 2, 1, 2, ... along a row
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) fdct8<true, 1>(d + r * 8);
#pragma unroll
  for (int c = 0; c < 8; ++c) fdct8<false, 8>(d + c);
  const int t = comp ? 1 : 0;
  uint32_t wv[32];
#pragma unroll
  for (int zz = 0; zz < 64; ++zz) {
    const int nat = kZig[zz];
    const int v = d[nat];
    const uint32_t a = (uint32_t)(v < 0 ? -v : v) + qa.half[t][nat];
    const int q = (int)__umulhi(a, qa.recip[t][nat]);
    const uint32_t u = (uint32_t)(v < 0 ? -q : q) & 0xffffu;
    if (zz & 1) wv[zz >> 1] |= u << 16;
    else wv[zz >> 1] = u;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = make_uint4(wv[4 * i], wv[4 * i + 1], wv[4 * i + 2], wv[4 * i + 3]);
}

// ---- 2 / 4: the Huffman walk over one block ----
// DC of luma block k (0..3, MCU order) of an MCU: a dummy block has the DC of the block coded before it (jccoefct.c)
__device__ __forceinline__ int dc_at(const int16_t* coef, const Geo& g, uint32_t mcu, int k) {
  if (k < 4) {
    const int mx = (int)(mcu % (uint32_t)g.mcux), my = (int)(mcu / (uint32_t)g.mcux);
    while (k > 0 && (2 * mx + (k & 1) >= g.rbw || 2 * my + (k >> 1) >= g.rbh)) --k;  // Y00 is always real
  }
  return coef[((size_t)mcu * 6 + k) * 64];
}

// the DC difference of block idx (coded order) against its component's predictor
__device__ __forceinline__ int dc_diff(const int16_t* coef, const Geo& g, uint32_t idx) {
  const uint32_t mcu = idx / 6u;
  const int k = (int)(idx % 6u);
  const int dc = dc_at(coef, g, mcu, k);
  int pred = 0;
  if (k > 0 && k < 4) pred = dc_at(coef, g, mcu, k - 1);
  else if (mcu > 0) pred = dc_at(coef, g, mcu - 1, k == 0 ? 3 : k);
  return dc - pred;
}

__device__ __forceinline__ int category(int v) { return 32 - __clz(v < 0 ? -v : v); }

// Sink gets put(bits, count), count <= 26: a code followed by its value bits (negative values as v - 1)
template <class Sink>
__device__ __forceinline__ void code_block(const int16_t* blk, int diff, const uint32_t* dct, const uint32_t* act,
                                           Sink& s) {
  const uint4* c4 = reinterpret_cast<const uint4*>(blk);
  uint32_t wv[32];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint4 v = c4[i];
    wv[4 * i] = v.x; wv[4 * i + 1] = v.y; wv[4 * i + 2] = v.z; wv[4 * i + 3] = v.w;
  }
  {
    const int nb = category(diff) & 15;
    const uint32_t e = dct[nb];
    s.put(((e & 0xffffu) << nb) | ((uint32_t)(diff - (diff < 0)) & ((1u << nb) - 1u)), (int)(e >> 16) + nb);
  }
  int run = 0;
#pragma unroll
  for (int zz = 1; zz < 64; ++zz) {
    const int v = (int16_t)(wv[zz >> 1] >> (16 * (zz & 1)));
    if (v == 0) {
      ++run;
    } else {
      while (run > 15) {
        s.put(act[0xf0] & 0xffffu, (int)(act[0xf0] >> 16));  // ZRL
        run -= 16;
      }
      const int nb = category(v) & 15;
      const uint32_t e = act[(run << 4) | nb];
      s.put(((e & 0xffffu) << nb) | ((uint32_t)(v - (v < 0)) & ((1u << nb) - 1u)), (int)(e >> 16) + nb);
      run = 0;
    }
  }
  if (run) s.put(act[0] & 0xffffu, (int)(act[0] >> 16));  // EOB
}

__device__ __forceinline__ void load_huff(uint32_t* dct, uint32_t* act) {  // [2][16], [2][256]
  for (int i = threadIdx.x; i < 32; i += blockDim.x) dct[i] = kHuff.dc[i >> 4][i & 15];
  for (int i = threadIdx.x; i < 512; i += blockDim.x) act[i] = kHuff.ac[i >> 8][i & 255];
  __syncthreads();
}

struct LenSink {
  uint32_t bits = 0;
  __device__ __forceinline__ void put(uint32_t, int n) { bits += (uint32_t)n; }
};

__global__ __launch_bounds__(256) void jpeg_enc_len(const int16_t* coef, Geo g, uint32_t* bits) {
  __shared__ uint32_t dct[32], act[512];
  load_huff(dct, act);
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= g.blocks) return;
  const int16_t* fc = coef + (size_t)blockIdx.y * g.blocks * 64;
  const int t = idx % 6u >= 4u;
  LenSink s;
  code_block(fc + (size_t)idx * 64, dc_diff(fc, g, idx), dct + 16 * t, act + 256 * t, s);
  bits[(size_t)blockIdx.y * g.blocks + idx] = s.bits;
}

struct BitSink {  // MSB-first bits into 32-bit words (word value = its four stream bytes, first byte on top)
  uint32_t* s;
  uint32_t wi, words;  // next word; words in the stream (nothing is written past them)
  uint64_t acc = 0;
  int cnt;            // bits of acc not written yet (the first word's leading bits belong to earlier blocks: zero)
  bool first = true;  // the next word is shared with the block before
  __device__ __forceinline__ void put(uint32_t v, int n) {
    acc = (acc << n) | v;
    cnt += n;
    if (cnt >= 32) {
      cnt -= 32;
      const uint32_t w = (uint32_t)(acc >> cnt);
      if (wi < words) {
        if (first) atomicOr(&s[wi], w);
        else s[wi] = w;
      }
      first = false;
      ++wi;
    }
  }
  __device__ __forceinline__ void finish() {  // the last word is shared with the block after
    if (cnt && wi < words) atomicOr(&s[wi], (uint32_t)(acc << (32 - cnt)));
  }
};

__global__ __launch_bounds__(256) void jpeg_enc_put(const int16_t* coef, Geo g, const uint32_t* boff,
                                                   uint32_t* stream, uint32_t swords) {
  __shared__ uint32_t dct[32], act[512];
  load_huff(dct, act);
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= g.blocks) return;
  const int16_t* fc = coef + (size_t)blockIdx.y * g.blocks * 64;
  const int t = idx % 6u >= 4u;
  const uint32_t o = boff[(size_t)blockIdx.y * g.blocks + idx];
  BitSink s{stream + (size_t)blockIdx.y * swords, o >> 5, swords};
  s.cnt = (int)(o & 31u);
  code_block(fc + (size_t)idx * 64, dc_diff(fc, g, idx), dct + 16 * t, act + 256 * t, s);
  s.finish();
}

// ---- 3 / 6: per-frame exclusive prefix sum ----
constexpr int SCAN_T = 1024;

__device__ __forceinline__ uint32_t stream_bytes(uint32_t bits) { return (bits + 7u) / 8u; }
__device__ __forceinline__ uint32_t live_chunks(uint32_t bits) { return (stream_bytes(bits) + CH - 1) / CH; }

// frame blockIdx.x: out[i] = in[0] + ... + in[i-1] for i < n, tot = the sum.  n = n_fixed, or with kChunks the
// frame's live stuffing chunks (from its bit total).  Each thread owns a contiguous run of ceil(n / 1024) items.
template <bool kChunks>
__global__ __launch_bounds__(SCAN_T) void jpeg_enc_scan(const uint32_t* in, uint32_t* out, uint32_t* tot,
                                                       size_t stride, uint32_t n_fixed, const uint32_t* tbits) {
  __shared__ uint32_t part[SCAN_T];
  const uint32_t t = threadIdx.x;
  const uint32_t n = kChunks ? live_chunks(tbits[blockIdx.x]) : n_fixed;
  const uint32_t per = (n + SCAN_T - 1) / SCAN_T;
  const uint32_t i0 = min(n, t * per), i1 = min(n, i0 + per);
  const uint32_t* fi = in + blockIdx.x * stride;
  uint32_t* fo = out + blockIdx.x * stride;
  uint32_t sum = 0;
  for (uint32_t i = i0; i < i1; ++i) sum += fi[i];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < SCAN_T; d <<= 1) {  // inclusive scan (Hillis-Steele)
    const uint32_t v = t >= (uint32_t)d ? part[t - d] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t run = part[t] - sum;
  for (uint32_t i = i0; i < i1; ++i) {
    const uint32_t v = fi[i];
    fo[i] = run;
    run += v;
  }
  if (t == SCAN_T - 1) tot[blockIdx.x] = part[t];
}

// ---- 5 / 7: 0xFF stuffing ----
// byte i (< nbytes) of the stream as the file has it: the last byte's unused low bits are 1
__device__ __forceinline__ uint32_t stream_byte(const uint32_t* wv, int i, uint32_t pos, uint32_t nbytes,
                                                uint32_t bits) {
  uint32_t b = (wv[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu;
  if (pos == nbytes - 1 && (bits & 7u)) b |= (1u << (8 - (bits & 7u))) - 1u;
  return b;
}

__global__ __launch_bounds__(256) void jpeg_enc_ffcount(const uint32_t* stream, uint32_t swords,
                                                       const uint32_t* tbits, uint32_t* ffcnt, uint32_t nch) {
  const uint32_t ch = blockIdx.x * 256u + threadIdx.x;
  const uint32_t bits = tbits[blockIdx.y], nbytes = stream_bytes(bits);
  if (ch >= nch || ch * CH >= nbytes) return;
  const uint4* s4 = reinterpret_cast<const uint4*>(stream + (size_t)blockIdx.y * swords + (size_t)ch * (CH / 4));
  const uint4 a = s4[0], b = s4[1];
  const uint32_t wv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const uint32_t pos = ch * CH + i;
    c += pos < nbytes && stream_byte(wv, i, pos, nbytes, bits) == 0xffu;
  }
  ffcnt[(size_t)blockIdx.y * nch + ch] = c;
}

__device__ __forceinline__ uint64_t file_bytes(uint32_t bits, uint32_t fftot) {
  return (uint64_t)HDR_BYTES + stream_bytes(bits) + fftot + 2;
}

__global__ __launch_bounds__(256) void jpeg_enc_scatter(const uint32_t* stream, uint32_t swords,
                                                       const uint32_t* tbits, const uint32_t* ffoff,
                                                       const uint32_t* fftot, uint32_t nch, uint8_t* out,
                                                       size_t out_stride) {
  const uint32_t ch = blockIdx.x * 256u + threadIdx.x;
  const uint32_t bits = tbits[blockIdx.y], nbytes = stream_bytes(bits);
  if (ch >= nch || ch * CH >= nbytes) return;
  if (file_bytes(bits, fftot[blockIdx.y]) > out_stride) return;  // the file does not fit: its slot stays untouched
  const uint4* s4 = reinterpret_cast<const uint4*>(stream + (size_t)blockIdx.y * swords + (size_t)ch * (CH / 4));
  const uint4 a = s4[0], b = s4[1];
  const uint32_t wv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint8_t* d = out + blockIdx.y * out_stride + HDR_BYTES + (size_t)ch * CH + ffoff[(size_t)blockIdx.y * nch + ch];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const uint32_t pos = ch * CH + i;
    if (pos < nbytes) {
      const uint32_t v = stream_byte(wv, i, pos, nbytes, bits);
      *d++ = (uint8_t)v;
      if (v == 0xffu) *d++ = 0;
    }
  }
}

// ---- 8: header, EOI, size ----
__global__ __launch_bounds__(64) void jpeg_enc_head(HeaderArg hd, const uint32_t* tbits, const uint32_t* fftot,
                                                   uint8_t* out, size_t out_stride, int64_t* sizes) {
  if (threadIdx.x) return;
  const uint64_t size = file_bytes(tbits[blockIdx.x], fftot[blockIdx.x]);
  if (size > out_stride) {
    sizes[blockIdx.x] = -1;
    return;
  }
  uint8_t* o = out + blockIdx.x * out_stride;  // 16-byte aligned
  uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
  for (int i = 0; i < HDR_BYTES / 4; ++i) o32[i] = hd.w[i];
#pragma unroll
  for (int i = HDR_BYTES / 4 * 4; i < HDR_BYTES; ++i) o[i] = (uint8_t)(hd.w[i / 4] >> (8 * (i % 4)));
  o[size - 2] = 0xff;
  o[size - 1] = 0xd9;
  sizes[blockIdx.x] = (int64_t)size;
}

// ---- host ----
void quant_table(int quality, int t, uint8_t* qt) {  // jcparam.c jpeg_set_quality with force_baseline, natural order
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    const int v = (kStdQt[t][i] * scale + 50) / 100;
    qt[i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
  }
}

// SOI, APP0 (JFIF 1.1, units 0, density 1:1), DQT x 2, SOF0 (4:2:0), DHT x 4, SOS: what libjpeg's jcmarker.c writes
HeaderArg make_header(int h, int w, const uint8_t qt[2][64]) {
  uint8_t b[HDR_WORDS * 4] = {};
  int n = 0;
  auto put = [&](int v) { b[n++] = (uint8_t)v; };
  auto put16 = [&](int v) { put(v >> 8); put(v & 0xff); };
  put16(0xffd8);
  put16(0xffe0); put16(16);
  for (char c : {'J', 'F', 'I', 'F'}) put(c);
  put(0); put(1); put(1); put(0); put16(1); put16(1); put(0); put(0);
  for (int t = 0; t < 2; ++t) {
    put16(0xffdb); put16(67); put(t);
    for (int i = 0; i < 64; ++i) put(qt[t][kZig[i]]);
  }
  put16(0xffc0); put16(17); put(8); put16(h); put16(w); put(3);
  put(1); put(0x22); put(0);
  put(2); put(0x11); put(1);
  put(3); put(0x11); put(1);
  for (int t = 0; t < 2; ++t) {
    put16(0xffc4); put16(19 + 12); put(t);
    for (int i = 0; i < 16; ++i) put(kDcBits[t][i]);
    for (int i = 0; i < 12; ++i) put(i);
    put16(0xffc4); put16(19 + 162); put(0x10 | t);
    for (int i = 0; i < 16; ++i) put(kAcBits[t][i]);
    for (int i = 0; i < 162; ++i) put(kAcVal[t][i]);
  }
  put16(0xffda); put16(12); put(3);
  put(1); put(0x00); put(2); put(0x11); put(3); put(0x11);
  put(0); put(63); put(0);
  static_assert(HDR_BYTES == 2 + 18 + 2 * 69 + 19 + 2 * (33 + 183) + 14, "header size");
  HeaderArg hd{};
  for (int i = 0; i < HDR_WORDS; ++i)
    hd.w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
              ((uint32_t)b[4 * i + 3] << 24);
  return hd;
}

bool enc_geom(int h, int w, JpegGeom* g) { return jpeg_geom(h, w, 3, 2, g) && g->blocks <= MAX_BLOCKS; }

size_t stream_words(const JpegGeom& g) {  // the unstuffed scan at its longest, in whole stuffing chunks
  const size_t words = (g.blocks * MAX_BLOCK_BITS + 31) / 32 + 1;
  return (words + CH / 4 - 1) / (CH / 4) * (CH / 4);
}

struct WsLayout {
  size_t coef, bits, boff, stream, ffcnt, ffoff, tbits, fftot, total;
};

WsLayout ws_layout(int n, const JpegGeom& g) {
  auto al = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t nch = stream_words(g) / (CH / 4);
  WsLayout L{};
  size_t o = 0;
  L.coef = o;   o += al((size_t)n * g.blocks * 128);
  L.bits = o;   o += al((size_t)n * g.blocks * 4);
  L.boff = o;   o += al((size_t)n * g.blocks * 4);
  L.stream = o; o += al((size_t)n * stream_words(g) * 4);
  L.ffcnt = o;  o += al((size_t)n * nch * 4);
  L.ffoff = o;  o += al((size_t)n * nch * 4);
  L.tbits = o;  o += al((size_t)n * 4);
  L.fftot = o;  o += al((size_t)n * 4);
  L.total = o;
  return L;
}

}  // namespace
}  // namespace nst

using namespace nst;

extern "C" {

int nst_jpeg_enc_bound(int h, int w, size_t* out_stride) {
  JpegGeom g;
  if (!out_stride || !enc_geom(h, w, &g)) {
    set_error("nst_jpeg_enc_bound: invalid arguments (h, w in 1..65535, at most 2^21 blocks)");
    return NST_E_INVALID;
  }
  // every block at its longest (MAX_BLOCK_BITS above), every stream byte a stuffed 0xFF, the header and EOI
  const size_t b = HDR_BYTES + 2 * ((g.blocks * MAX_BLOCK_BITS + 7) / 8) + 2;
  *out_stride = (b + 15) / 16 * 16;
  return NST_OK;
}

int nst_jpeg_enc_workspace_bytes(int n, int h, int w, size_t* out) {
  JpegGeom g;
  if (!out || n < 1 || !enc_geom(h, w, &g)) {
    set_error("nst_jpeg_enc_workspace_bytes: invalid arguments");
    return NST_E_INVALID;
  }
  *out = ws_layout(n, g).total;
  return NST_OK;
}

int nst_jpeg_encode_u8(const uint8_t* frames, int n, int h, int w, int quality, uint8_t* out, size_t out_stride,
                       int64_t* sizes, void* workspace, size_t workspace_bytes, void* stream) {
  JpegGeom jg;
  if (!frames || !out || !sizes || !workspace || n < 1 || !enc_geom(h, w, &jg) || quality < 1 || quality > 100 ||
      out_stride == 0 || out_stride % 16 || (uintptr_t)out % 16 || (uintptr_t)workspace % 16) {
    set_error("nst_jpeg_encode_u8: invalid arguments (n >= 1, h, w in 1..65535, quality in 1..100, out, out_stride "
              "and workspace 16-byte aligned)");
    return NST_E_INVALID;
  }
  const WsLayout L = ws_layout(n, jg);
  if (workspace_bytes < L.total) {
    set_error("nst_jpeg_encode_u8: invalid arguments (workspace smaller than nst_jpeg_enc_workspace_bytes)");
    return NST_E_INVALID;
  }
  uint8_t qt[2][64];
  QuantArg qa;
  for (int t = 0; t < 2; ++t) {
    quant_table(quality, t, qt[t]);
    for (int i = 0; i < 64; ++i) {
      const uint32_t div = 8u * qt[t][i];
      qa.half[t][i] = (uint16_t)(div / 2);
      qa.recip[t][i] = (uint32_t)((((uint64_t)1 << 32) + div - 1) / div);
    }
  }
  const HeaderArg hd = make_header(h, w, qt);
  Geo g{h, w, jg.bw[1], jg.bh[1], (w + 7) / 8, (h + 7) / 8, jg.ph[1], (uint32_t)jg.blocks};
  hipStream_t st = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)workspace;
  int16_t* coef = (int16_t*)(ws + L.coef);
  uint32_t* bits = (uint32_t*)(ws + L.bits);
  uint32_t* boff = (uint32_t*)(ws + L.boff);
  uint32_t* strm = (uint32_t*)(ws + L.stream);
  uint32_t* ffcnt = (uint32_t*)(ws + L.ffcnt);
  uint32_t* ffoff = (uint32_t*)(ws + L.ffoff);
  uint32_t* tbits = (uint32_t*)(ws + L.tbits);
  uint32_t* fftot = (uint32_t*)(ws + L.fftot);
  const uint32_t swords = (uint32_t)stream_words(jg), nch = swords / (CH / 4);
  const int wgs_y = (jg.bw[0] * jg.bh[0] + 63) / 64, wgs_c = (jg.bw[1] * jg.bh[1] + 63) / 64;
  const dim3 per_block((g.blocks + 255) / 256, n), per_chunk((nch + 255) / 256, n);
  NST_HIP_CHECK(hipMemsetAsync(strm, 0, (size_t)n * swords * 4, st));
  hipLaunchKernelGGL(jpeg_enc_blocks, dim3(wgs_y + 2 * wgs_c, n), dim3(64), 0, st, frames, g, wgs_y, wgs_c, qa, coef);
  hipLaunchKernelGGL(jpeg_enc_len, per_block, dim3(256), 0, st, coef, g, bits);
  hipLaunchKernelGGL(jpeg_enc_scan<false>, dim3(n), dim3(SCAN_T), 0, st, bits, boff, tbits, (size_t)g.blocks, g.blocks,
                     (const uint32_t*)nullptr);
  hipLaunchKernelGGL(jpeg_enc_put, per_block, dim3(256), 0, st, coef, g, boff, strm, swords);
  hipLaunchKernelGGL(jpeg_enc_ffcount, per_chunk, dim3(256), 0, st, strm, swords, tbits, ffcnt, nch);
  hipLaunchKernelGGL(jpeg_enc_scan<true>, dim3(n), dim3(SCAN_T), 0, st, ffcnt, ffoff, fftot, (size_t)nch, 0u, tbits);
  hipLaunchKernelGGL(jpeg_enc_scatter, per_chunk, dim3(256), 0, st, strm, swords, tbits, ffoff, fftot, nch, out,
                     out_stride);
  hipLaunchKernelGGL(jpeg_enc_head, dim3(n), dim3(64), 0, st, hd, tbits, fftot, out, out_stride, sizes);
  NST_HIP_CHECK(hipGetLastError());
  return NST_OK;
}

}  // extern "C"
