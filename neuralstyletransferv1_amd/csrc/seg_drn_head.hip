// seg_drn_head.hip — the DRN-D head of the DeepLab v3+ mask program (drn.py:124-134): layer0 7x7 3->16, layer1 3x3
// 16->16 and layer2 3x3 stride 2 16->32, each + BatchNorm + ReLU, all at FULL input resolution.  Through the GEMM
// conv these would need a 147..192-element im2col row per full-resolution pixel and would issue 128 output rows for
// 16 real ones, so they run as one templated direct convolution <K, CIN, COUT, STRIDE>:
//   * a workgroup makes a TWO x TY tile of output pixels; the weights ([tap][cin][cout] fp32, 9-18 KB) and the
//     input tile with its halo are staged in LDS once, with 16-byte (u8 frames: byte) coalesced loads;
//   * the input tile is kept channel-group major — [row][16-byte channel group][column] — so the 16 lanes that
//     share a row read consecutive 16-byte vectors (ds_read_b128 without bank conflicts at stride 1); the 3-channel
//     layer0 tile is planar fp32 [row][channel][column], normalised (preprocess_pil, sky_swap.py:179-183) on the
//     way in, so the zero padding is zero AFTER the normalisation as in launch_seg_stem_im2col;
//   * a thread owns PX output pixels (columns tx, tx + 16, ...: lanes of a row store consecutive pixels) x 16
//     output channels in fp32 registers; layer2's two 16-channel halves go to different waves (wave-uniform), so
//     every weight read is one LDS broadcast shared by PX pixels x 16 channels of FMAs;
//   * epilogue: acc * scale + shift (eval BatchNorm folded), ReLU, 16-byte stores of the NHWC pixel in the
//     activation dtype; channels between COUT and the channel stride (layer2: the GEMM stage width) get zeros.
// VALU fp32 FMAs in every compute dtype: 16 real output channels leave an MFMA tile mostly empty in the exact-f32
// mode (MFMA f32 = VALU rate), and the head is a few percent of the network's MACs.
#include <hip/hip_runtime.h>

#include "nst_hip.h"
#include "seg_internal.h"

namespace nst {

namespace {

enum { HEAD_IN_F32_NCHW = 0, HEAD_IN_U8_NHWC = 1, HEAD_IN_ACT = 2 };

template <int K, int CIN, int COUT, int STRIDE, int TY, int DT, int INK>
struct HeadCfg {
  static constexpr bool ACT_F32 = DT == NST_DT_F32;
  static constexpr int PX = STRIDE == 1 ? 4 : 2;        // output pixels per thread
  static constexpr int NH = COUT / 16;                  // 16-channel halves, one per group of waves
  static constexpr int NT = 16 * TY * NH;               // threads: 16 columns x TY rows x NH halves
  static constexpr int TWO = 16 * PX, THO = TY;         // output tile
  static constexpr int TWI = (TWO - 1) * STRIDE + K, THI = (THO - 1) * STRIDE + K;  // input tile with halo
  static constexpr int PAD = K / 2;
  static constexpr int ESZ = INK == HEAD_IN_ACT ? (ACT_F32 ? 4 : 2) : 4;  // element size of the LDS input tile
  static constexpr int CV = CIN == 3 ? 1 : 16 / ESZ;    // channels per 16-byte group
  static constexpr int CG = CIN == 3 ? 3 : CIN / CV;
  static constexpr int W_BYTES = K * K * CIN * COUT * 4;
  static constexpr int IN_BYTES = CIN == 3 ? THI * 3 * TWI * 4 : THI * CG * TWI * 16;
  static constexpr int LUT_BYTES = INK == HEAD_IN_U8_NHWC ? 768 * 4 : 0;
  static constexpr int IN_OFF = (W_BYTES + 15) / 16 * 16;
  static constexpr int LUT_OFF = (IN_OFF + IN_BYTES + 15) / 16 * 16;
  static constexpr int LDS_BYTES = LUT_OFF + LUT_BYTES;
  static_assert(COUT % 16 == 0 && (16 * TY) % 64 == 0, "a 16-channel half must be wave-uniform");
  static_assert(CIN == 3 || CIN % CV == 0, "whole 16-byte channel groups");
  static_assert((K * K * CIN * COUT) % 4 == 0, "weights copied as float4");
  static_assert(LDS_BYTES <= 64 * 1024, "static LDS");
};

__device__ __forceinline__ uint16_t head_bf16_rne(float f) {
  const uint32_t u = __float_as_uint(f);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
template <int DT>
__device__ __forceinline__ uint32_t head_pack2(float a, float b) {
  if constexpr (DT == NST_DT_F16)
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)a) | ((uint32_t)__builtin_bit_cast(uint16_t, (_Float16)b) << 16);
  else
    return (uint32_t)head_bf16_rne(a) | ((uint32_t)head_bf16_rne(b) << 16);
}
// the two 16-bit values of one dword -> fp32
template <int DT>
__device__ __forceinline__ void head_unpack2(uint32_t u, float& lo, float& hi) {
  if constexpr (DT == NST_DT_F16) {
    lo = (float)__builtin_bit_cast(_Float16, (uint16_t)(u & 0xffffu));
    hi = (float)__builtin_bit_cast(_Float16, (uint16_t)(u >> 16));
  } else {
    lo = __uint_as_float(u << 16);
    hi = __uint_as_float(u & 0xffff0000u);
  }
}

template <int K, int CIN, int COUT, int STRIDE, int TY, int DT, int INK>
__global__ __launch_bounds__(16 * TY * (COUT / 16)) void drn_head_kernel(
    const void* __restrict__ in, int h, int w, const float* __restrict__ wt, const float* __restrict__ scale,
    const float* __restrict__ shift, void* __restrict__ out, int ho, int wo, int out_cs) {
  using C = HeadCfg<K, CIN, COUT, STRIDE, TY, DT, INK>;
  constexpr int PX = C::PX, TWI = C::TWI, THI = C::THI, CV = C::CV, CG = C::CG, NT = C::NT;
  __shared__ __attribute__((aligned(16))) char lds[C::LDS_BYTES];
  float* wl = (float*)lds;
  char* tin = lds + C::IN_OFF;

  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = (tid >> 4) % TY;
  const int half = __builtin_amdgcn_readfirstlane(tid / (16 * TY));  // wave-uniform: 16 * TY is a multiple of 64
  const int img = blockIdx.z;
  const int ox0 = blockIdx.x * C::TWO, oy0 = blockIdx.y * C::THO;
  const int ix0 = ox0 * STRIDE - C::PAD, iy0 = oy0 * STRIDE - C::PAD;

  // ---- weights -> LDS (once per workgroup) ----
  for (int i = tid; i < C::W_BYTES / 16; i += NT) ((float4*)wl)[i] = ((const float4*)wt)[i];

  // ---- input tile + halo -> LDS ----
  if constexpr (INK == HEAD_IN_ACT) {
    const char* src = (const char*)in + (size_t)img * h * w * (CIN * C::ESZ);
    for (int i = tid; i < THI * TWI * CG; i += NT) {
      const int cg = i % CG, col = (i / CG) % TWI, row = i / (CG * TWI);
      const int gy = iy0 + row, gx = ix0 + col;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if ((unsigned)gy < (unsigned)h && (unsigned)gx < (unsigned)w)
        v = *(const uint4*)(src + ((size_t)gy * w + gx) * (CIN * C::ESZ) + cg * 16);
      *(uint4*)(tin + ((row * CG + cg) * TWI + col) * 16) = v;
    }
  } else if constexpr (INK == HEAD_IN_F32_NCHW) {
    const float* src = (const float*)in + (size_t)img * 3 * h * w;
    for (int i = tid; i < THI * 3 * TWI; i += NT) {
      const int col = i % TWI, c = (i / TWI) % 3, row = i / (3 * TWI);
      const int gy = iy0 + row, gx = ix0 + col;
      float v = 0.f;
      if ((unsigned)gy < (unsigned)h && (unsigned)gx < (unsigned)w) v = src[((size_t)c * h + gy) * w + gx];
      ((float*)tin)[i] = v;  // i == (row * 3 + c) * TWI + col
    }
  } else {
    // u8 frames: float32(u8) / 255 in float32, then (x - mean) / std in float64, then float32 (numpy's promotion in
    // preprocess_pil), through a per-workgroup table of the 3 x 256 possible values as stem_im2col_kernel does
    float* lut = (float*)(lds + C::LUT_OFF);
    const double mean[3] = {0.485, 0.456, 0.406}, sd[3] = {0.229, 0.224, 0.225};
    for (int i = tid; i < 768; i += NT) {
      const int c = i >> 8, v = i & 255;
      lut[i] = (float)(((double)((float)v / 255.0f) - mean[c]) / sd[c]);
    }
    __syncthreads();
    const uint8_t* src = (const uint8_t*)in + (size_t)img * h * w * 3;
    for (int i = tid; i < THI * TWI * 3; i += NT) {
      const int c = i % 3, col = (i / 3) % TWI, row = i / (3 * TWI);
      const int gy = iy0 + row, gx = ix0 + col;
      float v = 0.f;
      if ((unsigned)gy < (unsigned)h && (unsigned)gx < (unsigned)w) v = lut[c * 256 + src[((size_t)gy * w + gx) * 3 + c]];
      ((float*)tin)[(row * 3 + c) * TWI + col] = v;
    }
  }
  __syncthreads();

  // ---- PX pixels x 16 channels per thread ----
  float acc[PX][16];
#pragma unroll
  for (int p = 0; p < PX; ++p)
#pragma unroll
    for (int co = 0; co < 16; ++co) acc[p][co] = 0.f;
  const float* wh = wl + half * 16;
#pragma unroll 1
  for (int ky = 0; ky < K; ++ky) {
    const int row = ty * STRIDE + ky;
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
#pragma unroll
      for (int cg = 0; cg < CG; ++cg) {
        float xv[PX][CV];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
          const int col = (tx + 16 * p) * STRIDE + kx;
          if constexpr (CIN == 3) {
            xv[p][0] = ((const float*)tin)[(row * 3 + cg) * TWI + col];
          } else {
            const uint4 v = *(const uint4*)(tin + ((row * CG + cg) * TWI + col) * 16);
            if constexpr (C::ESZ == 4) {
              xv[p][0] = __uint_as_float(v.x); xv[p][1] = __uint_as_float(v.y);
              xv[p][2] = __uint_as_float(v.z); xv[p][3] = __uint_as_float(v.w);
            } else {
              head_unpack2<DT>(v.x, xv[p][0], xv[p][1]); head_unpack2<DT>(v.y, xv[p][2], xv[p][3]);
              head_unpack2<DT>(v.z, xv[p][4], xv[p][5]); head_unpack2<DT>(v.w, xv[p][6], xv[p][7]);
            }
          }
        }
#pragma unroll
        for (int c = 0; c < CV; ++c) {
          const float4* wp = (const float4*)(wh + ((ky * K + kx) * CIN + cg * CV + c) * COUT);
          const float4 w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3];
          const float wv[16] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w,
                                w2.x, w2.y, w2.z, w2.w, w3.x, w3.y, w3.z, w3.w};
#pragma unroll
          for (int p = 0; p < PX; ++p)
#pragma unroll
            for (int co = 0; co < 16; ++co) acc[p][co] = fmaf(xv[p][c], wv[co], acc[p][co]);
        }
      }
    }
  }

  // ---- BatchNorm + ReLU, NHWC stores ----
  const int oy = oy0 + ty;
  if (oy >= ho) return;
  float sc[16], sh[16];
#pragma unroll
  for (int co = 0; co < 16; ++co) {
    sc[co] = scale[half * 16 + co];
    sh[co] = shift[half * 16 + co];
  }
  constexpr int OSZ = C::ACT_F32 ? 4 : 2;
#pragma unroll
  for (int p = 0; p < PX; ++p) {
    const int ox = ox0 + tx + 16 * p;
    if (ox >= wo) continue;
    char* dst = (char*)out + (((size_t)img * ho + oy) * wo + ox) * ((size_t)out_cs * OSZ);
    float y[16];
#pragma unroll
    for (int co = 0; co < 16; ++co) y[co] = fmaxf(acc[p][co] * sc[co] + sh[co], 0.f);
    if constexpr (C::ACT_F32) {
      float4* d = (float4*)(dst + half * 64);
#pragma unroll
      for (int q = 0; q < 4; ++q) d[q] = make_float4(y[4 * q], y[4 * q + 1], y[4 * q + 2], y[4 * q + 3]);
    } else {
      uint4* d = (uint4*)(dst + half * 32);
#pragma unroll
      for (int q = 0; q < 2; ++q)
        d[q] = make_uint4(head_pack2<DT>(y[8 * q], y[8 * q + 1]), head_pack2<DT>(y[8 * q + 2], y[8 * q + 3]),
                          head_pack2<DT>(y[8 * q + 4], y[8 * q + 5]), head_pack2<DT>(y[8 * q + 6], y[8 * q + 7]));
    }
    // padding channels [COUT, out_cs): zeros, 16 at a time, shared out among the halves
    for (int c = COUT + half * 16; c < out_cs; c += 16 * C::NH) {
      uint4* z = (uint4*)(dst + (size_t)c * OSZ);
#pragma unroll
      for (int q = 0; q < OSZ; ++q) z[q] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

template <int K, int CIN, int COUT, int STRIDE, int TY, int DT, int INK>
hipError_t launch_head(const void* in, int n, int h, int w, const float* wt, const float* scale, const float* shift,
                       void* out, int out_cs, hipStream_t st) {
  using C = HeadCfg<K, CIN, COUT, STRIDE, TY, DT, INK>;
  const int ho = (h - 1) / STRIDE + 1, wo = (w - 1) / STRIDE + 1;  // pad = K / 2
  if (out_cs < COUT || out_cs % 16 || n > 65535 || (ho + C::THO - 1) / C::THO > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((wo + C::TWO - 1) / C::TWO), (unsigned)((ho + C::THO - 1) / C::THO), (unsigned)n);
  hipLaunchKernelGGL((drn_head_kernel<K, CIN, COUT, STRIDE, TY, DT, INK>), grid, dim3(C::NT), 0, st, in, h, w, wt,
                     scale, shift, out, ho, wo, out_cs);
  return hipGetLastError();
}

// tile heights: the largest whose weights + input tile fit the 64 KB of static LDS
template <int DT>
hipError_t launch_head_dt(int layer, const void* in, int x_u8, int n, int h, int w, const float* wt, const float* scale,
                          const float* shift, void* out, int out_cs, hipStream_t st) {
  constexpr bool F32 = DT == NST_DT_F32;
  if (layer == 0)
    return x_u8 ? launch_head<7, 3, 16, 1, 16, DT, HEAD_IN_U8_NHWC>(in, n, h, w, wt, scale, shift, out, out_cs, st)
                : launch_head<7, 3, 16, 1, 16, DT, HEAD_IN_F32_NCHW>(in, n, h, w, wt, scale, shift, out, out_cs, st);
  if (layer == 1)
    return launch_head<3, 16, 16, 1, F32 ? 8 : 16, DT, HEAD_IN_ACT>(in, n, h, w, wt, scale, shift, out, out_cs, st);
  if (layer == 2)
    return launch_head<3, 16, 32, 2, F32 ? 4 : 8, DT, HEAD_IN_ACT>(in, n, h, w, wt, scale, shift, out, out_cs, st);
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_seg_drn_head(int layer, int dtype, const void* in, int x_u8, int n, int h, int w, const float* wt,
                               const float* scale, const float* shift, void* out, int out_cs, hipStream_t st) {
  if (n <= 0 || h <= 0 || w <= 0) return hipErrorInvalidValue;
  if (dtype == NST_DT_F32) return launch_head_dt<NST_DT_F32>(layer, in, x_u8, n, h, w, wt, scale, shift, out, out_cs, st);
  if (dtype == NST_DT_BF16) return launch_head_dt<NST_DT_BF16>(layer, in, x_u8, n, h, w, wt, scale, shift, out, out_cs, st);
  if (dtype == NST_DT_F16) return launch_head_dt<NST_DT_F16>(layer, in, x_u8, n, h, w, wt, scale, shift, out, out_cs, st);
  return hipErrorInvalidValue;
}

}  // namespace nst
