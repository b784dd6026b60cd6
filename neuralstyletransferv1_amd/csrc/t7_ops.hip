// t7_ops.hip — the kernels the Torch7 fast-style nets (NST_ARCH_TORCH7_IN / _BN) add to the conv program: the
// shaved residual join of their valid-conv trunk, the constant norm table of SpatialBatchNormalization, and the
// Tanh / MulConstant / de-mean / clip / truncate tail (pipeline.py:445-478).  fp32 arithmetic op by op in the
// reference's order; the library is built with -ffp-contract=off.
#include "nst_internal.h"
#include "nst_hip.h"
#include "conv_impl.h"

namespace nst {

// ---------------------------------------------------------------------------------------
// nn.Sequential(nn.ConcatTable(branch, nn.ShaveImage(s)), nn.CAddTable): out = IN(y) + shave(r).  One thread per
// (pixel, 16-byte channel vector) of the output map; the arithmetic and roundings of residual_kernel (nst_ops.hip).
template <typename T>
__global__ __launch_bounds__(256) void residual_shave_kernel(const T* __restrict__ y, const float2* __restrict__ ys,
                                                             const T* __restrict__ r, const float2* __restrict__ rs,
                                                             int r_relu, T* __restrict__ out, int oh, int ow, int shave,
                                                             int c) {
  constexpr int CPC = 16 / (int)sizeof(T);
  const int cv_n = c / CPC;
  const int n = blockIdx.y;
  const size_t item = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t items = (size_t)oh * ow * cv_n;
  if (item >= items) return;
  const int cv = (int)(item % cv_n);
  const int px = (int)(item / cv_n);
  const int oy = px / ow, ox = px - oy * ow;
  const int rw = ow + 2 * shave, rh = oh + 2 * shave;
  const int ch0 = cv * CPC;
  const uint4 va = *(const uint4*)(y + ((size_t)n * oh * ow + px) * c + ch0);
  const uint4 vb = *(const uint4*)(r + (((size_t)n * rh + oy + shave) * rw + ox + shave) * c + ch0);
  float vy[CPC], vr[CPC];
  if constexpr (sizeof(T) == 2) {
    const uint32_t wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      vy[2 * j] = lo16<T>(wa[j]);
      vy[2 * j + 1] = hi16<T>(wa[j]);
      vr[2 * j] = lo16<T>(wb[j]);
      vr[2 * j + 1] = hi16<T>(wb[j]);
    }
  } else {
    vy[0] = __uint_as_float(va.x); vy[1] = __uint_as_float(va.y);
    vy[2] = __uint_as_float(va.z); vy[3] = __uint_as_float(va.w);
    vr[0] = __uint_as_float(vb.x); vr[1] = __uint_as_float(vb.y);
    vr[2] = __uint_as_float(vb.z); vr[3] = __uint_as_float(vb.w);
  }
  float o[CPC];
#pragma unroll
  for (int j = 0; j < CPC; ++j) {
    const float2 a = ys[(size_t)n * c + ch0 + j];
    float rr = vr[j];
    if (rs) {
      const float2 b = rs[(size_t)n * c + ch0 + j];
      // as a normalising fill stages it (conv_impl.h norm_chunk): one fma, rounded to T
      if constexpr (sizeof(T) == 2)
        rr = lo16<T>(pack16<T>(__builtin_fmaf(rr, b.x, b.y), 0.f));
      else
        rr = rr * b.x + b.y;
      if (r_relu) rr = fmaxf(rr, 0.f);
    }
    float v = vy[j] * a.x + a.y;
    o[j] = rr + v;
  }
  T* dst = out + ((size_t)n * oh * ow + px) * c + ch0;
  if constexpr (sizeof(T) == 2) {
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = pack16<T>(o[2 * j], o[2 * j + 1]);
    *(uint4*)dst = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    *(float4*)dst = make_float4(o[0], o[1], o[2], o[3]);
  }
}

hipError_t launch_residual_shave(int dtype, const void* y, const float2* ys, const void* r, const float2* rs, int r_relu,
                                 void* out, int n, int oh, int ow, int shave, int c, hipStream_t st) {
  const int cpc = f32_storage(dtype) ? 4 : 8;
  if (c % cpc != 0 || oh <= 0 || ow <= 0 || shave < 0 || n <= 0 || n > 65535) return hipErrorInvalidValue;
  const size_t items = (size_t)oh * ow * (c / cpc);
  const size_t blocks = (items + 255) / 256;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks, (unsigned)n), block(256);
  if (dtype == NST_DT_BF16)
    hipLaunchKernelGGL(residual_shave_kernel<__bf16>, grid, block, 0, st, (const __bf16*)y, ys, (const __bf16*)r, rs,
                       r_relu, (__bf16*)out, oh, ow, shave, c);
  else if (dtype == NST_DT_F16)
    hipLaunchKernelGGL(residual_shave_kernel<_Float16>, grid, block, 0, st, (const _Float16*)y, ys, (const _Float16*)r,
                       rs, r_relu, (_Float16*)out, oh, ow, shave, c);
  else
    hipLaunchKernelGGL(residual_shave_kernel<float>, grid, block, 0, st, (const float*)y, ys, (const float*)r, rs,
                       r_relu, (float*)out, oh, ow, shave, c);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void norm_table_fill_kernel(const float2* __restrict__ tab, int total, int c,
                                                              float2* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) out[i] = tab[i % c];
}

hipError_t launch_norm_table_fill(const float2* tab, int n, int c, float2* out, hipStream_t st) {
  if (n <= 0 || c <= 0 || (size_t)n * c > 0x7fffffffu) return hipErrorInvalidValue;
  const int total = n * c;
  hipLaunchKernelGGL(norm_table_fill_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, tab, total, c, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// nn.Tanh, nn.MulConstant, then pipeline.py:466-474: out[..., c] += mean[c] (float32), np.clip(out, 0, 255),
// .astype(np.uint8) (truncation), COLOR_BGR2RGB; mode 1 divides the byte by 255 as to_tensor does (:1443).
__global__ __launch_bounds__(256) void t7_tail_kernel(const float* __restrict__ t, int n, int h, int w, float mul,
                                                      int mode, void* __restrict__ out) {
  const size_t plane = (size_t)h * w;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n * plane) return;
  const size_t b = i / plane, px = i - b * plane;
  const float* tb = t + b * 3 * plane + px;
  const float mean[3] = {103.939f, 116.779f, 123.68f};
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = tanhf(tb[c * plane]) * mul;
  if (mode == 0) {
    float* o = (float*)out + b * 3 * plane + px;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = v[c];
    return;
  }
  uint8_t k[3];  // RGB
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float f = v[c] + mean[c];
    f = fminf(fmaxf(f, 0.f), 255.f);
    k[2 - c] = (uint8_t)f;
  }
  if (mode == 1) {
    float* o = (float*)out + b * 3 * plane + px;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = (float)k[c] / 255.0f;
  } else {
    uint8_t* o = (uint8_t*)out + i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = k[c];
  }
}

hipError_t launch_t7_tail(const float* t, int n, int h, int w, float mul, int mode, void* out, hipStream_t st) {
  const size_t total = (size_t)n * h * w;
  if (n <= 0 || h <= 0 || w <= 0 || mode < 0 || mode > 2 || (total + 255) / 256 > 0x7fffffffu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(t7_tail_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, t, n, h, w, mul, mode, out);
  return hipGetLastError();
}

}  // namespace nst
