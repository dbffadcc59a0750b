// The wave-wide sum and the LayerNorm row of the normalisation family: included by norm.hip, rowchain.hip and glue.hip.
//
// ARITHMETIC CONTRACT of a LayerNorm row of C channels (a multiple of 4, at most 256 * MAXV), all fp32.  One wave owns the row; lane l
// holds the float4 pieces i < MAXV at channels (l + 64 i) * 4 .. + 3, zeros past C.
//   first pass    s = the lane's sum over its pieces, in order, of (x + y) + (z + w);  mean = wave_sum(s) / C, where wave_sum is the
//                 butterfly v += shfl_xor(v, o), o = 32, 16, 8, 4, 2, 1: every lane ends with the same bits
//   second pass   q = the lane's sum over its pieces below C of (a*a + b*b) + (d*d + e*e), a .. e the four channels minus the mean;
//                 rstd = 1 / sqrtf(wave_sum(q) / C + eps): the centred, biased variance; eps enters here and nowhere else
//   apply         (v - mean) * rstd * g + b per channel
// layernorm_kernel<MAXV> (norm.hip) is this for any C; a row chain's LayerNorm (rowchain.hip) is MAXV = 1, C = 256 on a row in LDS;
// row_affine_ln_kernel takes mean and rstd and has its own apply.  cam_embed_chain_kernel (glue.hip) holds one channel per thread and
// reduces block-wide, four wave sums through LDS: it shares wave_sum only.
#pragma once
#include "common.hpp"

__device__ __forceinline__ float wave_sum(float v) {      // over the 64 lanes; every lane gets it
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float ln_lane_sum(const float4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float ln_lane_squares(const float4 v, float mean) {
  const float a = v.x - mean, b = v.y - mean, d = v.z - mean, e = v.w - mean;
  return (a * a + b * b) + (d * d + e * e);
}

__device__ __forceinline__ float ln_mean(float s, int C) { return wave_sum(s) / C; }                                  // s: the lane sum
__device__ __forceinline__ float ln_rstd(float q, int C, float eps) { return 1.f / sqrtf(wave_sum(q) / C + eps); }      // q: the lane squares

__device__ __forceinline__ float4 ln_apply(const float4& v, float mean, float rstd, const float4& g, const float4& b) {
  float4 o;
  o.x = (v.x - mean) * rstd * g.x + b.x;
  o.y = (v.y - mean) * rstd * g.y + b.y;
  o.z = (v.z - mean) * rstd * g.z + b.z;
  o.w = (v.w - mean) * rstd * g.w + b.w;
  return o;
}
