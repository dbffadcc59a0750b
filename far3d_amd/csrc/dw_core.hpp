// What the depthwise family shares: dwconv.hip (the window kernel behind far3d_dwconv3x3_nhwc and far3d_dwconv3x3_act_nhwc), dwsep.hip
// (the fused depthwise + pointwise layer) and, for the vector I/O alone, the eSE kernels of norm.hip.
//
// Arithmetic contract of a depthwise output element, the same in every kernel of the family:
//   * fp32, s = 0, then s = fmaf(x, w, s) over the nine taps in the fixed order (ky, kx) = (0,0) (0,1) (0,2) (1,0) ... (2,2), a padding
//     tap as x = 0 -- explicit fmaf calls, so the contraction is pinned in the source.  The nine statements stay written out in the two
//     kernels: a function template over their register arrays changed the machine code of both (profiles/dw_core/README.md);
//   * the bias is ONE fp32 add after the taps, and no add at all when the bias pointer is NULL;
//   * the activation, DW_ACT below (Swish with full-precision expf and division);
//   * rounding to storage, DwIo<T>::pack: fp32 as is, bf16 round-to-nearest-even, pair hi = bf16(v), lo = bf16(v - hi).
// So the bits of an element depend on its own window, weights and bias only -- never on N, the lane's run, the number of weight sets or
// the launch's other pixels -- and the MFMA operand of dwsep_kernel holds bit for bit what the window kernel stores.
#pragma once
#include <initializer_list>
#include <type_traits>
#include "common.hpp"
#include "far3d_hip.h"

namespace {

// activation codes of the C ABI (far3d_conv2d_nhwc's)
constexpr int DW_ACT_NONE = 0, DW_ACT_RELU = 1, DW_ACT_SWISH = 2;
// a statement, not a function: as a function the ladder changed every dwsep_kernel instantiation
#define DW_ACT(s_, act_)                                  \
  if ((act_) == DW_ACT_RELU) (s_) = fmaxf((s_), 0.f);     \
  else if ((act_) == DW_ACT_SWISH) (s_) = swish_f32((s_))

// output pixels per lane of the window kernel: stride 1 loads RUN + 2 input columns for RUN outputs, stride 2 loads 2 RUN + 1
template <int S> struct DwRun { static constexpr int v = S == 1 ? 8 : 4; };

// One 16-byte channel vector of a pixel (8 bf16 / 4 fp32; pair storage: 8 logical channels = 16 bytes of hi + 16 bytes of lo, p -> the hi
// halves of one 32-channel block, the lo halves 32 elements on).  Raw: the bytes as stored, so that a conversion can wait until every
// load is issued (ldraw, cvt) and a value can be rounded to storage without a store (pack; st stores it, round converts it back).  The
// pair load and the two `round` are written out although cvt(ldraw(p)) and cvt(pack(v)) say the same: those forms changed the register
// allocation of the pair kernels of dwconv.hip and dwsep.hip and the pooling eSE kernels of norm.hip.
template <typename T> struct DwIo;
template <> struct DwIo<float> {
  static constexpr int VEC = 4;
  static __device__ __forceinline__ void ld(const float* p, float (&v)[4]) {
    const float4 r = *reinterpret_cast<const float4*>(p);
    v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
  }
  static __device__ __forceinline__ void st(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
__device__ __forceinline__ void unpack8(const uint4& r, float (&v)[8]) {
  v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xffff0000u);
  v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xffff0000u);
  v[4] = __uint_as_float(r.z << 16); v[5] = __uint_as_float(r.z & 0xffff0000u);
  v[6] = __uint_as_float(r.w << 16); v[7] = __uint_as_float(r.w & 0xffff0000u);
}
template <> struct DwIo<bf16_t> {
  static constexpr int VEC = 8;
  struct Raw { uint4 a; };
  static __device__ __forceinline__ Raw ldraw(const bf16_t* p) { Raw r; r.a = *reinterpret_cast<const uint4*>(p); return r; }
  static __device__ __forceinline__ void cvt(const Raw& q, float (&v)[8]) { unpack8(q.a, v); }
  static __device__ __forceinline__ void ld(const bf16_t* p, float (&v)[8]) { cvt(ldraw(p), v); }
  static __device__ __forceinline__ Raw pack(const float (&v)[8]) {
    Raw r;
    r.a = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
    return r;
  }
  static __device__ __forceinline__ void st(bf16_t* p, const float (&v)[8]) { *reinterpret_cast<uint4*>(p) = pack(v).a; }
  static __device__ __forceinline__ void round(float (&v)[8]) {      // what a store followed by a load returns
#pragma unroll
    for (int e = 0; e < 8; e += 2) { const uint32_t q = pack_bf16x2(v[e], v[e + 1]); v[e] = __uint_as_float(q << 16); v[e + 1] = __uint_as_float(q & 0xffff0000u); }
  }
};
template <> struct DwIo<pair_t> {
  static constexpr int VEC = 8;
  struct Raw { uint4 h, l; };
  static __device__ __forceinline__ Raw ldraw(const pair_t* p) {
    Raw r;
    r.h = *reinterpret_cast<const uint4*>(p);
    r.l = *reinterpret_cast<const uint4*>(p + 32);
    return r;
  }
  static __device__ __forceinline__ void join(const uint4& h, const uint4& l, float (&v)[8]) {
    float lo[8];
    unpack8(h, v);
    unpack8(l, lo);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += lo[j];      // exact: hi and lo are pieces of one fp32 mantissa
  }
  static __device__ __forceinline__ void cvt(const Raw& q, float (&v)[8]) { join(q.h, q.l, v); }
  static __device__ __forceinline__ void ld(const pair_t* p, float (&v)[8]) {
    join(*reinterpret_cast<const uint4*>(p), *reinterpret_cast<const uint4*>(p + 32), v);
  }
  static __device__ __forceinline__ Raw pack(const float (&v)[8]) {
    uint2 h0, l0, h1, l1;
    split4f(v[0], v[1], v[2], v[3], h0, l0);
    split4f(v[4], v[5], v[6], v[7], h1, l1);
    Raw r;
    r.h = make_uint4(h0.x, h0.y, h1.x, h1.y);
    r.l = make_uint4(l0.x, l0.y, l1.x, l1.y);
    return r;
  }
  static __device__ __forceinline__ void st(pair_t* p, const float (&v)[8]) {
    const Raw r = pack(v);
    *reinterpret_cast<uint4*>(p) = r.h;
    *reinterpret_cast<uint4*>(p + 32) = r.l;
  }
  static __device__ __forceinline__ void round(float (&v)[8]) {
    const Raw r = pack(v);
    const uint32_t hh[4] = {r.h.x, r.h.y, r.h.z, r.h.w}, ll[4] = {r.l.x, r.l.y, r.l.z, r.l.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[2 * e] = __uint_as_float(hh[e] << 16) + __uint_as_float(ll[e] << 16);
      v[2 * e + 1] = __uint_as_float(hh[e] & 0xffff0000u) + __uint_as_float(ll[e] & 0xffff0000u);
    }
  }
};

// ---- host side: the operand rules far3d_dwconv3x3_nhwc, far3d_dwconv3x3_act_nhwc and far3d_dwsep_conv_nhwc share, each taking the
// entry's name.  An entry calls them in its own order: the order decides which message a call with two faults gets.
inline int dw_check_stride(const char* who, int stride) {
  FAR3D_CHECK_ARG(stride == 1 || stride == 2, "%s: stride %d (1 or 2 only)", who, stride);
  return FAR3D_OK;
}
inline bool dw_act_ok(int act) { return act >= DW_ACT_NONE && act <= DW_ACT_SWISH; }
inline int dw_check_out_size(const char* who, int H, int W, int stride, int Ho, int Wo) {
  const int eh = (H - 1) / stride + 1, ew = (W - 1) / stride + 1;
  FAR3D_CHECK_ARG(Ho == eh && Wo == ew, "%s: output %dx%d != %dx%d (3x3, pad 1, stride %d of %dx%d)", who, Ho, Wo, eh, ew, stride, H, W);
  return FAR3D_OK;
}
// Pixel and image strides of x (C logical channels) and y (Cy), cs stored elements per logical channel.  one_count: the message of the
// entry whose two maps have the same channels names one count.
inline int dw_check_strides(const char* who, bool one_count, int cs, int N, int H, int W, int C, int ldx, long xs, int Ho, int Wo, int Cy,
                            int ldy, long ys) {
  const bool fits = ldx >= C * cs && ldy >= Cy * cs;
  if (one_count) FAR3D_CHECK_ARG(fits, "%s: pixel strides %d / %d below the %d stored channels", who, ldx, ldy, C * cs);
  FAR3D_CHECK_ARG(fits, "%s: pixel strides %d / %d below the %d / %d stored channels", who, ldx, ldy, C * cs, Cy * cs);
  FAR3D_CHECK_ARG(N == 1 || (xs >= (long)H * W * ldx - (ldx - C * cs) && ys >= (long)Ho * Wo * ldy - (ldy - Cy * cs)),
                  "%s: image strides below one image", who);
  return FAR3D_OK;
}
// every stride a multiple of `al` elements (16 bytes) and every pointer (NULL included) of 16 bytes
inline bool dw_aligned16(int al, int ldx, int ldy, long xs, long ys, std::initializer_list<const void*> ptrs) {
  bool ok = ldx % al == 0 && ldy % al == 0 && xs % al == 0 && ys % al == 0;
  for (const void* p : ptrs) ok = ok && ((uintptr_t)p % 16) == 0;
  return ok;
}
inline int dw_check_launch_size(const char* who, long blocks) {
  FAR3D_CHECK_ARG(blocks <= 0x7fffffffL, "%s: launch too large (%ld workgroups)", who, blocks);
  return FAR3D_OK;
}

}  // namespace
