// Fused depthwise-separable layer on NHWC maps: y = act2( W_pw . round_storage( act1( dw3x3(x; w9) + b1 ) ) + b2 ) in ONE launch -- the
// `dw_conv3x3` + `pw_conv1x1` layers of VoVNet's depthwise specs (ref models/backbones/vovnet.py:100-121) and mmcv's
// DepthwiseSeparableConvModule of the light YOLOX towers (ref models/dense_heads/yolox_head.py:197-219).  The two-launch form
// (far3d_dwconv3x3[_act]_nhwc into a scratch map, far3d_conv2d_nhwc from there) writes and re-reads a map only the second launch reads.
//
// Mapping.  The B fragment of v_mfma_f32_32x32x16_bf16 is, per lane, B[k = 8(l>>5) + j][col = l&31], j = 0..7: with pixels as columns
// and channels as k that is 8 consecutive channels of one pixel -- the 16-byte channel vector a lane of dwconv.hip owns.  So a wave takes
// 32 consecutive output pixels (of the flattened N*Ho*Wo index; lane l: pixel l&31, channel octet l>>5 of each 16-channel step), computes
// the depthwise result of its octet in registers, rounds it to the storage type and hands it to the MFMA as is: no HBM, no LDS transpose.
// The pointwise weights are the A operand (rows = output channels, as in igemm_kernels.hpp), staged per 32-channel K chunk through LDS
// (rows padded by 16 B: stride 80 B / 144 B, conflict-free 16-lane ds_read_b128 groups) and shared by the workgroup's four waves; the
// next chunk's global loads are in flight during the depthwise arithmetic.  A lane ends up with 4 consecutive output channels of its pixel
// per accumulator quad -> 8-byte stores (pair: 8 bytes of hi + 8 of lo).
//
// Depthwise half: the arithmetic contract of dw_core.hpp -- the nine pinned fmaf in its tap order (padding taps as x = 0), one fp32 add of
// the bias (none when b1 is NULL), DW_ACT, then DwIo<T>::pack, the rounding of the window kernel's store -- so the MFMA operand holds bit
// for bit what far3d_dwconv3x3_act_nhwc stores.  Pair storage: the three products hi.hi, hi.lo, lo.hi of the split kernels.  The vector
// load, the activation and the rounding are dw_core.hpp's; the tap chain is written out here as in dwconv.hip.
#include "dw_core.hpp"

namespace {

typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 ds_bf16x8_t;
typedef __attribute__((__vector_size__(16 * sizeof(float)))) float ds_f32x16_t;
typedef uint32_t ds_u32x4_t __attribute__((ext_vector_type(4)));

constexpr int DS_THREADS = 256, DS_WAVES = 4, DS_PIX = 32 * DS_WAVES;     // 128 output pixels per workgroup
constexpr int DS_BK = 32;                                                 // channels per staged K chunk (two MFMA k steps)

template <typename T> struct DsT;
template <> struct DsT<bf16_t> { static constexpr int CS = 1, ROW = DS_BK + 8; };          // LDS row: 32 bf16 + 16 B pad
template <> struct DsT<pair_t> { static constexpr int CS = 2, ROW = 2 * DS_BK + 8; };      // [32 hi | 32 lo] + 16 B pad

__device__ __forceinline__ void ds_mma(ds_f32x16_t& acc, const ds_u32x4_t& a, const ds_u32x4_t& b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(ds_bf16x8_t, a), __builtin_bit_cast(ds_bf16x8_t, b), acc, 0, 0, 0);
}

// NB: 32-row blocks of output channels the workgroup computes (Cout <= 32 NB; the packed weights carry >= 256 zero rows past Cout, so
// the rows of a partly used NB are readable, and their results are never stored)
template <typename T, int NB>
__global__ __launch_bounds__(DS_THREADS) void dwsep_kernel(const T* __restrict__ x, const float* __restrict__ w9, const float* __restrict__ b1,
                                                           const bf16_t* __restrict__ wp, const float* __restrict__ b2, T* __restrict__ y,
                                                           long npix, int H, int W, int C, int ldx, long xs, int Ho, int Wo, int Cout, int ldy,
                                                           long ys, int stride, int act1, int act2) {
  constexpr int CS = DsT<T>::CS, ROW = DsT<T>::ROW;
  constexpr int ROWV = DS_BK * CS / 8;                       // 16-byte pieces per weight row of a chunk
  constexpr int NLD = (NB * 32 * ROWV + DS_THREADS - 1) / DS_THREADS;
  __shared__ __attribute__((aligned(16))) bf16_t lds[NB * 32 * ROW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const long p = (long)blockIdx.x * DS_PIX + wave * 32 + r;
  const bool pv = p < npix;
  int ox = 0, oy = 0;
  long n = 0;
  if (pv) {
    ox = (int)(p % Wo);
    const long q = p / Wo;
    oy = (int)(q % Ho);
    n = q / Ho;
  }
  // the window: a pointer to its (possibly outside) top-left tap, and one validity bit per tap (pad 1 / a lane past the last pixel)
  const int iy0 = oy * stride - 1, ix0 = ox * stride - 1;
  const T* xw = x + n * xs + ((long)iy0 * W + ix0) * ldx;
  unsigned tvm = 0;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
      if (pv && iy0 + ky >= 0 && iy0 + ky < H && ix0 + kx >= 0 && ix0 + kx < W) tvm |= 1u << (ky * 3 + kx);

  ds_f32x16_t acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;

  const long wrow = (long)C * CS;                            // elements per packed weight row (Cin padded to 32 = C)
  constexpr int NPIECE = NB * 32 * ROWV;                    // 16-byte pieces of a chunk; a multiple of the workgroup but for NB = 1
  // the chunk in flight: up to 8 pieces per thread in named registers (an indexed array of them ends up in scratch memory)
  uint4 st0, st1, st2, st3, st4, st5, st6, st7;
#define DS_FETCH1(i_, kc_)                                                                                                         \
  if constexpr (NLD > i_) {                                                                                                        \
    const int e = tid + i_ * DS_THREADS;                                                                                           \
    if (NPIECE % DS_THREADS == 0 || e < NPIECE)                                                                                    \
      st##i_ = *reinterpret_cast<const uint4*>(wp + (long)(e / ROWV) * wrow + (long)(kc_) * DS_BK * CS + (e % ROWV) * 8);          \
  }
#define DS_COMMIT1(i_)                                                                                                             \
  if constexpr (NLD > i_) {                                                                                                        \
    const int e = tid + i_ * DS_THREADS;                                                                                           \
    if (NPIECE % DS_THREADS == 0 || e < NPIECE) *reinterpret_cast<uint4*>(lds + (e / ROWV) * ROW + (e % ROWV) * 8) = st##i_;       \
  }
#define DS_FETCH(kc_)                                                                                                              \
  DS_FETCH1(0, kc_) DS_FETCH1(1, kc_) DS_FETCH1(2, kc_) DS_FETCH1(3, kc_) DS_FETCH1(4, kc_) DS_FETCH1(5, kc_) DS_FETCH1(6, kc_) DS_FETCH1(7, kc_)
#define DS_COMMIT() DS_COMMIT1(0) DS_COMMIT1(1) DS_COMMIT1(2) DS_COMMIT1(3) DS_COMMIT1(4) DS_COMMIT1(5) DS_COMMIT1(6) DS_COMMIT1(7)
  static_assert(NLD <= 8, "a chunk is at most 8 pieces per thread");

  const int nk = C / DS_BK;
  DS_FETCH(0)
  for (int kc = 0; kc < nk; ++kc) {
    __syncthreads();                                         // every wave has read the previous chunk
    DS_COMMIT()
    __syncthreads();
    if (kc + 1 < nk) { DS_FETCH(kc + 1) }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int c = kc * DS_BK + kk * 16 + h * 8;            // this lane's channel octet
      float s[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] = 0.f;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        float xv[8];
        if (tvm & (1u << t)) {
          DwIo<T>::ld(xw + ((long)(t / 3) * W + (t % 3)) * ldx + chan_off<T>(c), xv);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) xv[j] = 0.f;
        }
        const float4 w0 = *reinterpret_cast<const float4*>(w9 + (long)t * C + c);
        const float4 w1 = *reinterpret_cast<const float4*>(w9 + (long)t * C + c + 4);
        s[0] = fmaf(xv[0], w0.x, s[0]); s[1] = fmaf(xv[1], w0.y, s[1]); s[2] = fmaf(xv[2], w0.z, s[2]); s[3] = fmaf(xv[3], w0.w, s[3]);
        s[4] = fmaf(xv[4], w1.x, s[4]); s[5] = fmaf(xv[5], w1.y, s[5]); s[6] = fmaf(xv[6], w1.z, s[6]); s[7] = fmaf(xv[7], w1.w, s[7]);
      }
      if (b1) {
        const float4 q0 = *reinterpret_cast<const float4*>(b1 + c), q1 = *reinterpret_cast<const float4*>(b1 + c + 4);
        s[0] = s[0] + q0.x; s[1] = s[1] + q0.y; s[2] = s[2] + q0.z; s[3] = s[3] + q0.w;
        s[4] = s[4] + q1.x; s[5] = s[5] + q1.y; s[6] = s[6] + q1.z; s[7] = s[7] + q1.w;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) { DW_ACT(s[j], act1); }
      // round to storage with the statement of DwIo<T>::st: the MFMA operand is what the two-launch path writes to its scratch map
      const typename DwIo<T>::Raw q = DwIo<T>::pack(s);
      ds_u32x4_t bh, bl;
      if constexpr (CS == 2) {
        bh = ds_u32x4_t{q.h.x, q.h.y, q.h.z, q.h.w};
        bl = ds_u32x4_t{q.l.x, q.l.y, q.l.z, q.l.w};
      } else {
        bh = ds_u32x4_t{q.a.x, q.a.y, q.a.z, q.a.w};
      }
      const bf16_t* arow = lds + r * ROW + kk * 16 + h * 8;   // A[row r][k = 8h + j] of this k step
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const ds_u32x4_t ah = *reinterpret_cast<const ds_u32x4_t*>(arow + b * 32 * ROW);
        if constexpr (CS == 2) {
          const ds_u32x4_t al = *reinterpret_cast<const ds_u32x4_t*>(arow + b * 32 * ROW + 32);
          ds_mma(acc[b], al, bh);          // the small terms first
          ds_mma(acc[b], ah, bl);
        }
        ds_mma(acc[b], ah, bh);
      }
    }
  }

#undef DS_FETCH
#undef DS_COMMIT
#undef DS_FETCH1
#undef DS_COMMIT1
  if (!pv) return;
  T* yp = y + n * ys + ((long)oy * Wo + ox) * ldy;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b * 32 >= Cout) break;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int o = b * 32 + g * 8 + h * 4;                  // C/D: row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), col = lane & 31
      float v[4] = {acc[b][g * 4], acc[b][g * 4 + 1], acc[b][g * 4 + 2], acc[b][g * 4 + 3]};
      if (b2) {
        const float4 q = *reinterpret_cast<const float4*>(b2 + o);
        v[0] += q.x; v[1] += q.y; v[2] += q.z; v[3] += q.w;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) { DW_ACT(v[e], act2); }
      store4(yp + chan_off<T>(o), make_float4(v[0], v[1], v[2], v[3]));
    }
  }
}

template <typename T, int NB>
void dwsep_launch_nb(const void* x, const float* w9, const float* b1, const void* wp, const float* b2, void* y, long npix, long blocks, int H,
                     int W, int C, int ldx, long xs, int Ho, int Wo, int Cout, int ldy, long ys, int stride, int act1, int act2, hipStream_t st) {
  hipLaunchKernelGGL((dwsep_kernel<T, NB>), dim3((unsigned)blocks), dim3(DS_THREADS), 0, st, (const T*)x, w9, b1, (const bf16_t*)wp, b2, (T*)y,
                     npix, H, W, C, ldx, xs, Ho, Wo, Cout, ldy, ys, stride, act1, act2);
}

template <typename T>
void dwsep_launch(const void* x, const float* w9, const float* b1, const void* wp, const float* b2, void* y, long npix, long blocks, int H, int W,
                  int C, int ldx, long xs, int Ho, int Wo, int Cout, int ldy, long ys, int stride, int act1, int act2, hipStream_t st) {
  if (Cout <= 32)
    dwsep_launch_nb<T, 1>(x, w9, b1, wp, b2, y, npix, blocks, H, W, C, ldx, xs, Ho, Wo, Cout, ldy, ys, stride, act1, act2, st);
  else if (Cout <= 64)
    dwsep_launch_nb<T, 2>(x, w9, b1, wp, b2, y, npix, blocks, H, W, C, ldx, xs, Ho, Wo, Cout, ldy, ys, stride, act1, act2, st);
  else if (Cout <= 128)
    dwsep_launch_nb<T, 4>(x, w9, b1, wp, b2, y, npix, blocks, H, W, C, ldx, xs, Ho, Wo, Cout, ldy, ys, stride, act1, act2, st);
  else
    dwsep_launch_nb<T, 8>(x, w9, b1, wp, b2, y, npix, blocks, H, W, C, ldx, xs, Ho, Wo, Cout, ldy, ys, stride, act1, act2, st);
}

}  // namespace

extern "C" int far3d_dwsep_conv_nhwc(const void* x, int dt, const float* w9, const float* b1, int act1, const void* w_pw, int w_dt,
                                     const float* b2, int act2, void* y, int N, int H, int W, int C, int ldx, long x_img_stride, int Ho,
                                     int Wo, int Cout, int ldy, long y_img_stride, int stride, void* stream) {
  const char* who = "far3d_dwsep_conv_nhwc";      // for the checks of dw_core.hpp; the entry's own are spelled out
  FAR3D_CHECK_ARG(x && w9 && w_pw && y, "far3d_dwsep_conv_nhwc: null pointer argument");
  FAR3D_CHECK_ARG((dt == FAR3D_DT_BF16 && w_dt == FAR3D_DT_BF16) || (dt == FAR3D_DT_BF16_PAIR && w_dt == FAR3D_DT_F32_BF16X3),
                  "far3d_dwsep_conv_nhwc: storage %d with weights %d (bf16 with bf16 weights, or pair storage with split weights)", dt, w_dt);
  if (const int rc = dw_check_stride(who, stride)) return rc;
  FAR3D_CHECK_ARG(dw_act_ok(act1) && dw_act_ok(act2), "far3d_dwsep_conv_nhwc: act %d / %d (0 none, 1 ReLU, 2 Swish)", act1, act2);
  FAR3D_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && Cout > 0, "far3d_dwsep_conv_nhwc: bad sizes N=%d H=%d W=%d C=%d Cout=%d", N, H, W, C, Cout);
  FAR3D_CHECK_ARG(C % 32 == 0 && Cout % 32 == 0 && Cout <= 256, "far3d_dwsep_conv_nhwc: C=%d Cout=%d (multiples of 32, Cout <= 256)", C, Cout);
  if (const int rc = dw_check_out_size(who, H, W, stride, Ho, Wo)) return rc;
  const int cs = dt == FAR3D_DT_BF16_PAIR ? 2 : 1;     // stored elements per logical channel
  if (const int rc = dw_check_strides(who, false, cs, N, H, W, C, ldx, x_img_stride, Ho, Wo, Cout, ldy, y_img_stride)) return rc;
  FAR3D_CHECK_ARG(dw_aligned16(8, ldx, ldy, x_img_stride, y_img_stride, {x, y, w9, b1, w_pw, b2}),
                  "far3d_dwsep_conv_nhwc: misaligned rows (pointers and strides must be multiples of 16 bytes = 8 bf16 elements)");
  // the bytes the launch reads of x and writes of y: [first channel of the first pixel, last channel of the last pixel]
  const uintptr_t x0 = (uintptr_t)x, x1 = x0 + 2 * (size_t)((long)(N - 1) * x_img_stride + ((long)H * W - 1) * ldx + C * cs);
  const uintptr_t y0 = (uintptr_t)y, y1 = y0 + 2 * (size_t)((long)(N - 1) * y_img_stride + ((long)Ho * Wo - 1) * ldy + Cout * cs);
  if (!(x1 <= y0 || y1 <= x0)) {
    // interleaved byte ranges are fine when x and y are disjoint channel slices of one buffer (an OSA concat buffer): the same pixel
    // stride, image strides that keep every pixel's residue, and channel windows that do not meet
    bool ok = ldx == ldy && (N == 1 || (x_img_stride % ldx == 0 && y_img_stride % ldx == 0));
    if (ok) {
      const long d = (long)((intptr_t)y0 - (intptr_t)x0) / 2;
      const long dm = ((d % ldx) + ldx) % ldx;              // y's first stored channel relative to x's, within a pixel
      ok = dm >= (long)C * cs && dm + (long)Cout * cs <= ldx;
    }
    FAR3D_CHECK_ARG(ok, "far3d_dwsep_conv_nhwc: x and y overlap");
  }
  const long npix = (long)N * Ho * Wo;
  const long blocks = (npix + DS_PIX - 1) / DS_PIX;
  if (const int rc = dw_check_launch_size(who, blocks)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (cs == 2)
    dwsep_launch<pair_t>(x, w9, b1, w_pw, b2, y, npix, blocks, H, W, C, ldx, x_img_stride, Ho, Wo, Cout, ldy, y_img_stride, stride, act1, act2, st);
  else
    dwsep_launch<bf16_t>(x, w9, b1, w_pw, b2, y, npix, blocks, H, W, C, ldx, x_img_stride, Ho, Wo, Cout, ldy, y_img_stride, stride, act1, act2, st);
  FAR3D_CHECK_LAUNCH("far3d_dwsep_conv_nhwc");
  return FAR3D_OK;
}
