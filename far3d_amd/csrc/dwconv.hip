// Depthwise 3x3 convolution on NHWC maps (pad 1, stride 1 or 2, no bias, no activation; far3d_dwconv3x3_act_nhwc below adds both): the first half of the `dw_conv3x3` layers of
// VoVNet's depthwise specs (ref models/backbones/vovnet.py:100-121; the pointwise 1x1 + BN + ReLU that follows is far3d_conv2d_nhwc).
//
// Bandwidth-bound: 9 FMAs per element against one load and one store.  A lane owns one 16-byte channel vector (8 bf16 / 4 fp32; pair
// storage: 8 logical channels = 16 bytes of hi + 16 bytes of lo) and a run of DW_RUN output pixels along W of one output row.  Its nine
// weight vectors and its 3x3 window live in registers; the window slides along the run, so the lane loads every input pixel of its three
// input rows once.  Consecutive lanes hold consecutive channel vectors of a pixel (contiguous 16-byte pieces), then the next run.  No LDS.
//
// Arithmetic: fp32, acc = fma(x, w, acc) over the taps in the fixed order (ky, kx) = (0,0) (0,1) ... (2,2), padding taps as x = 0 --
// explicit fmaf calls, so the contraction is pinned in the source and the bits of an output element depend on its own nine inputs and
// weights only (never on N, the run it falls in or the launch's other pixels).
#include "common.hpp"

namespace {

template <typename T> struct DwIo;
template <> struct DwIo<float> {
  static constexpr int VEC = 4;
  static __device__ __forceinline__ void ld(const float* p, float* v) {
    const float4 r = *reinterpret_cast<const float4*>(p);
    v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
  }
  static __device__ __forceinline__ void st(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
__device__ __forceinline__ void unpack8(const uint4& r, float* v) {
  v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xffff0000u);
  v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xffff0000u);
  v[4] = __uint_as_float(r.z << 16); v[5] = __uint_as_float(r.z & 0xffff0000u);
  v[6] = __uint_as_float(r.w << 16); v[7] = __uint_as_float(r.w & 0xffff0000u);
}
template <> struct DwIo<bf16_t> {
  static constexpr int VEC = 8;
  static __device__ __forceinline__ void ld(const bf16_t* p, float* v) { unpack8(*reinterpret_cast<const uint4*>(p), v); }
  static __device__ __forceinline__ void st(bf16_t* p, const float* v) {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
  }
};
template <> struct DwIo<pair_t> {     // p -> the hi halves of 8 channels of one 32-channel block; their lo halves 32 elements on
  static constexpr int VEC = 8;
  static __device__ __forceinline__ void ld(const pair_t* p, float* v) {
    float lo[8];
    unpack8(*reinterpret_cast<const uint4*>(p), v);
    unpack8(*reinterpret_cast<const uint4*>(p + 32), lo);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += lo[j];      // exact: hi and lo are pieces of one fp32 mantissa
  }
  static __device__ __forceinline__ void st(pair_t* p, const float* v) {
    uint2 h0, l0, h1, l1;
    split4f(v[0], v[1], v[2], v[3], h0, l0);
    split4f(v[4], v[5], v[6], v[7], h1, l1);
    *reinterpret_cast<uint4*>(p) = make_uint4(h0.x, h0.y, h1.x, h1.y);
    *reinterpret_cast<uint4*>(p + 32) = make_uint4(l0.x, l0.y, l1.x, l1.y);
  }
};

// output pixels per lane: stride 1 loads RUN + 2 input columns for RUN outputs, stride 2 loads 2 RUN + 1
template <int S> struct DwRun { static constexpr int v = S == 1 ? 8 : 4; };

template <typename T, int S>
__global__ __launch_bounds__(256) void dwconv3x3_kernel(const T* __restrict__ x, const float* __restrict__ w, T* __restrict__ y, long items,
                                                        int H, int W, int C, int ldx, long xs, int Ho, int Wo, int ldy, long ys) {
  constexpr int V = DwIo<T>::VEC, RUN = DwRun<S>::v;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= items) return;
  const int cvn = C / V, xrn = (Wo + RUN - 1) / RUN;
  const int c = (int)(i % cvn) * V;
  long r = i / cvn;
  const int ox0 = (int)(r % xrn) * RUN;
  r /= xrn;
  const int oy = (int)(r % Ho);
  const long n = r / Ho;

  float wt[9][V];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
#pragma unroll
    for (int q = 0; q < V; q += 4) {
      const float4 f = *reinterpret_cast<const float4*>(w + (long)t * C + c + q);
      wt[t][q] = f.x; wt[t][q + 1] = f.y; wt[t][q + 2] = f.z; wt[t][q + 3] = f.w;
    }
  }

  const T* rowp[3];
  bool rowv[3];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy * S - 1 + ky;
    rowv[ky] = iy >= 0 && iy < H;
    rowp[ky] = x + n * xs + (long)(rowv[ky] ? iy : 0) * W * ldx + chan_off<T>(c);
  }
  T* yp = y + n * ys + (long)oy * Wo * ldy + chan_off<T>(c);

  // one window column: the three input rows at column ix, zeros outside the map (pad 1)
  auto load_col = [&](int ix, float (&col)[3][V]) {
    const bool cv = ix >= 0 && ix < W;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      if (cv && rowv[ky]) {
        DwIo<T>::ld(rowp[ky] + (long)ix * ldx, col[ky]);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) col[ky][j] = 0.f;
      }
    }
  };
  auto emit = [&](int ox, const float (&a)[3][V], const float (&b)[3][V], const float (&d)[3][V]) {
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float s = 0.f;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        s = fmaf(a[ky][j], wt[ky * 3 + 0][j], s);
        s = fmaf(b[ky][j], wt[ky * 3 + 1][j], s);
        s = fmaf(d[ky][j], wt[ky * 3 + 2][j], s);
      }
      acc[j] = s;
    }
    DwIo<T>::st(yp + (long)ox * ldy, acc);
  };

  float a[3][V], b[3][V], d[3][V];
  if (S == 1) {
    load_col(ox0 - 1, a);
    load_col(ox0, b);
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
      const int ox = ox0 + k;
      if (ox >= Wo) break;
      load_col(ox + 1, d);
      emit(ox, a, b, d);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int j = 0; j < V; ++j) { a[ky][j] = b[ky][j]; b[ky][j] = d[ky][j]; }
    }
  } else {
    load_col(ox0 * 2 - 1, a);
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
      const int ox = ox0 + k;
      if (ox >= Wo) break;
      load_col(ox * 2, b);
      load_col(ox * 2 + 1, d);
      emit(ox, a, b, d);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int j = 0; j < V; ++j) a[ky][j] = d[ky][j];
    }
  }
}

template <typename T>
void dw_launch(const void* x, const float* w, void* y, long items, long blocks, int H, int W, int C, int ldx, long xs, int Ho, int Wo,
               int ldy, long ys, int stride, hipStream_t st) {
  if (stride == 1)
    hipLaunchKernelGGL((dwconv3x3_kernel<T, 1>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, w, (T*)y, items, H, W, C, ldx, xs, Ho,
                       Wo, ldy, ys);
  else
    hipLaunchKernelGGL((dwconv3x3_kernel<T, 2>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, w, (T*)y, items, H, W, C, ldx, xs, Ho,
                       Wo, ldy, ys);
}


// ---- far3d_dwconv3x3_act_nhwc: the same window walk with a folded-BN bias, an activation and up to two weight sets per window (the first
// halves of mmcv's DepthwiseSeparableConvModule in the light YOLOX towers, ref models/dense_heads/yolox_head.py:197-219; with two sets, the
// cls and reg towers' first depthwise layers read their common FPN map once).  Output channel r*C + c = act(dw(x[c]; w[r]) + b[r][c]).
// The nine fmas per set are the ones of dwconv3x3_kernel in the same order, the bias is one fp32 add after them (absent: no add at all),
// so an element's bits depend on its own window, weights and bias only -- not on N, its run or REPS -- and REPS = 1 without bias and
// activation returns dwconv3x3_kernel's bits.
template <typename T, int S, int REPS>
__global__ __launch_bounds__(256) void dwconv3x3_act_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                            T* __restrict__ y, long items, int H, int W, int C, int ldx, long xs, int Ho, int Wo,
                                                            int ldy, long ys, int act) {
  constexpr int V = DwIo<T>::VEC, RUN = DwRun<S>::v;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= items) return;
  const int cvn = C / V, xrn = (Wo + RUN - 1) / RUN;
  const int c = (int)(i % cvn) * V;
  long r = i / cvn;
  const int ox0 = (int)(r % xrn) * RUN;
  r /= xrn;
  const int oy = (int)(r % Ho);
  const long n = r / Ho;

  float wt[REPS][9][V], bs[REPS][V];
#pragma unroll
  for (int p = 0; p < REPS; ++p) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
      for (int q = 0; q < V; q += 4) {
        const float4 f = *reinterpret_cast<const float4*>(w + ((long)p * 9 + t) * C + c + q);
        wt[p][t][q] = f.x; wt[p][t][q + 1] = f.y; wt[p][t][q + 2] = f.z; wt[p][t][q + 3] = f.w;
      }
    }
#pragma unroll
    for (int q = 0; q < V; q += 4) {
      float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
      if (bias) f = *reinterpret_cast<const float4*>(bias + (long)p * C + c + q);
      bs[p][q] = f.x; bs[p][q + 1] = f.y; bs[p][q + 2] = f.z; bs[p][q + 3] = f.w;
    }
  }

  const T* rowp[3];
  bool rowv[3];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy * S - 1 + ky;
    rowv[ky] = iy >= 0 && iy < H;
    rowp[ky] = x + n * xs + (long)(rowv[ky] ? iy : 0) * W * ldx + chan_off<T>(c);
  }
  T* yp[REPS];
#pragma unroll
  for (int p = 0; p < REPS; ++p) yp[p] = y + n * ys + (long)oy * Wo * ldy + chan_off<T>(p * C + c);

  auto load_col = [&](int ix, float (&col)[3][V]) {
    const bool cv = ix >= 0 && ix < W;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      if (cv && rowv[ky]) {
        DwIo<T>::ld(rowp[ky] + (long)ix * ldx, col[ky]);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) col[ky][j] = 0.f;
      }
    }
  };
  auto emit = [&](int ox, const float (&a)[3][V], const float (&b)[3][V], const float (&d)[3][V]) {
#pragma unroll
    for (int p = 0; p < REPS; ++p) {
      float acc[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float s = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          s = fmaf(a[ky][j], wt[p][ky * 3 + 0][j], s);
          s = fmaf(b[ky][j], wt[p][ky * 3 + 1][j], s);
          s = fmaf(d[ky][j], wt[p][ky * 3 + 2][j], s);
        }
        if (bias) s = s + bs[p][j];
        if (act == 1) s = fmaxf(s, 0.f);
        else if (act == 2) s = swish_f32(s);
        acc[j] = s;
      }
      DwIo<T>::st(yp[p] + (long)ox * ldy, acc);
    }
  };

  float a[3][V], b[3][V], d[3][V];
  if (S == 1) {
    load_col(ox0 - 1, a);
    load_col(ox0, b);
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
      const int ox = ox0 + k;
      if (ox >= Wo) break;
      load_col(ox + 1, d);
      emit(ox, a, b, d);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int j = 0; j < V; ++j) { a[ky][j] = b[ky][j]; b[ky][j] = d[ky][j]; }
    }
  } else {
    load_col(ox0 * 2 - 1, a);
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
      const int ox = ox0 + k;
      if (ox >= Wo) break;
      load_col(ox * 2, b);
      load_col(ox * 2 + 1, d);
      emit(ox, a, b, d);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int j = 0; j < V; ++j) a[ky][j] = d[ky][j];
    }
  }
}

template <typename T, int S>
void dw_act_launch_s(const void* x, const float* w, const float* bias, void* y, long items, long blocks, int H, int W, int C, int ldx, long xs,
                     int Ho, int Wo, int ldy, long ys, int reps, int act, hipStream_t st) {
  if (reps == 1)
    hipLaunchKernelGGL((dwconv3x3_act_kernel<T, S, 1>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, w, bias, (T*)y, items, H, W, C, ldx,
                       xs, Ho, Wo, ldy, ys, act);
  else
    hipLaunchKernelGGL((dwconv3x3_act_kernel<T, S, 2>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, w, bias, (T*)y, items, H, W, C, ldx,
                       xs, Ho, Wo, ldy, ys, act);
}

template <typename T>
void dw_act_launch(const void* x, const float* w, const float* bias, void* y, long items, long blocks, int H, int W, int C, int ldx, long xs,
                   int Ho, int Wo, int ldy, long ys, int stride, int reps, int act, hipStream_t st) {
  if (stride == 1)
    dw_act_launch_s<T, 1>(x, w, bias, y, items, blocks, H, W, C, ldx, xs, Ho, Wo, ldy, ys, reps, act, st);
  else
    dw_act_launch_s<T, 2>(x, w, bias, y, items, blocks, H, W, C, ldx, xs, Ho, Wo, ldy, ys, reps, act, st);
}

}  // namespace

extern "C" int far3d_dwconv3x3_nhwc(const void* x, int dt, const float* w, void* y, int N, int H, int W, int C, int ldx,
                                    long x_img_stride, int Ho, int Wo, int ldy, long y_img_stride, int stride, void* stream) {
  FAR3D_CHECK_ARG(x && w && y, "far3d_dwconv3x3_nhwc: null pointer argument");
  FAR3D_CHECK_ARG(dt == FAR3D_DT_F32 || dt == FAR3D_DT_BF16 || dt == FAR3D_DT_BF16_PAIR, "far3d_dwconv3x3_nhwc: unsupported dtype %d", dt);
  FAR3D_CHECK_ARG(stride == 1 || stride == 2, "far3d_dwconv3x3_nhwc: stride %d (1 or 2 only)", stride);
  FAR3D_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0, "far3d_dwconv3x3_nhwc: bad sizes N=%d H=%d W=%d C=%d", N, H, W, C);
  FAR3D_CHECK_ARG(C % 8 == 0, "far3d_dwconv3x3_nhwc: C=%d is not a multiple of 8", C);
  const bool pair = dt == FAR3D_DT_BF16_PAIR;
  FAR3D_CHECK_ARG(!pair || C % 32 == 0, "far3d_dwconv3x3_nhwc: pair storage needs C %% 32 == 0 (C=%d)", C);
  const int eh = (H - 1) / stride + 1, ew = (W - 1) / stride + 1;
  FAR3D_CHECK_ARG(Ho == eh && Wo == ew, "far3d_dwconv3x3_nhwc: output %dx%d != %dx%d (3x3, pad 1, stride %d of %dx%d)", Ho, Wo, eh, ew, stride,
                  H, W);
  const int cs = pair ? 2 : 1;                         // stored elements per logical channel
  const int al = dt == FAR3D_DT_F32 ? 4 : 8;           // elements per 16 bytes
  const size_t eb = dt == FAR3D_DT_F32 ? 4 : 2;
  FAR3D_CHECK_ARG(ldx >= C * cs && ldy >= C * cs, "far3d_dwconv3x3_nhwc: pixel strides %d / %d below the %d stored channels", ldx, ldy, C * cs);
  FAR3D_CHECK_ARG(N == 1 || (x_img_stride >= (long)H * W * ldx - (ldx - C * cs) && y_img_stride >= (long)Ho * Wo * ldy - (ldy - C * cs)),
                  "far3d_dwconv3x3_nhwc: image strides below one image");
  FAR3D_CHECK_ARG(ldx % al == 0 && ldy % al == 0 && x_img_stride % al == 0 && y_img_stride % al == 0 &&
                      ((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0 && ((uintptr_t)w % 16) == 0,
                  "far3d_dwconv3x3_nhwc: misaligned rows (pointers and strides must be multiples of 16 bytes = %d elements of %zu bytes)", al, eb);
  const int vec = dt == FAR3D_DT_F32 ? 4 : 8;
  const int run = stride == 1 ? DwRun<1>::v : DwRun<2>::v;
  const long items = (long)N * Ho * ((Wo + run - 1) / run) * (C / vec);      // pixel runs x channel vectors: one lane each
  const long blocks = (items + 255) / 256;
  FAR3D_CHECK_ARG(blocks <= 0x7fffffffL, "far3d_dwconv3x3_nhwc: launch too large (%ld workgroups)", blocks);
  hipStream_t st = (hipStream_t)stream;
  if (dt == FAR3D_DT_F32)
    dw_launch<float>(x, w, y, items, blocks, H, W, C, ldx, x_img_stride, Ho, Wo, ldy, y_img_stride, stride, st);
  else if (pair)
    dw_launch<pair_t>(x, w, y, items, blocks, H, W, C, ldx, x_img_stride, Ho, Wo, ldy, y_img_stride, stride, st);
  else
    dw_launch<bf16_t>(x, w, y, items, blocks, H, W, C, ldx, x_img_stride, Ho, Wo, ldy, y_img_stride, stride, st);
  FAR3D_CHECK_LAUNCH("far3d_dwconv3x3_nhwc");
  return FAR3D_OK;
}

extern "C" int far3d_dwconv3x3_act_nhwc(const void* x, int dt, const float* w, const float* bias, void* y, int N, int H, int W, int C, int ldx,
                                        long x_img_stride, int Ho, int Wo, int ldy, long y_img_stride, int stride, int reps, int act,
                                        void* stream) {
  FAR3D_CHECK_ARG(x && w && y, "far3d_dwconv3x3_act_nhwc: null pointer argument");
  FAR3D_CHECK_ARG(dt == FAR3D_DT_F32 || dt == FAR3D_DT_BF16 || dt == FAR3D_DT_BF16_PAIR, "far3d_dwconv3x3_act_nhwc: unsupported dtype %d", dt);
  FAR3D_CHECK_ARG(stride == 1 || stride == 2, "far3d_dwconv3x3_act_nhwc: stride %d (1 or 2 only)", stride);
  FAR3D_CHECK_ARG(reps == 1 || reps == 2, "far3d_dwconv3x3_act_nhwc: reps %d (1 or 2 weight sets)", reps);
  FAR3D_CHECK_ARG(act >= 0 && act <= 2, "far3d_dwconv3x3_act_nhwc: act %d (0 none, 1 ReLU, 2 Swish)", act);
  FAR3D_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0, "far3d_dwconv3x3_act_nhwc: bad sizes N=%d H=%d W=%d C=%d", N, H, W, C);
  FAR3D_CHECK_ARG(C % 8 == 0, "far3d_dwconv3x3_act_nhwc: C=%d is not a multiple of 8", C);
  const bool pair = dt == FAR3D_DT_BF16_PAIR;
  FAR3D_CHECK_ARG(!pair || C % 32 == 0, "far3d_dwconv3x3_act_nhwc: pair storage needs C %% 32 == 0 (C=%d)", C);
  const int eh = (H - 1) / stride + 1, ew = (W - 1) / stride + 1;
  FAR3D_CHECK_ARG(Ho == eh && Wo == ew, "far3d_dwconv3x3_act_nhwc: output %dx%d != %dx%d (3x3, pad 1, stride %d of %dx%d)", Ho, Wo, eh, ew,
                  stride, H, W);
  const int cs = pair ? 2 : 1;                         // stored elements per logical channel
  const int al = dt == FAR3D_DT_F32 ? 4 : 8;           // elements per 16 bytes
  const size_t eb = dt == FAR3D_DT_F32 ? 4 : 2;
  FAR3D_CHECK_ARG(ldx >= C * cs && ldy >= reps * C * cs, "far3d_dwconv3x3_act_nhwc: pixel strides %d / %d below the %d / %d stored channels", ldx,
                  ldy, C * cs, reps * C * cs);
  FAR3D_CHECK_ARG(N == 1 || (x_img_stride >= (long)H * W * ldx - (ldx - C * cs) && y_img_stride >= (long)Ho * Wo * ldy - (ldy - reps * C * cs)),
                  "far3d_dwconv3x3_act_nhwc: image strides below one image");
  FAR3D_CHECK_ARG(ldx % al == 0 && ldy % al == 0 && x_img_stride % al == 0 && y_img_stride % al == 0 &&
                      ((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0 && ((uintptr_t)w % 16) == 0 && ((uintptr_t)bias % 16) == 0,
                  "far3d_dwconv3x3_act_nhwc: misaligned rows (pointers and strides must be multiples of 16 bytes = %d elements of %zu bytes)", al,
                  eb);
  const int vec = dt == FAR3D_DT_F32 ? 4 : 8;
  const int run = stride == 1 ? DwRun<1>::v : DwRun<2>::v;
  const long items = (long)N * Ho * ((Wo + run - 1) / run) * (C / vec);      // pixel runs x channel vectors: one lane each
  const long blocks = (items + 255) / 256;
  FAR3D_CHECK_ARG(blocks <= 0x7fffffffL, "far3d_dwconv3x3_act_nhwc: launch too large (%ld workgroups)", blocks);
  hipStream_t st = (hipStream_t)stream;
  if (dt == FAR3D_DT_F32)
    dw_act_launch<float>(x, w, bias, y, items, blocks, H, W, C, ldx, x_img_stride, Ho, Wo, ldy, y_img_stride, stride, reps, act, st);
  else if (pair)
    dw_act_launch<pair_t>(x, w, bias, y, items, blocks, H, W, C, ldx, x_img_stride, Ho, Wo, ldy, y_img_stride, stride, reps, act, st);
  else
    dw_act_launch<bf16_t>(x, w, bias, y, items, blocks, H, W, C, ldx, x_img_stride, Ho, Wo, ldy, y_img_stride, stride, reps, act, st);
  FAR3D_CHECK_LAUNCH("far3d_dwconv3x3_act_nhwc");
  return FAR3D_OK;
}
