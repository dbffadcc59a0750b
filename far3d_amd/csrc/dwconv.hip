// Depthwise 3x3 convolution on NHWC maps (pad 1, stride 1 or 2), optionally with a folded-BN bias, an activation and up to two weight sets
// per window: ONE window kernel behind two entries.
//   far3d_dwconv3x3_nhwc      one weight set, no bias, no activation: the first half of the `dw_conv3x3` layers of VoVNet's depthwise specs
//                             (ref models/backbones/vovnet.py:100-121; the pointwise 1x1 + BN + ReLU that follows is far3d_conv2d_nhwc);
//   far3d_dwconv3x3_act_nhwc  the first halves of mmcv's DepthwiseSeparableConvModule in the light YOLOX towers (ref
//                             models/dense_heads/yolox_head.py:197-219; with two sets, the cls and reg towers' first depthwise layers read
//                             their common FPN map once).  Output channel r*C + c = act(dw(x[c]; w[r]) + b[r][c]).
//
// Bandwidth-bound: 9 FMAs per element against one load and one store.  A lane owns one 16-byte channel vector (8 bf16 / 4 fp32; pair
// storage: 8 logical channels = 16 bytes of hi + 16 bytes of lo) and a run of DwRun output pixels along W of one output row.  Its nine
// weight vectors per set and its 3x3 window live in registers; the window slides along the run, so the lane loads every input pixel of its
// three input rows once.  Consecutive lanes hold consecutive channel vectors of a pixel (contiguous 16-byte pieces), then the next run.
// No LDS.  The arithmetic contract (tap order, bias, activation, storage rounding) is stated in dw_core.hpp.
#include "dw_core.hpp"

namespace {

// MODE: the weight sets per window, 1 or 2, or DW_PLAIN: one set and neither bias nor activation in the code at all -- the instantiations
// of far3d_dwconv3x3_nhwc, which with MODE = 1 spent 0.5 to 27 us more per launch than the kernel it had of its own.
constexpr int DW_PLAIN = 0;
template <typename T, int S, int MODE>
__global__ __launch_bounds__(256) void dwconv3x3_act_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                            T* __restrict__ y, long items, int H, int W, int C, int ldx, long xs, int Ho, int Wo,
                                                            int ldy, long ys, int act) {
  constexpr bool PLAIN = MODE == DW_PLAIN;
  constexpr int REPS = PLAIN ? 1 : MODE;
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
    if constexpr (!PLAIN) {
#pragma unroll
      for (int q = 0; q < V; q += 4) {
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bias) f = *reinterpret_cast<const float4*>(bias + (long)p * C + c + q);
        bs[p][q] = f.x; bs[p][q + 1] = f.y; bs[p][q + 2] = f.z; bs[p][q + 3] = f.w;
      }
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
        if constexpr (!PLAIN) {
          if (bias) s = s + bs[p][j];
          DW_ACT(s, act);
        }
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

// storage, stride and mode -> f(T(), S, MODE), the last two as integral constants
template <typename F>
inline void dw_for_kernel(int dt, int stride, int mode, F f) {
  auto sets = [&](auto t, auto s) {
    if (mode == DW_PLAIN) f(t, s, std::integral_constant<int, DW_PLAIN>{});
    else if (mode == 1) f(t, s, std::integral_constant<int, 1>{});
    else f(t, s, std::integral_constant<int, 2>{});
  };
  auto strides = [&](auto t) {
    if (stride == 1) sets(t, std::integral_constant<int, 1>{}); else sets(t, std::integral_constant<int, 2>{});
  };
  if (dt == FAR3D_DT_F32) strides(float()); else if (dt == FAR3D_DT_BF16_PAIR) strides(pair_t()); else strides(bf16_t());
}

// Both entries: checks in far3d_dwconv3x3_act_nhwc's order (the plain entry passes reps = 1, act = 0 and no bias, which pass theirs), then
// the launch.  `plain` chooses the form of the pixel-stride message and the kernel without bias and activation code.
int dw_entry(const char* who, bool plain, const void* x, int dt, const float* w, const float* bias, void* y, int N, int H, int W, int C,
             int ldx, long xs, int Ho, int Wo, int ldy, long ys, int stride, int reps, int act, void* stream) {
  FAR3D_CHECK_ARG(x && w && y, "%s: null pointer argument", who);
  FAR3D_CHECK_ARG(dt == FAR3D_DT_F32 || dt == FAR3D_DT_BF16 || dt == FAR3D_DT_BF16_PAIR, "%s: unsupported dtype %d", who, dt);
  if (const int rc = dw_check_stride(who, stride)) return rc;
  FAR3D_CHECK_ARG(reps == 1 || reps == 2, "%s: reps %d (1 or 2 weight sets)", who, reps);
  FAR3D_CHECK_ARG(dw_act_ok(act), "%s: act %d (0 none, 1 ReLU, 2 Swish)", who, act);
  FAR3D_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0, "%s: bad sizes N=%d H=%d W=%d C=%d", who, N, H, W, C);
  FAR3D_CHECK_ARG(C % 8 == 0, "%s: C=%d is not a multiple of 8", who, C);
  const bool pair = dt == FAR3D_DT_BF16_PAIR;
  FAR3D_CHECK_ARG(!pair || C % 32 == 0, "%s: pair storage needs C %% 32 == 0 (C=%d)", who, C);
  if (const int rc = dw_check_out_size(who, H, W, stride, Ho, Wo)) return rc;
  if (const int rc = dw_check_strides(who, plain, pair ? 2 : 1, N, H, W, C, ldx, xs, Ho, Wo, reps * C, ldy, ys)) return rc;
  const int vec = dt == FAR3D_DT_F32 ? 4 : 8;          // elements per 16 bytes
  FAR3D_CHECK_ARG(dw_aligned16(vec, ldx, ldy, xs, ys, {x, y, w, bias}),
                  "%s: misaligned rows (pointers and strides must be multiples of 16 bytes = %d elements of %zu bytes)", who, vec, (size_t)(16 / vec));
  const int run = stride == 1 ? DwRun<1>::v : DwRun<2>::v;
  const long items = (long)N * Ho * ((Wo + run - 1) / run) * (C / vec);      // pixel runs x channel vectors: one lane each
  const long blocks = (items + 255) / 256;
  if (const int rc = dw_check_launch_size(who, blocks)) return rc;
  dw_for_kernel(dt, stride, plain ? DW_PLAIN : reps, [&](auto t, auto s, auto mode) {
    using T = decltype(t);
    hipLaunchKernelGGL((dwconv3x3_act_kernel<T, decltype(s)::value, decltype(mode)::value>), dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, (const T*)x, w, bias, (T*)y, items, H, W, C, ldx, xs, Ho, Wo, ldy, ys, act);
  });
  FAR3D_CHECK_LAUNCH(who);
  return FAR3D_OK;
}

}  // namespace

extern "C" int far3d_dwconv3x3_nhwc(const void* x, int dt, const float* w, void* y, int N, int H, int W, int C, int ldx,
                                    long x_img_stride, int Ho, int Wo, int ldy, long y_img_stride, int stride, void* stream) {
  return dw_entry("far3d_dwconv3x3_nhwc", true, x, dt, w, nullptr, y, N, H, W, C, ldx, x_img_stride, Ho, Wo, ldy, y_img_stride, stride, 1,
                  DW_ACT_NONE, stream);
}

extern "C" int far3d_dwconv3x3_act_nhwc(const void* x, int dt, const float* w, const float* bias, void* y, int N, int H, int W, int C, int ldx,
                                        long x_img_stride, int Ho, int Wo, int ldy, long y_img_stride, int stride, int reps, int act,
                                        void* stream) {
  return dw_entry("far3d_dwconv3x3_act_nhwc", false, x, dt, w, bias, y, N, H, W, C, ldx, x_img_stride, Ho, Wo, ldy, y_img_stride, stride,
                  reps, act, stream);
}
