// Row-wise normalisations and reductions of the path (HBM-bound; one wave per row, 16-B accesses).
//   far3d_layernorm        -- nn.LayerNorm(C) (+ optional ReLU) (+ optional second output y2 = y + add, used to
//                             hand the next GEMM "query + query_pos" without another pass).  Decoder norms
//                             (ref models/utils/detr3d_transformer.py:304-307,398-400), cls branch LN
//                             (ref models/dense_heads/farhead.py:230-239), cam_embed LN (:506-512), time_embedding LN.
//   far3d_row_affine_ln    -- out = gamma[row] * LN_noaffine(x[row]) + beta[row] (+ add[row]): the MLN(180) modulation of
//                             queries / memory (ref models/utils/misc.py:153-190; farhead.py:292-303).
//   far3d_groupnorm_nhwc   -- GroupNorm(32, C) + ReLU on NHWC maps (ref models/depth_predictor/depth_predictor.py:43-45).
//   far3d_ese_nhwc         -- VoVNet eSE: x * hsigmoid(fc(avgpool(x))) (+ identity) (ref models/backbones/vovnet.py:173-185,232-236).
//   far3d_maxpool3x3s2_nhwc-- MaxPool2d(3, 2, ceil_mode=True) (ref models/backbones/vovnet.py:249-250).
#include "common.hpp"
#include "dw_core.hpp"
#include "row_core.hpp"
#include <algorithm>

// ---- host side: what the entries of this file share.  An entry calls the rules in its own order with its own name: the order decides
// which message a call with two faults gets.
namespace {
// storage code -> f(T()); F32 = false for the kernels that exist for the two bf16 storages only
template <bool F32 = true, typename F> inline void norm_for_storage(int dt, F f) {
  if constexpr (F32)
    if (dt == FAR3D_DT_F32) return f(float());
  if (dt == FAR3D_DT_BF16_PAIR) f(pair_t()); else f(bf16_t());
}
inline bool pair_channels_ok(int dt, int C) { return dt != FAR3D_DT_BF16_PAIR || C % 32 == 0; }      // C against pair storage
inline int storage_scale(int dt) { return dt == FAR3D_DT_BF16_PAIR ? 2 : 1; }                        // stored elements per logical channel
inline int norm_check_storage(const char* who, int dt, bool channels_ok = true) {
  FAR3D_CHECK_ARG((dt == FAR3D_DT_F32 || dt == FAR3D_DT_BF16 || dt == FAR3D_DT_BF16_PAIR) && channels_ok, "%s: unsupported dtype", who);
  return FAR3D_OK;
}
inline bool multiples_of(long m, std::initializer_list<long> v) { return std::all_of(v.begin(), v.end(), [m](long s) { return s % m == 0; }); }
inline bool aligned16(std::initializer_list<const void*> v) {      // NULL passes
  return std::all_of(v.begin(), v.end(), [](const void* p) { return (uintptr_t)p % 16 == 0; });
}
// MaxPool2d(3, 2, ceil_mode=True): ceil((n - 3) / 2) + 1 outputs, the last window starting inside the input
inline int pooled_size(int n) { const int e = (n - 3 + 1) / 2 + 1; return (e - 1) * 2 >= n ? e - 1 : e; }
// grid of the element-wise kernels: one 4-channel piece per thread, a grid-stride loop past 8192 workgroups
inline dim3 elementwise_grid(long total4) { return dim3((unsigned)std::min(8192L, (total4 + 255) / 256)); }
}  // namespace

// ---------------------------------------------------------------- LayerNorm
template <int MAXV>  // float4 per lane; C <= 256 * MAXV.  The row's arithmetic: row_core.hpp
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ y, int rows,
                                                        int C, int ldx, int ldy, float eps, int act,
                                                        const float* __restrict__ add, int lda, void* __restrict__ y2,
                                                        int ldy2, int y2_dt, void* __restrict__ yb, int ldyb, int yb_dt,
                                                        const int* __restrict__ out_rows) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int orow = out_rows ? out_rows[row] : row;      // row of y2 / yb (far3d_layernorm_rows); requested with the row itself
  const float* xr = x + (long)row * ldx;
  float4 v[MAXV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = (lane + 64 * i) * 4;
    v[i] = c < C ? *reinterpret_cast<const float4*>(xr + c) : make_float4(0, 0, 0, 0);
    s += ln_lane_sum(v[i]);
  }
  const float mean = ln_mean(s, C);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if ((lane + 64 * i) * 4 < C) q += ln_lane_squares(v[i], mean);
  const float rstd = ln_rstd(q, C, eps);
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (c < C) {
      float4 g = make_float4(1, 1, 1, 1), b = make_float4(0, 0, 0, 0);
      if (gamma) g = *reinterpret_cast<const float4*>(gamma + c);
      if (beta) b = *reinterpret_cast<const float4*>(beta + c);
      float4 o = ln_apply(v[i], mean, rstd, g, b);
      if (act == 1) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
      *reinterpret_cast<float4*>(y + (long)row * ldy + c) = o;
      if (yb) {
        if (yb_dt == FAR3D_DT_F32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(yb) + (long)orow * ldyb + c) = o;
        else *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(yb) + (long)orow * ldyb + c) = make_uint2(pack_bf16x2(o.x, o.y), pack_bf16x2(o.z, o.w));
      }
      if (y2) {
        const float4 a = *reinterpret_cast<const float4*>(add + (long)row * lda + c);
        const float4 q2 = make_float4(o.x + a.x, o.y + a.y, o.z + a.z, o.w + a.w);
        if (y2_dt == FAR3D_DT_F32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(y2) + (long)orow * ldy2 + c) = q2;
        else *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(y2) + (long)orow * ldy2 + c) = make_uint2(pack_bf16x2(q2.x, q2.y), pack_bf16x2(q2.z, q2.w));
      }
    }
  }
}

static int layernorm_launch(const float* x, const float* gamma, const float* beta, float* y, int rows, int C,
                            int ldx, int ldy, float eps, int act, const float* add, int lda, void* y2, int ldy2,
                            int y2_dt, void* yb, int ldyb, int yb_dt, const int32_t* out_rows, void* stream) {
  FAR3D_CHECK_ARG(x && y, "far3d_layernorm: null x/y");
  FAR3D_CHECK_ARG(rows >= 0 && C > 0 && (C % 4) == 0 && C <= 1024, "far3d_layernorm: C=%d must be a multiple of 4, <= 1024", C);
  FAR3D_CHECK_ARG(ldx % 4 == 0 && ldy % 4 == 0 && (!y2 || (add && lda % 4 == 0 && ldy2 % 4 == 0)) && (!yb || ldyb % 4 == 0),
                  "far3d_layernorm: row strides must be multiples of 4 elements; y2 needs add");
  if (rows == 0) return FAR3D_OK;
  dim3 grid((rows + 3) / 4), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (C <= 256)
    hipLaunchKernelGGL(layernorm_kernel<1>, grid, block, 0, st, x, gamma, beta, y, rows, C, ldx, ldy, eps, act, add, lda, y2, ldy2, y2_dt, yb, ldyb, yb_dt, (const int*)out_rows);
  else
    hipLaunchKernelGGL(layernorm_kernel<4>, grid, block, 0, st, x, gamma, beta, y, rows, C, ldx, ldy, eps, act, add, lda, y2, ldy2, y2_dt, yb, ldyb, yb_dt, (const int*)out_rows);
  FAR3D_CHECK_LAUNCH("far3d_layernorm");
  return FAR3D_OK;
}

extern "C" int far3d_layernorm(const float* x, const float* gamma, const float* beta, float* y, int rows, int C,
                               int ldx, int ldy, float eps, int act, const float* add, int lda, void* y2, int ldy2,
                               int y2_dt, void* yb, int ldyb, int yb_dt, void* stream) {
  return layernorm_launch(x, gamma, beta, y, rows, C, ldx, ldy, eps, act, add, lda, y2, ldy2, y2_dt, yb, ldyb, yb_dt, nullptr, stream);
}

extern "C" int far3d_layernorm_rows(const float* x, const float* gamma, const float* beta, float* y, int rows, int C,
                                    int ldx, int ldy, float eps, int act, const float* add, int lda, void* y2, int ldy2,
                                    int y2_dt, void* yb, int ldyb, int yb_dt, const int32_t* out_rows, void* stream) {
  FAR3D_CHECK_ARG(out_rows && (y2 || yb), "far3d_layernorm_rows: needs out_rows and at least one of y2 / yb");
  return layernorm_launch(x, gamma, beta, y, rows, C, ldx, ldy, eps, act, add, lda, y2, ldy2, y2_dt, yb, ldyb, yb_dt, out_rows, stream);
}

// ---------------------------------------------------------------- row-affine LayerNorm (MLN apply)
__global__ __launch_bounds__(256) void row_affine_ln_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ add,
                                                            float* __restrict__ y, int rows, int C, int ldx, int ldg, int lda,
                                                            int ldy, float eps, int do_ln) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int c = lane * 4;   // C == 256
  float4 v = *reinterpret_cast<const float4*>(x + (long)row * ldx + c);
  if (do_ln) {
    const float mean = ln_mean(ln_lane_sum(v), C);
    const float rstd = ln_rstd(ln_lane_squares(v, mean), C, eps);
    v = make_float4((v.x - mean) * rstd, (v.y - mean) * rstd, (v.z - mean) * rstd, (v.w - mean) * rstd);
  }
  const float4 g = *reinterpret_cast<const float4*>(gamma + (long)row * ldg + c);
  const float4 b = *reinterpret_cast<const float4*>(beta + (long)row * ldg + c);
  float4 o = make_float4(g.x * v.x + b.x, g.y * v.y + b.y, g.z * v.z + b.z, g.w * v.w + b.w);
  if (add) {
    const float4 a = *reinterpret_cast<const float4*>(add + (long)row * lda + c);
    o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
  }
  *reinterpret_cast<float4*>(y + (long)row * ldy + c) = o;
}

// gamma/beta rows use stride ldg (0 = one shared row for all rows); add rows stride lda (0 = shared row).
extern "C" int far3d_row_affine_ln(const float* x, const float* gamma, const float* beta, const float* add, float* y,
                                   int rows, int C, int ldx, int ldg, int lda, int ldy, float eps, int do_ln, void* stream) {
  FAR3D_CHECK_ARG(x && gamma && beta && y, "far3d_row_affine_ln: null argument");
  FAR3D_CHECK_ARG(C == 256 && ldx % 4 == 0 && ldg % 4 == 0 && lda % 4 == 0 && ldy % 4 == 0, "far3d_row_affine_ln: C must be 256, strides multiples of 4");
  if (rows <= 0) return FAR3D_OK;
  hipLaunchKernelGGL(row_affine_ln_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, add, y, rows,
                     C, ldx, ldg, lda, ldy, eps, do_ln);
  FAR3D_CHECK_LAUNCH("far3d_row_affine_ln");
  return FAR3D_OK;
}

// ---------------------------------------------------------------- per-(image, channel) sums over H*W
// Used by eSE (channel means) and GroupNorm (sum and sum of squares).  x NHWC (T), C channels.
// DETERMINISTIC: workgroup (blk, n) writes its partial sums to part[n][blk][C][2] with plain stores; the consumer
// (ese_gate_kernel / gn_stats_kernel) adds the `nblk` partials in index order.  No atomics, no memset -- run-to-run and
// hipGraph-vs-eager results are bit-identical.
template <typename T>
__global__ __launch_bounds__(256) void chan_sums_kernel(const T* __restrict__ x, float* __restrict__ part, int HW, int C,
                                                        int ldx, long img_stride, int rows_per_block) {
  // thread -> 4 consecutive channels; the 256 threads cover rstep = 256*4/C rows per pass; 8 passes are kept in flight.
  __shared__ float red[2][1024];
  const int n = blockIdx.y;
  const int cq = C / 4;
  const int tcol = threadIdx.x % cq, trow = threadIdx.x / cq;
  const int rstep = 256 / cq;
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = min(HW, r0 + rows_per_block);
  float4 s = make_float4(0, 0, 0, 0), q = make_float4(0, 0, 0, 0);
  if (trow < rstep) {
    const T* base = x + (long)n * img_stride + chan_off<T>(tcol * 4);
    int r = r0 + trow;
    for (; r + 7 * rstep < r1; r += 8 * rstep) {          // 8 row loads in flight per thread: the loop is latency bound
      float4 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = load4(base + (long)(r + k * rstep) * ldx);
      s.x += ((v[0].x + v[1].x) + (v[2].x + v[3].x)) + ((v[4].x + v[5].x) + (v[6].x + v[7].x));
      s.y += ((v[0].y + v[1].y) + (v[2].y + v[3].y)) + ((v[4].y + v[5].y) + (v[6].y + v[7].y));
      s.z += ((v[0].z + v[1].z) + (v[2].z + v[3].z)) + ((v[4].z + v[5].z) + (v[6].z + v[7].z));
      s.w += ((v[0].w + v[1].w) + (v[2].w + v[3].w)) + ((v[4].w + v[5].w) + (v[6].w + v[7].w));
      q.x += ((v[0].x * v[0].x + v[1].x * v[1].x) + (v[2].x * v[2].x + v[3].x * v[3].x)) + ((v[4].x * v[4].x + v[5].x * v[5].x) + (v[6].x * v[6].x + v[7].x * v[7].x));
      q.y += ((v[0].y * v[0].y + v[1].y * v[1].y) + (v[2].y * v[2].y + v[3].y * v[3].y)) + ((v[4].y * v[4].y + v[5].y * v[5].y) + (v[6].y * v[6].y + v[7].y * v[7].y));
      q.z += ((v[0].z * v[0].z + v[1].z * v[1].z) + (v[2].z * v[2].z + v[3].z * v[3].z)) + ((v[4].z * v[4].z + v[5].z * v[5].z) + (v[6].z * v[6].z + v[7].z * v[7].z));
      q.w += ((v[0].w * v[0].w + v[1].w * v[1].w) + (v[2].w * v[2].w + v[3].w * v[3].w)) + ((v[4].w * v[4].w + v[5].w * v[5].w) + (v[6].w * v[6].w + v[7].w * v[7].w));
    }
    for (; r < r1; r += rstep) {
      const float4 a = load4(base + (long)r * ldx);
      s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
      q.x += a.x * a.x; q.y += a.y * a.y; q.z += a.z * a.z; q.w += a.w * a.w;
    }
  }
  // cross-row reduction through LDS: rstep*C <= 1024 floats
  if (trow < rstep) {
    *reinterpret_cast<float4*>(&red[0][trow * C + tcol * 4]) = s;
    *reinterpret_cast<float4*>(&red[1][trow * C + tcol * 4]) = q;
  }
  __syncthreads();
  const int nblk = gridDim.x;
  float* dst = part + ((long)n * nblk + blockIdx.x) * C * 2;
  for (int c = threadIdx.x; c < C; c += 256) {
    float ss = 0.f, qq = 0.f;
    for (int k = 0; k < rstep; ++k) { ss += red[0][k * C + c]; qq += red[1][k * C + c]; }
    *reinterpret_cast<float2*>(dst + 2 * c) = make_float2(ss, qq);
  }
}

// Partial-sum workgroups per image (>= 64 Ki elements per workgroup, at most FAR3D_SUMS_MAX_PARTS) and the rows each of them takes:
// a multiple of the 8 * rstep rows of one unrolled pass.  nparts = ceil(HW / rows_per_block), so no workgroup is empty.
struct ChanSumsPlan { int nparts, rows_per_block; };
static ChanSumsPlan chan_sums_plan(int HW, int C) {
  const long n = std::min<long>(FAR3D_SUMS_MAX_PARTS, std::max<long>(1, ((long)HW * C) >> 16));
  const int pass = 8 * (256 / (C / 4));
  const int rows_per_block = (int)(((HW + n - 1) / n + pass - 1) / pass) * pass;
  return {(HW + rows_per_block - 1) / rows_per_block, rows_per_block};
}

static int launch_chan_sums(const void* x, int dt, float* part, int N, int HW, int C, int ldx, long img_stride, hipStream_t st) {
  const ChanSumsPlan p = chan_sums_plan(HW, C);
  norm_for_storage(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(chan_sums_kernel<T>, dim3(p.nparts, N), dim3(256), 0, st, (const T*)x, part, HW, C, ldx, img_stride, p.rows_per_block);
  });
  return p.nparts;
}

// ---------------------------------------------------------------- eSE
// Partial sums of image n, channel c: part[(n * nparts + b) * C + c] (float2: sum, sum of squares), b = 0..nparts-1; added in
// index order (deterministic).  A thread sums NCH channels (c0, c0 + cstep, ...) at once with 8 partials of each in flight:
// nparts <= 32 costs 4 dependent round trips for all of them (summing them one channel / one tail element at a time cost ~20 round
// trips and made the 16 gate launches of a frame 15 us each).  Slots past nparts / C load nothing and add +0.0.
template <int NCH>
__device__ __forceinline__ void sum_parts(const float2* __restrict__ src, int nparts, int C, int c0, int cstep, float2 (&out)[NCH]) {
  float ss[NCH], qq[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) { ss[j] = 0.f; qq[j] = 0.f; }
  for (int b = 0; b < nparts; b += 8) {
    float2 v[NCH][8];
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
      for (int k = 0; k < 8; ++k)
        v[j][k] = src[(long)min(b + k, nparts - 1) * C + min(c0 + j * cstep, C - 1)];     // clamped, never predicated: a load under a
                                                                                          // condition waits for the one before it
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (!(c0 + j * cstep < C && b + k < nparts)) v[j][k] = make_float2(0.f, 0.f);
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
      for (int k = 0; k < 8; ++k) { ss[j] += v[j][k].x; qq[j] += v[j][k].y; }
  }
#pragma unroll
  for (int j = 0; j < NCH; ++j) out[j] = make_float2(ss[j], qq[j]);
}

// gate[n][c] = hsigmoid( sum_k fcw[c][k] * mean[n][k] + fcb[c] ).  A workgroup owns 16 output channels of one image: it first
// adds the per-workgroup partial channel sums of the pooling kernel (every workgroup of the image does; they are L2 hits), then
// each wave does 4 rows of the mat-vec.
// fixed != null: the channel sums arrive as 64-bit fixed-point integers [N][C] (far3d_conv2d_nhwc's chan_sums) instead of partials.
__global__ __launch_bounds__(256) void ese_gate_kernel(const float* __restrict__ part, const float* __restrict__ fcw,
                                                       const float* __restrict__ fcb, float* __restrict__ gate, int C,
                                                       float inv_hw, int nparts, const long long* __restrict__ fixed) {
  __shared__ float mean[1024];
  const int n = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float2* src = reinterpret_cast<const float2*>(part) + (long)n * nparts * C;
  // each wave: 4 output channels at once (4 independent weight-row streams), float4 loads.  The weight rows do not depend on the
  // pooled means: their loads (C <= 1024: at most 4 per row and lane) go out first and overlap the partial-sum round trips.
  const int c0 = blockIdx.x * 16 + wv * 4;
  float4 w[4][4];
  float bias[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bias[j] = fcb[min(c0 + j, C - 1)];          // clamped (a predicated load waits for the one before it);
                                                                             // channels past C are never stored
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = lane * 4 + i * 256;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      w[i][j] = (k < C && c0 + j < C) ? *reinterpret_cast<const float4*>(fcw + (long)(c0 + j) * C + k) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (fixed) {
    long long fx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) fx[j] = fixed[(long)n * C + min((int)threadIdx.x + j * 256, C - 1)];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (threadIdx.x + j * 256 < C)
        mean[threadIdx.x + j * 256] = (float)((double)fx[j] * (1.0 / (1 << FAR3D_SUMS_FRAC_BITS)) * (double)inv_hw);
  } else {
    float2 sm[4];                                  // C <= 1024: channels t, t + 256, t + 512, t + 768
    sum_parts<4>(src, nparts, C, threadIdx.x, 256, sm);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (threadIdx.x + j * 256 < C) mean[threadIdx.x + j * 256] = sm[j].x * inv_hw;
  }
  __syncthreads();
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = lane * 4 + i * 256;
    if (k < C) {
      const float4 m = *reinterpret_cast<const float4*>(mean + k);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += (w[i][j].x * m.x + w[i][j].y * m.y) + (w[i][j].z * m.z + w[i][j].w * m.w);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = wave_sum(acc[j]);
    if (lane == 0 && c0 + j < C) {
      const float z = a + bias[j];
      gate[(long)n * C + c0 + j] = fminf(fmaxf(z + 3.f, 0.f), 6.f) / 6.f;   // F.relu6(x + 3) / 6
    }
  }
}

// x * g rounded, THEN + d (two fp32 operations as in the reference, vovnet.py:185,232-236): never contracted into an fma, so that
// far3d_ese_nhwc and far3d_ese_fused_nhwc -- two kernels evaluating the same expression -- give the same bits whatever the compiler
// would have chosen to fuse in each (HIP's __fmul_rn is a plain `*` and contracts like one)
__device__ __forceinline__ float ese_mul(float x, float g) {
#pragma clang fp contract(off)
  return x * g;
}
__device__ __forceinline__ float ese_mul_add(float x, float g, float d) {
#pragma clang fp contract(off)
  const float p = x * g;
  return p + d;
}

template <typename T>
__global__ __launch_bounds__(256) void ese_apply_kernel(const T* __restrict__ x, const float* __restrict__ gate,
                                                        const T* __restrict__ idn, T* __restrict__ y, long total4, int C,
                                                        int HW, int ldx, long xs, int ldi, long is, int ldy, long ys,
                                                        long long* __restrict__ consumed, int nconsumed) {
  // the fixed-point channel sums the gate kernel (an earlier launch) read are returned to zero for their next producer
  if (consumed)
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nconsumed; i += (long)gridDim.x * blockDim.x) consumed[i] = 0;
  const int cq = C / 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % cq) * 4;
    const long pr = i / cq;
    const int n = (int)(pr / HW);
    const long pix = pr - (long)n * HW;
    const int co = chan_off<T>(c);
    float4 v = load4(x + n * xs + pix * ldx + co);
    const float4 g = *reinterpret_cast<const float4*>(gate + (long)n * C + c);
    if (idn) {
      const float4 d = load4(idn + n * is + pix * ldi + co);
      v.x = ese_mul_add(v.x, g.x, d.x); v.y = ese_mul_add(v.y, g.y, d.y); v.z = ese_mul_add(v.z, g.z, d.z); v.w = ese_mul_add(v.w, g.w, d.w);
    } else {
      v.x = ese_mul(v.x, g.x); v.y = ese_mul(v.y, g.y); v.z = ese_mul(v.z, g.z); v.w = ese_mul(v.w, g.w);
    }
    store4(y + n * ys + pix * ldy + co, v);
  }
}

// scratch (floats): [N][FAR3D_SUMS_MAX_PARTS][C][2] partial sums, then [N][C] gates.  Size FAR3D_SUMS_SCRATCH_FLOATS(N, C); never
// needs zeroing, and one workspace (sized for the widest layer) serves a whole stream of calls.
extern "C" int far3d_ese_nhwc(const void* x, int dt, const float* fcw, const float* fcb, const void* identity, void* y,
                              float* scratch, int N, int HW, int C, int ldx, long x_img_stride, int ldi,
                              long i_img_stride, int ldy, long y_img_stride, long long* chan_sums, void* stream) {
  const char* who = "far3d_ese_nhwc";
  FAR3D_CHECK_ARG(x && fcw && fcb && y && scratch, "%s: null pointer argument", who);
  FAR3D_CHECK_ARG(!chan_sums || dt != FAR3D_DT_F32, "%s: fixed-point channel sums describe a bf16 / pair map", who);
  FAR3D_CHECK_ARG(N > 0 && HW > 0 && C > 0 && C <= 1024 && multiples_of(4, {C, ldx, ldy, identity ? ldi : 0}),
                  "%s: bad sizes (C=%d must be a multiple of 4, <= 1024)", who, C);
  if (const int rc = norm_check_storage(who, dt)) return rc;
  FAR3D_CHECK_ARG(pair_channels_ok(dt, C), "%s: pair storage needs C %% 32 == 0", who);
  hipStream_t st = (hipStream_t)stream;
  float* sums = scratch;
  float* gate = scratch + (long)N * FAR3D_SUMS_MAX_PARTS * C * 2;
  const int nparts = chan_sums ? 0 : launch_chan_sums(x, dt, sums, N, HW, C, ldx, x_img_stride, st);
  hipLaunchKernelGGL(ese_gate_kernel, dim3((C + 15) / 16, N), dim3(256), 0, st, sums, fcw, fcb, gate, C, 1.f / HW, nparts, (const long long*)chan_sums);
  const long total4 = (long)N * HW * (C / 4);
  norm_for_storage(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(ese_apply_kernel<T>, elementwise_grid(total4), dim3(256), 0, st, (const T*)x, gate, (const T*)identity, (T*)y, total4, C,
                       HW, ldx, x_img_stride, ldi, i_img_stride, ldy, y_img_stride, chan_sums, N * C);
  });
  FAR3D_CHECK_LAUNCH(who);
  return FAR3D_OK;
}

// ---------------------------------------------------------------- eSE apply + stage-end max-pool in one pass (round 5)
// far3d_ese_fused_nhwc = the gate launch of far3d_ese_nhwc(chan_sums) + ONE streaming launch that
//   * applies y = x * g (+ identity) in 16-byte pieces: a thread keeps ONE group of 8 channels (its gates live in registers, no division
//     in the loop, the next piece's loads in flight while the current one is stored);
//   * pooled != null: also writes maxpool3x3s2(ceil)(y), computed from x directly -- every tap is re-evaluated as x * g (+ identity) and
//     ROUNDED TO THE STORAGE FORMAT first, so the result is bit-identical to pooling the stored y; y == null: only the pooled map is wanted
//     (VoVNet stage 2 inside the detector: nothing else reads its output) and the full-resolution map is never written;
//   * returns the consumed channel sums to zero.
// Built first as ONE launch -- the gate workgroups at the head of the grid, the data workgroups spinning on a device-scope counter until
// the gates were published -- and measured 5x SLOWER than the two launches (profiles/r5/ese_handover.txt): on this 8-XCD part the
// hand-over needs either agent-scope fences (`buffer_wbl2 sc1` + `buffer_inv sc1`: a write-back and an invalidation of the XCD's whole L2,
// once per workgroup) or sc1 loads / stores that go past the L2 for every gate of every thread, and a thousand resident workgroups
// polling seven counters serialise on their cache lines.  A kernel boundary is the cheap device-wide release / acquire here.
// the 16-byte channel vectors of a pixel (ld / ldraw / cvt / st / round) are the depthwise family's: dw_core.hpp
template <typename T> using Vec8 = DwIo<T>;

struct EseFusedParams {
  const void* x; const void* idn; void* y; void* pooled;
  const float* gate; long long* sums;
  int N, H, W, C, ldx, ldi, ldy, ldp, Hp, Wp, DB;
  long xs, is, ys, ps;
};

template <typename T, bool POOL>      // POOL = false: the launches without a pooled output (13 of the 16 of a frame) keep their small register file
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void ese_fused_kernel(EseFusedParams P) {
  const int n = blockIdx.y, tid = threadIdx.x, C = P.C;
  const int b = blockIdx.x, cq = C / 8;
  const int HW = P.H * P.W;
  const int stride = P.DB * 256;                           // a multiple of cq: a thread's channel group is the same for all its items
  const int i0 = b * 256 + tid;
  const int cg = i0 % cq, pstep = stride / cq;
  const int co = chan_off<T>(cg * 8);
  const T* x = reinterpret_cast<const T*>(P.x) + (long)n * P.xs + co;
  const T* idn = P.idn ? reinterpret_cast<const T*>(P.idn) + (long)n * P.is + co : nullptr;
  T* y = P.y ? reinterpret_cast<T*>(P.y) + (long)n * P.ys + co : nullptr;
  int pix = i0 / cq;
  float g[8];
  {
    const float4 g0 = *reinterpret_cast<const float4*>(P.gate + (long)n * C + cg * 8), g1 = *reinterpret_cast<const float4*>(P.gate + (long)n * C + cg * 8 + 4);
    g[0] = g0.x; g[1] = g0.y; g[2] = g0.z; g[3] = g0.w; g[4] = g1.x; g[5] = g1.y; g[6] = g1.z; g[7] = g1.w;
  }
  float xv[8], dv[8];
  if (y && pix < HW) {
    Vec8<T>::ld(x + (long)pix * P.ldx, xv);
    if (idn) Vec8<T>::ld(idn + (long)pix * P.ldi, dv);
  }
  // the gate launch has read the channel sums: return them to zero for their next producer
  for (int i = i0; i < C; i += stride) P.sums[(long)n * C + i] = 0;
  if (y) {
    for (; pix < HW; pix += pstep) {
      const int nxt = pix + pstep;
      float xn[8], dn[8];
      if (nxt < HW) {
        Vec8<T>::ld(x + (long)nxt * P.ldx, xn);
        if (idn) Vec8<T>::ld(idn + (long)nxt * P.ldi, dn);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) xv[e] = idn ? ese_mul_add(xv[e], g[e], dv[e]) : ese_mul(xv[e], g[e]);
      Vec8<T>::st(y + (long)pix * P.ldy, xv);
#pragma unroll
      for (int e = 0; e < 8; ++e) { xv[e] = xn[e]; dv[e] = dn[e]; }
    }
  }
  if constexpr (POOL) {
    T* pd = reinterpret_cast<T*>(P.pooled) + (long)n * P.ps + co;
    const int HWp = P.Hp * P.Wp;
    for (int q = i0 / cq; q < HWp; q += pstep) {
      const int oy = q / P.Wp, ox = q - oy * P.Wp;
      // taps past the edge are clamped onto the last row / column, which lies inside the window (ceil mode: a window starts inside the
      // input): a duplicate tap leaves the maximum as it is, and the loads are UNCONDITIONAL -- under `if (iy >= H) continue` every
      // load waited for the one before it (nine dependent round trips per pooled pixel).  A kernel row (3 taps of x and of the
      // identity) is in flight at a time, kept as loaded (16-byte registers) until all of them are issued.
      float m[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
#pragma unroll 1
      for (int ky = 0; ky < 3; ++ky) {                 // not unrolled: the compiler otherwise hoists all 18 loads and spills
        const int iy = min(oy * 2 + ky, P.H - 1);
        typename Vec8<T>::Raw tv[3], td[3];
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const long pp = (long)iy * P.W + min(ox * 2 + kx, P.W - 1);
          tv[kx] = Vec8<T>::ldraw(x + pp * P.ldx);
          if (idn) td[kx] = Vec8<T>::ldraw(idn + pp * P.ldi);
        }
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          float v[8], d[8];
          Vec8<T>::cvt(tv[kx], v);
          if (idn) Vec8<T>::cvt(td[kx], d);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = idn ? ese_mul_add(v[e], g[e], d[e]) : ese_mul(v[e], g[e]);
          Vec8<T>::round(v);
#pragma unroll
          for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], v[e]);
        }
      }
      Vec8<T>::st(pd + (long)q * P.ldp, m);
    }
  }
}

extern "C" int far3d_ese_fused_nhwc(const void* x, int dt, const float* fcw, const float* fcb, const void* identity, void* y, void* pooled,
                                    float* gate, int N, int H, int W, int C, int ldx, long x_img_stride, int ldi,
                                    long i_img_stride, int ldy, long y_img_stride, int Hp, int Wp, int ldp, long p_img_stride,
                                    long long* chan_sums, void* stream) {
  const char* who = "far3d_ese_fused_nhwc";
  FAR3D_CHECK_ARG(x && fcw && fcb && gate && chan_sums && (y || pooled), "%s: null pointer argument (y or pooled must be given)", who);
  FAR3D_CHECK_ARG(dt == FAR3D_DT_BF16 || dt == FAR3D_DT_BF16_PAIR, "%s: bf16 or pair-stored maps (the fixed-point channel sums describe those)", who);
  FAR3D_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && C <= 1024 && C % 8 == 0 && pair_channels_ok(dt, C), "%s: bad sizes (C=%d)", who, C);
  FAR3D_CHECK_ARG(aligned16({x, identity, y, pooled, gate}) &&
                  multiples_of(8, {ldx, x_img_stride, identity ? ldi : 0, identity ? i_img_stride : 0, y ? ldy : 0, y ? y_img_stride : 0,
                                   pooled ? ldp : 0, pooled ? p_img_stride : 0}),
                  "%s: pointers and strides must be multiples of 16 bytes", who);
  if (pooled)
    FAR3D_CHECK_ARG(Hp == pooled_size(H) && Wp == pooled_size(W), "%s: pooled size %dx%d != ceil-mode size %dx%d", who, Hp, Wp, pooled_size(H),
                    pooled_size(W));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ese_gate_kernel, dim3((C + 15) / 16, N), dim3(256), 0, st, (const float*)nullptr, fcw, fcb, gate, C, 1.f / ((float)H * W), 0,
                     (const long long*)chan_sums);
  EseFusedParams P;
  P.x = x; P.idn = identity; P.y = y; P.pooled = pooled; P.gate = gate; P.sums = chan_sums;
  P.N = N; P.H = H; P.W = W; P.C = C; P.ldx = ldx; P.ldi = ldi; P.ldy = ldy; P.ldp = ldp; P.Hp = Hp; P.Wp = Wp;
  P.xs = x_img_stride; P.is = i_img_stride; P.ys = y_img_stride; P.ps = p_img_stride;
  // workgroups per image: one 8-channel piece per thread and ~4 passes, the thread stride a multiple of C / 8 (unit: the smallest
  // workgroup count whose 256 * unit threads are a multiple of C / 8 -- 1 for C = 256 / 512 / 1024, 3 for C = 768)
  const int cq = C / 8;
  int unit = 1;
  while ((256 * unit) % cq) ++unit;
  const long items = (long)(y ? H * W : Hp * Wp) * cq;
  long db = std::min(1200L, (items + 4 * 256 - 1) / (4 * 256));
  db = (db + unit - 1) / unit * unit;
  P.DB = (int)db;
  norm_for_storage<false>(dt, [&](auto t) {
    auto launch = [&](auto pool) {
      hipLaunchKernelGGL((ese_fused_kernel<decltype(t), decltype(pool)::value>), dim3((unsigned)P.DB, (unsigned)N), dim3(256), 0, st, P);
    };
    if (pooled) launch(std::true_type{}); else launch(std::false_type{});
  });
  FAR3D_CHECK_LAUNCH(who);
  return FAR3D_OK;
}

// ---------------------------------------------------------------- GroupNorm + ReLU (NHWC)
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ part, float* __restrict__ stat, int C,
                                                       int groups, float inv_cnt, float eps, int nparts) {
  // one workgroup per image: per-channel sums first (all partial loads in flight), then thread g adds its group's channels in
  // ascending order -- the same additions in the same order as a per-group serial loop
  __shared__ float2 cs[1024];
  const int n = blockIdx.x, cpg = C / groups;
  const float2* src = reinterpret_cast<const float2*>(part) + (long)n * nparts * C;
  float2 sm[4];
  sum_parts<4>(src, nparts, C, threadIdx.x, 256, sm);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (threadIdx.x + j * 256 < C) cs[threadIdx.x + j * 256] = sm[j];
  __syncthreads();
  for (int g = threadIdx.x; g < groups; g += 256) {
    float s = 0.f, q = 0.f;
    for (int c = g * cpg; c < (g + 1) * cpg; ++c) { s += cs[c].x; q += cs[c].y; }
    const float mean = s * inv_cnt;
    const float var = fmaxf(q * inv_cnt - mean * mean, 0.f);
    stat[2 * ((long)n * groups + g)] = mean;
    stat[2 * ((long)n * groups + g) + 1] = 1.f / sqrtf(var + eps);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void gn_apply_kernel(const T* __restrict__ x, const float* __restrict__ stat,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       T* __restrict__ y, long total4, int C, int groups, int HW, int relu) {
  const int cq = C / 4, cpg = C / groups;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % cq) * 4;
    const long pr = i / cq;
    const int n = (int)(pr / HW);
    const long eo = pr * (C * ChanScale<T>::v) + chan_off<T>(c);
    float4 v = load4(x + eo);
    float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int g = (c + e) / cpg;
      const float mean = stat[((long)n * groups + g) * 2], rstd = stat[((long)n * groups + g) * 2 + 1];
      o[e] = (o[e] - mean) * rstd * gamma[c + e] + beta[c + e];
      if (relu) o[e] = fmaxf(o[e], 0.f);
    }
    store4(y + eo, make_float4(o[0], o[1], o[2], o[3]));
  }
}

extern "C" int far3d_groupnorm_nhwc(const void* x, int dt, const float* gamma, const float* beta, void* y, float* scratch,
                                    int N, int HW, int C, int groups, float eps, int relu, void* stream) {
  const char* who = "far3d_groupnorm_nhwc";
  FAR3D_CHECK_ARG(x && gamma && beta && y && scratch, "%s: null pointer argument", who);
  FAR3D_CHECK_ARG(N > 0 && HW > 0 && C % 4 == 0 && C <= 1024 && groups > 0 && C % groups == 0, "%s: bad sizes C=%d groups=%d", who, C, groups);
  if (const int rc = norm_check_storage(who, dt, pair_channels_ok(dt, C))) return rc;
  FAR3D_CHECK_ARG(groups * 2 <= C, "%s: groups*2 must be <= C", who);      // gn_stats_kernel's rule; in front of the first launch
  const int cs = storage_scale(dt);
  hipStream_t st = (hipStream_t)stream;
  float* sums = scratch;                                              // [N][nparts][C][2]
  float* stat = scratch + (long)N * FAR3D_SUMS_MAX_PARTS * C * 2;     // [N][groups][2]
  const int nparts = launch_chan_sums(x, dt, sums, N, HW, C, C * cs, (long)HW * C * cs, st);
  hipLaunchKernelGGL(gn_stats_kernel, dim3(N), dim3(256), 0, st, sums, stat, C, groups, 1.f / ((float)HW * (C / groups)), eps, nparts);
  const long total4 = (long)N * HW * (C / 4);
  norm_for_storage(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(gn_apply_kernel<T>, elementwise_grid(total4), dim3(256), 0, st, (const T*)x, stat, gamma, beta, (T*)y, total4, C, groups, HW, relu);
  });
  FAR3D_CHECK_LAUNCH(who);
  return FAR3D_OK;
}

// ---------------------------------------------------------------- MaxPool 3x3 stride 2, ceil_mode (NHWC)
template <typename T>
__global__ __launch_bounds__(256) void maxpool_kernel(const T* __restrict__ x, T* __restrict__ y, long total4, int C, int H,
                                                      int W, int Ho, int Wo, int ldy, long ys) {
  const int cq = C / 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % cq) * 4;
    long pr = i / cq;
    const int ox = (int)(pr % Wo); pr /= Wo;
    const int oy = (int)(pr % Ho);
    const int n = (int)(pr / Ho);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * 2 + ky;
      if (iy >= H) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * 2 + kx;
        if (ix >= W) continue;
        const float4 v = load4(x + (((long)n * H + iy) * W + ix) * (C * ChanScale<T>::v) + chan_off<T>(c));
        m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
      }
    }
    store4(y + (long)n * ys + ((long)oy * Wo + ox) * ldy + chan_off<T>(c), m);
  }
}

extern "C" int far3d_maxpool3x3s2_nhwc(const void* x, int dt, void* y, int N, int H, int W, int C, int Ho, int Wo, int ldy,
                                       long y_img_stride, void* stream) {
  const char* who = "far3d_maxpool3x3s2_nhwc";
  FAR3D_CHECK_ARG(x && y, "%s: null pointer argument", who);
  if (const int rc = norm_check_storage(who, dt, pair_channels_ok(dt, C))) return rc;
  FAR3D_CHECK_ARG(N > 0 && H > 0 && W > 0 && C % 4 == 0 && ldy >= C * storage_scale(dt) && ldy % 4 == 0, "%s: bad sizes", who);
  FAR3D_CHECK_ARG(Ho == pooled_size(H) && Wo == pooled_size(W), "%s: output %dx%d != ceil-mode size %dx%d", who, Ho, Wo, pooled_size(H),
                  pooled_size(W));
  const long total4 = (long)N * Ho * Wo * (C / 4);
  norm_for_storage(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(maxpool_kernel<T>, elementwise_grid(total4), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, total4, C, H, W, Ho, Wo,
                       ldy, y_img_stride);
  });
  FAR3D_CHECK_LAUNCH(who);
  return FAR3D_OK;
}
