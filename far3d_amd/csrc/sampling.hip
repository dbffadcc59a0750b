// Deformable sampling kernels for the Far3D cross-attention.
//
//  * far3d_msda_forward      -- drop-in for mmcv's ms_deform_attn_forward as called at
//                               reference detr3d_transformer.py:561-563 (operator boundary).
//  * far3d_aggregate_forward -- the fused perspective-aware aggregation: everything in
//                               DeformableFeatureAggregationCuda.feature_sampling + _get_weights'
//                               softmax (detr3d_transformer.py:535-569) in ONE launch:
//                               projection of the 13 key points into the 7 cameras, visibility
//                               culling, 364-way softmax per group, bilinear gather over 4 levels,
//                               weighting, and the cross-camera sum.  No (B*N,A,8,4,13,2) replicated
//                               location tensor, no (B*N,A,8,52) permuted weight tensor, no
//                               (B*N,A,256) per-camera output ever reaches HBM.
//
// Layout facts the kernels are built around (gfx950, wave = 64 lanes):
//   value maps are token-major (camera, token, 256 channels); one token row is 1 KiB fp32 / 512 B
//   bf16, so ONE wave-wide 16 B(8 B)-per-lane load fetches a whole token row for all 8 groups:
//   lane = group*8 + chunk, 4 channels per lane.  All 8 groups sample the same pixel (the reference
//   replicates locations over groups, :555), so a bilinear sample is 4 fully-coalesced row loads.
#include "common.hpp"
#include "agg_tables.hpp"
#include <stdlib.h>
#include <type_traits>

// ------------------------------------------------------------------------------------------
// Generic MSDA (mmcv contract).  value (bs,S,H,Dh) TV; shapes (L,2) i64 (h,w); lsi (L) i64;
// loc (bs,Q,H,L,P,2) f32 in [0,1] (x,y); attn (bs,Q,H,L,P) f32; out (bs,Q,H*Dh) f32.
// One thread owns 4 consecutive channels of one (b,q,h): neighbouring lanes read neighbouring
// 16-B pieces of the same token row -> coalesced.
// ------------------------------------------------------------------------------------------
template <typename TV>
__global__ __launch_bounds__(256) void msda_fwd_kernel(const TV* __restrict__ value,
                                                       const int64_t* __restrict__ shapes,
                                                       const int64_t* __restrict__ lsi,
                                                       const float* __restrict__ loc,
                                                       const float* __restrict__ attn,
                                                       float* __restrict__ out, int bs, int S, int H,
                                                       int Dh, int L, int Q, int P) {
  const int c4n = Dh >> 2;
  const long total = (long)bs * Q * H * c4n;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(idx % c4n);
    long t = idx / c4n;
    const int h = (int)(t % H);
    t /= H;
    const int q = (int)(t % Q);
    const int b = (int)(t / Q);
    const long bqh = ((long)b * Q + q) * H + h;
    const float* locp = loc + bqh * L * P * 2;
    const float* wp = attn + bqh * L * P;
    const TV* vb = value + (long)b * S * H * Dh + h * Dh + c4 * 4;
    const long row = (long)H * Dh;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int l = 0; l < L; ++l) {
      const int Hl = (int)shapes[2 * l], Wl = (int)shapes[2 * l + 1];
      const TV* vl = vb + lsi[l] * row;
      for (int p = 0; p < P; ++p) {
        const float lx = locp[(l * P + p) * 2], ly = locp[(l * P + p) * 2 + 1];
        const float aw = wp[l * P + p];
        const float h_im = ly * Hl - 0.5f, w_im = lx * Wl - 0.5f;
        if (h_im > -1.f && w_im > -1.f && h_im < Hl && w_im < Wl) {
          const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
          const int h_high = h_low + 1, w_high = w_low + 1;
          const float lh = h_im - h_low, lw = w_im - w_low;
          const float hh = 1.f - lh, hw = 1.f - lw;
          float4 v1 = make_float4(0, 0, 0, 0), v2 = v1, v3 = v1, v4 = v1;
          if (h_low >= 0 && w_low >= 0) v1 = load4(vl + ((long)h_low * Wl + w_low) * row);
          if (h_low >= 0 && w_high <= Wl - 1) v2 = load4(vl + ((long)h_low * Wl + w_high) * row);
          if (h_high <= Hl - 1 && w_low >= 0) v3 = load4(vl + ((long)h_high * Wl + w_low) * row);
          if (h_high <= Hl - 1 && w_high <= Wl - 1) v4 = load4(vl + ((long)h_high * Wl + w_high) * row);
          const float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
          acc.x += aw * (w1 * v1.x + w2 * v2.x + w3 * v3.x + w4 * v4.x);
          acc.y += aw * (w1 * v1.y + w2 * v2.y + w3 * v3.y + w4 * v4.y);
          acc.z += aw * (w1 * v1.z + w2 * v2.z + w3 * v3.z + w4 * v4.z);
          acc.w += aw * (w1 * v1.w + w2 * v2.w + w3 * v3.w + w4 * v4.w);
        }
      }
    }
    *reinterpret_cast<float4*>(out + bqh * Dh + c4 * 4) = acc;
  }
}

extern "C" int far3d_msda_forward(const void* value, int value_dtype, const int64_t* spatial_shapes,
                                  const int64_t* level_start_index, const float* sampling_loc,
                                  const float* attn_weight, float* out, int bs, int S, int H, int Dh,
                                  int L, int Q, int P, void* stream) {
  FAR3D_CHECK_ARG(bs >= 0 && S > 0 && H > 0 && Dh > 0 && L > 0 && Q >= 0 && P > 0,
                  "far3d_msda_forward: bad sizes bs=%d S=%d H=%d Dh=%d L=%d Q=%d P=%d", bs, S, H, Dh, L, Q, P);
  FAR3D_CHECK_ARG((Dh & 3) == 0, "far3d_msda_forward: head dim %d must be a multiple of 4", Dh);
  FAR3D_CHECK_ARG(value_dtype == FAR3D_DT_F32 || value_dtype == FAR3D_DT_BF16,
                  "far3d_msda_forward: unsupported value dtype %d", value_dtype);
  const long total = (long)bs * Q * H * (Dh / 4);
  if (total == 0) return FAR3D_OK;  // empty query set: nothing to write (pointers may be null)
  FAR3D_CHECK_ARG(value && spatial_shapes && level_start_index && sampling_loc && attn_weight && out,
                  "far3d_msda_forward: null pointer argument");
  long blocks = (total + 255) / 256;
  if (blocks > 256L * 16) blocks = 256L * 16;
  hipStream_t st = (hipStream_t)stream;
  if (value_dtype == FAR3D_DT_F32)
    hipLaunchKernelGGL(msda_fwd_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)value,
                       spatial_shapes, level_start_index, sampling_loc, attn_weight, out, bs, S, H, Dh, L, Q, P);
  else
    hipLaunchKernelGGL(msda_fwd_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, (const bf16_t*)value,
                       spatial_shapes, level_start_index, sampling_loc, attn_weight, out, bs, S, H, Dh, L, Q, P);
  FAR3D_CHECK_LAUNCH("far3d_msda_forward");
  return FAR3D_OK;
}

// ------------------------------------------------------------------------------------------
// Fused perspective-aware aggregation.  One 256-thread workgroup (4 waves) per query.
//   phase 1: 91 (camera, point) projections -> LDS (u,v) + per-level in-range bit mask
//   phase 2: 364-way softmax for the 8 groups (logit = U[a] + Vc[n]; see aggregate.py) -> LDS
//   phase 3: each wave walks the visible (camera,point) pairs; per level 4 coalesced row loads
//   phase 4: 4-wave LDS reduction, 1 KiB coalesced store
// ------------------------------------------------------------------------------------------
#define AGG_MAX_L 4
#define AGG_MAX_NLP 384  // 12 softmax items per thread
struct AggParams {
  int A, N, S, P, L;
  int H[AGG_MAX_L], W[AGG_MAX_L], start[AGG_MAX_L];
  float pc_lo[3], pc_span[3];
  float pad_w, pad_h;
  int q_per_xcd;
  int out_dt;
  int ldU, ldO;   // row strides (floats) of U and of the key-point offsets
  float ipw, iph;                       // 1 / pad_w, 1 / pad_h
  float Wf[AGG_MAX_L], Hf[AGG_MAX_L];   // level sizes as floats
  // variant 9 (sibling workgroups for heavy queries, round 5): perm holds A main entries + split_extra sibling entries
  float* split_part;                    // [rows][2][256] partial sums of the two workgroups of a split query
  int* split_tick;                      // [rows] arrival tickets, zero at rest
  int split_extra;
};
// What the BATCHED instantiations of kernels 7 and 8 take in AggParams' place (far3d_aggregate_batched_holes): the same fields, then the
// hole of unused query rows.  hole_count: a DEVICE array of one count per sample, never NULL (AGG_SAMPLE_HOLE_COUNT below); sample b's
// rows [hole_start + hole_count[b], hole_end) hold no query.  The one-sample instantiations keep AggParams: their arguments and code do not change.
struct AggParamsBatched : AggParams {
  const int* hole_count;
  int hole_start, hole_end;
};
template <bool BATCHED> using AggParamsOf = std::conditional_t<BATCHED, AggParamsBatched, AggParams>;
#define AGG_SPLIT_FLAG (1 << 29)        // perm entry: this query is handled by two workgroups (set on both of its entries)
#define AGG_SIBLING_FLAG (1 << 30)      // perm entry of the second workgroup (part 1)
#define AGG_ROW_MASK 0x1fffffff
#define AGG_NO_SIBLING 0x7fffffff       // unused sibling slot

// ------------------------------------------------------------------------------------------
// v3 of the fused aggregation (round 1's kernel; kept as variant 3 for A/B).  PMC counters on v1 showed the kernel VALU-bound (2.5k VALU
// instructions per wave, L2 hit 60 %, HBM fetch == the 46 MB of value maps): every lane recomputed wave-uniform sample
// geometry.  v3 computes each visible (camera, point, level) sample ONCE (one thread per camera-point in phase 1), stores a
// 32-byte record {clamped top-left offset, dx, dy, weight row, 4 bilinear weights} in a compacted LDS list (deterministic
// block scan), and the gather loop is reduced to: broadcast record read, 4 coalesced row loads, 16 FMAs -- NB samples in
// flight per wave.  Softmax uses the hardware exp2 path and incremental (camera, logit) indices.
// ------------------------------------------------------------------------------------------
// dynamic LDS of aggregate_v3_kernel: its carve-up (w_s, stat_s, scan_s, rec_s below), in bytes
static inline size_t agg3_lds_bytes(int N, int P, int L) {
  const int NLP = N * P * L;
  return (size_t)(NLP * 8 > 1024 ? NLP * 8 : 1024) * 4 + 64 * 4 + 16 * 4 + (size_t)NLP * 32;
}
template <typename TV, int NB, int RP = 0>   // RP: bf16 row-pair gather (16-byte loads, both bilinear columns per instruction)
__global__ __launch_bounds__(256) void aggregate_v3_kernel(const TV* __restrict__ feat, const float* __restrict__ ref,
                                                           const float* __restrict__ offs, const float* __restrict__ l2i,
                                                           const float* __restrict__ U, const float* __restrict__ Vc,
                                                           const int* __restrict__ perm, void* __restrict__ out, AggParams prm) {
  int a = (blockIdx.x & 7) * prm.q_per_xcd + (blockIdx.x >> 3);
  if (a >= prm.A) return;
  if (perm) a = perm[a];
  if (a < 0) {      // ~a: a row without a query (see far3d_agg_order): zero row
    a = ~a;
    if (prm.out_dt == FAR3D_DT_F32) reinterpret_cast<float*>(out)[(long)a * 256 + threadIdx.x] = 0.f;
    else reinterpret_cast<bf16_t*>(out)[(long)a * 256 + threadIdx.x] = 0;
    return;
  }
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int NP = prm.N * prm.P, NLP = NP * prm.L, J = prm.L * prm.P;
  float* w_s = reinterpret_cast<float*>(smem);                 // [NLP][8] softmax weights; reused as [4][256] reduction buffer
  float* stat_s = w_s + (NLP * 8 > 1024 ? NLP * 8 : 1024);     // [64]
  int* scan_s = reinterpret_cast<int*>(stat_s + 64);           // [16]
  int4* rec_s = reinterpret_cast<int4*>(scan_s + 16);          // [NLP][2] sample records (compacted: only [0, nsamp) are live)
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;

  // ---- phase 1: one thread per (camera, point): projection, per-level geometry (detr3d_transformer.py:524-525,547-552)
  int mask = 0;
  float u = 0.f, v = 0.f;
  int n1 = 0, p1 = 0;
  if (t < NP) {
    n1 = t / prm.P; p1 = t - n1 * prm.P;
    float k[3];
#pragma unroll
    for (int d = 0; d < 3; ++d)
      k[d] = (ref[a * 3 + d] * prm.pc_span[d] + prm.pc_lo[d]) + offs[(long)a * prm.ldO + p1 * 3 + d];
    const float* m = l2i + n1 * 16;
    const float x = m[0] * k[0] + m[1] * k[1] + m[2] * k[2] + m[3];
    const float y = m[4] * k[0] + m[5] * k[1] + m[6] * k[2] + m[7];
    const float z = m[8] * k[0] + m[9] * k[1] + m[10] * k[2] + m[11];
    const float zc = fmaxf(z, 1e-5f);
    u = (x / zc) / prm.pad_w; v = (y / zc) / prm.pad_h;
#pragma unroll
    for (int l = 0; l < AGG_MAX_L; ++l) {
      if (l < prm.L) {
        const float h_im = v * prm.H[l] - 0.5f, w_im = u * prm.W[l] - 0.5f;
        if (h_im > -1.f && w_im > -1.f && h_im < prm.H[l] && w_im < prm.W[l]) mask |= 1 << l;
      }
    }
  }
  // deterministic compaction: exclusive scan of the per-thread visible-level counts
  {
    const int c = __popc(mask);
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int nb = __shfl_up(inc, o);
      if (lane >= o) inc += nb;
    }
    if (lane == 63) scan_s[wv] = inc;
    __syncthreads();
    int base = 0;
    for (int k = 0; k < wv; ++k) base += scan_s[k];
    int pos = base + inc - c;
    if (t == 255) scan_s[4] = base + inc;
#pragma unroll
    for (int l = 0; l < AGG_MAX_L; ++l) {
      if ((mask >> l) & 1) {
        const int Hl = prm.H[l], Wl = prm.W[l];
        const float h_im = v * Hl - 0.5f, w_im = u * Wl - 0.5f;
        const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
        const float lh = h_im - h_low, lw = w_im - w_low;
        const float hh = 1.f - lh, hw = 1.f - lw;
        const bool t_ok = h_low >= 0, b_ok = h_low + 1 <= Hl - 1, l_ok = w_low >= 0, r_ok = w_low + 1 <= Wl - 1;
        const int y0 = t_ok ? h_low : 0, y1 = b_ok ? h_low + 1 : Hl - 1;
        const int x0 = l_ok ? w_low : 0, x1 = r_ok ? w_low + 1 : Wl - 1;
        int4 r0;
        r0.x = ((n1 * prm.S + prm.start[l]) + y0 * Wl + x0) * 256;   // element offset of the (clamped) top-left pixel
        r0.y = (x1 - x0) * 256;                                      // 0 when the right column is clamped away
        r0.z = (y1 - y0) * Wl * 256;
        r0.w = ((n1 * prm.L + l) * prm.P + p1) * 8;                  // row of this sample in w_s
        float4 wq;
        wq.x = (t_ok && l_ok) ? hh * hw : 0.f;
        wq.y = (t_ok && r_ok) ? hh * lw : 0.f;
        wq.z = (b_ok && l_ok) ? lh * hw : 0.f;
        wq.w = (b_ok && r_ok) ? lh * lw : 0.f;
        rec_s[2 * pos] = r0;
        rec_s[2 * pos + 1] = make_int4(__float_as_int(wq.x), __float_as_int(wq.y), __float_as_int(wq.z), __float_as_int(wq.w));
        ++pos;
      }
    }
  }

  // ---- phase 2: softmax over cams x levels x points per group (detr3d_transformer.py:539-540)
  {
    const int gg = t & 7, r = t >> 3;
    float lg[AGG_MAX_NLP / 32];
    float mx = -INFINITY;
    int n = 0, j = r;   // idx = r + 32*i  ->  (camera n, logit j) tracked incrementally (J > 32)
    while (j >= J) { j -= J; ++n; }
    const float* Ua = U + (long)a * prm.ldU + gg;
    const float* Vg = Vc + gg;
#pragma unroll
    for (int i = 0; i < AGG_MAX_NLP / 32; ++i) {
      lg[i] = -INFINITY;
      if (r + 32 * i < NLP) lg[i] = Ua[j * 8] + Vg[(n * J + j) * 8];
      mx = fmaxf(mx, lg[i]);
      j += 32;
      while (j >= J) { j -= J; ++n; }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 8));
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    if (lane < 8) stat_s[wv * 8 + lane] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(stat_s[gg], stat_s[8 + gg]), fmaxf(stat_s[16 + gg], stat_s[24 + gg]));
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < AGG_MAX_NLP / 32; ++i) {
      lg[i] = (r + 32 * i < NLP) ? __expf(lg[i] - mx) : 0.f;
      sum += lg[i];
    }
    sum += __shfl_xor(sum, 8);
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    if (lane < 8) stat_s[32 + wv * 8 + lane] = sum;
    __syncthreads();
    sum = (stat_s[32 + gg] + stat_s[40 + gg]) + (stat_s[48 + gg] + stat_s[56 + gg]);
    const float inv = 1.f / sum;
#pragma unroll
    for (int i = 0; i < AGG_MAX_NLP / 32; ++i) {
      const int idx = r + 32 * i;
      if (idx < NLP) w_s[idx * 8 + gg] = lg[i] * inv;
    }
  }
  __syncthreads();
  const int nsamp = scan_s[4];

  if constexpr (RP != 0 && sizeof(TV) == 2) {
    // ---- phase 3 (bf16): lanes 0-31 take the left bilinear column, lanes 32-63 the right one; a lane owns 8 channels
    // (16 bytes) of its pixel, so one instruction fetches the two adjacent 512-byte token rows of a sample's top (then
    // bottom) tap pair.  Half the load instructions of the 8-byte layout, twice the samples in flight per VGPR; the two
    // column partial sums are added once at the end (the weighted sum is linear).
    typedef unsigned rp_u32x4 __attribute__((ext_vector_type(4)));
    const int l31 = lane & 31, hi = lane >> 5, g = l31 >> 2;
    float a8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a8[k] = 0.f;
    const bf16_t* fb = reinterpret_cast<const bf16_t*>(feat) + l31 * 8;
    for (int b0 = wv; b0 < nsamp; b0 += 4 * NB) {
      rp_u32x4 vt[NB], vb[NB];
      float wt[NB], wb[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int si = b0 + 4 * i;
        const bool ok = si < nsamp;
        const int4 r0 = rec_s[2 * (ok ? si : 0)];
        const int4 r1 = rec_s[2 * (ok ? si : 0) + 1];
        const bf16_t* p = fb + r0.x + (hi ? r0.y : 0);
        vt[i] = *reinterpret_cast<const rp_u32x4*>(p);
        vb[i] = *reinterpret_cast<const rp_u32x4*>(p + r0.z);
        const float aw = ok ? w_s[r0.w + g] : 0.f;
        wt[i] = aw * __int_as_float(hi ? r1.y : r1.x);
        wb[i] = aw * __int_as_float(hi ? r1.w : r1.z);
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          a8[2 * k] += wt[i] * __uint_as_float(vt[i][k] << 16) + wb[i] * __uint_as_float(vb[i][k] << 16);
          a8[2 * k + 1] += wt[i] * __uint_as_float(vt[i][k] & 0xffff0000u) + wb[i] * __uint_as_float(vb[i][k] & 0xffff0000u);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) a8[k] += __shfl_xor(a8[k], 32);
    __syncthreads();
    float* red_s = w_s;
    if (hi == 0) {
      *reinterpret_cast<float4*>(red_s + wv * 256 + l31 * 8) = make_float4(a8[0], a8[1], a8[2], a8[3]);
      *reinterpret_cast<float4*>(red_s + wv * 256 + l31 * 8 + 4) = make_float4(a8[4], a8[5], a8[6], a8[7]);
    }
    __syncthreads();
    const float res = (red_s[t] + red_s[256 + t]) + (red_s[512 + t] + red_s[768 + t]);
    if (prm.out_dt == FAR3D_DT_F32) reinterpret_cast<float*>(out)[(long)a * 256 + t] = res;
    else reinterpret_cast<bf16_t*>(out)[(long)a * 256 + t] = f32_to_bf16(res);
    return;
  }
  // ---- phase 3: gather.  lane = group*8 + chunk (4 channels); a sample = 4 coalesced token-row loads.
  const int g = lane >> 3;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const TV* fbase = feat + lane * 4;
  for (int b0 = wv; b0 < nsamp; b0 += 4 * NB) {
    float4 v1[NB], v2[NB], v3[NB], v4[NB];
    float cw[NB][4];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int si = b0 + 4 * i;
      const bool ok = si < nsamp;
      const int4 r0 = rec_s[2 * (ok ? si : 0)];
      const int4 r1 = rec_s[2 * (ok ? si : 0) + 1];
      const TV* p00 = fbase + r0.x;
      v1[i] = load4(p00);
      v2[i] = load4(p00 + r0.y);
      v3[i] = load4(p00 + r0.z);
      v4[i] = load4(p00 + r0.z + r0.y);
      const float aw = ok ? w_s[r0.w + g] : 0.f;
      cw[i][0] = aw * __int_as_float(r1.x); cw[i][1] = aw * __int_as_float(r1.y);
      cw[i][2] = aw * __int_as_float(r1.z); cw[i][3] = aw * __int_as_float(r1.w);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      acc.x += (cw[i][0] * v1[i].x + cw[i][1] * v2[i].x) + (cw[i][2] * v3[i].x + cw[i][3] * v4[i].x);
      acc.y += (cw[i][0] * v1[i].y + cw[i][1] * v2[i].y) + (cw[i][2] * v3[i].y + cw[i][3] * v4[i].y);
      acc.z += (cw[i][0] * v1[i].z + cw[i][1] * v2[i].z) + (cw[i][2] * v3[i].z + cw[i][3] * v4[i].z);
      acc.w += (cw[i][0] * v1[i].w + cw[i][1] * v2[i].w) + (cw[i][2] * v3[i].w + cw[i][3] * v4[i].w);
    }
  }

  // ---- phase 4: cross-wave (= cross-camera/point) reduction through the (now dead) weight buffer; coalesced store
  __syncthreads();
  float* red_s = w_s;
  *reinterpret_cast<float4*>(red_s + wv * 256 + lane * 4) = acc;
  __syncthreads();
  const float res = (red_s[t] + red_s[256 + t]) + (red_s[512 + t] + red_s[768 + t]);
  if (prm.out_dt == FAR3D_DT_F32) reinterpret_cast<float*>(out)[(long)a * 256 + t] = res;
  else reinterpret_cast<bf16_t*>(out)[(long)a * 256 + t] = f32_to_bf16(res);
}

// ------------------------------------------------------------------------------------------
// Tap-merging aggregation, `aggregate_v7_kernel` (the default of rounds 2-3; variant 7 since v8): two waves per query, no atomics.
//
// Why: the v3 counters (profiles/r1) showed no HBM over-fetch at all -- the kernel sat on (i) ~11 us of block-wide fixed
// phases (3 barriers per query for the scan / softmax statistics) and (ii) L2 -> CU gather volume: every visible sample moved
// 4 x 512 B although the 13 key points of a query land on few distinct tokens (228 bilinear taps -> ~85 distinct rows).
//
// The merge uses the tent form of bilinear interpolation: the weight of the token at integer (tx,ty) for a sample at
// (px,py) is max(0,1-|px-tx|) * max(0,1-|py-ty|) -- exactly the four mmcv corner weights, zero for every other token, and
// tokens outside the map simply do not exist (= zero padding; the `h_im > -1 ...` test of ms_deform_attn is implied).  So for a
// (camera, level) whose 13 points span at most 64 tokens (a pw x ph patch, pw*ph = 64), lane T owns token T of the patch and
// accumulates W[T][g] = sum_p softmax_w[p][g] * tent(p, T) in registers: dense, branch-free, no sort, no atomics.  Tokens with
// a non-zero weight are appended (ballot + mbcnt) to a per-wave LDS list of {row offset, 8 group weights}; a (camera, level)
// whose points spread wider falls back to one list entry per (point, corner).  The gather then walks the list: one 16-byte
// load per lane = two 512-byte bf16 token rows per instruction (one 1-KiB fp32 row), 8 (4) channels per lane, several loads in
// flight.  Same arithmetic as the reference up to fp32 re-association.  The softmax normaliser 1/S[g] is applied ONCE to the
// final sums (every merged weight of group g carries it), so the weights are stored un-normalised.
//
// Two earlier shapes of the same algorithm were measured and removed (git history has them): one wave per query
// (2990 VALU instructions per query but 53 % of the wave cycles in s_waitcnt at ~1.5 waves per SIMD: 28 us vs 22 us for v3) and
// four waves per query with wave = camera (82 VGPRs -> 5 workgroups per CU, a second round of workgroups, one wave building a
// visible camera for ~20k cycles while three wait: 26 us).
// ------------------------------------------------------------------------------------------
#define AGG4_MAX_N 16

typedef float agg_f2 __attribute__((ext_vector_type(2)));
typedef float agg8_f4 __attribute__((ext_vector_type(4)));

template <typename TV, int UNR, int OPT = 0>
__device__ __forceinline__ void agg7_gather(const TV* __restrict__ feat, const int* off_s, const float* wt_s, int cnt, int lane,
                                            float (&acc)[8]) {
  if (cnt <= 0) return;
  if constexpr (sizeof(TV) == 2) {
    typedef unsigned g4_u32x4 __attribute__((ext_vector_type(4)));
    const int l31 = lane & 31, hi = lane >> 5, g = l31 >> 2;
    const bf16_t* fb = reinterpret_cast<const bf16_t*>(feat) + l31 * 8;
    g4_u32x4 va[UNR], vb[UNR];
    float wa[UNR], wb[UNR];
    auto issue = [&](int k0, g4_u32x4 (&v)[UNR], float (&w)[UNR]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < UNR; ++i) {
        const int e = k0 + 2 * i + hi;
        const bool ok = e < cnt;
        v[i] = *reinterpret_cast<const g4_u32x4*>(fb + off_s[ok ? e : 0]);
        w[i] = ok ? wt_s[e * 8 + g] : 0.f;
      }
    };
    auto consume = [&](const g4_u32x4 (&v)[UNR], const float (&w)[UNR]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < UNR; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if constexpr (OPT) {          // one v_pk_fma_f32 per bf16 pair
            const agg_f2 x = {__uint_as_float(v[i][k] << 16), __uint_as_float(v[i][k] & 0xffff0000u)};
            agg_f2 a = {acc[2 * k], acc[2 * k + 1]};
            a = x * w[i] + a;
            acc[2 * k] = a.x; acc[2 * k + 1] = a.y;
          } else {
            acc[2 * k] += w[i] * __uint_as_float(v[i][k] << 16);
            acc[2 * k + 1] += w[i] * __uint_as_float(v[i][k] & 0xffff0000u);
          }
        }
      }
    };
    issue(0, va, wa);
    for (int k0 = 2 * UNR; ; k0 += 4 * UNR) {
      if (k0 < cnt) issue(k0, vb, wb);
      consume(va, wa);
      if (k0 >= cnt) break;
      if (k0 + 2 * UNR < cnt) issue(k0 + 2 * UNR, va, wa);
      consume(vb, wb);
      if (k0 + 2 * UNR >= cnt) break;
    }
  } else {
    const int g = lane >> 3;
    const float* fb = reinterpret_cast<const float*>(feat) + lane * 4;
    float4 va[UNR], vb[UNR];
    float wa[UNR], wb[UNR];
    auto issue = [&](int k0, float4 (&v)[UNR], float (&w)[UNR]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < UNR; ++i) {
        const int e = k0 + i;
        const bool ok = e < cnt;
        v[i] = *reinterpret_cast<const float4*>(fb + off_s[ok ? e : 0]);
        w[i] = ok ? wt_s[e * 8 + g] : 0.f;
      }
    };
    auto consume = [&](const float4 (&v)[UNR], const float (&w)[UNR]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < UNR; ++i) {
        acc[0] += w[i] * v[i].x; acc[1] += w[i] * v[i].y; acc[2] += w[i] * v[i].z; acc[3] += w[i] * v[i].w;
      }
    };
    issue(0, va, wa);
    for (int k0 = UNR; ; k0 += 2 * UNR) {
      if (k0 < cnt) issue(k0, vb, wb);
      consume(va, wa);
      if (k0 >= cnt) break;
      if (k0 + UNR < cnt) issue(k0 + UNR, va, wa);
      consume(vb, wb);
      if (k0 + UNR >= cnt) break;
    }
  }
}

// ---- cross-lane reductions on the VALU (variant 11): DPP quad_perm / row_ror inside a 16-lane row, v_permlane16_swap /
// v_permlane32_swap across rows -- instead of __shfl_xor, which compiles to a dependent ds_bpermute round trip through the LDS pipe
template <int CTRL> __device__ __forceinline__ float agg_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// lane i <- v[i ^ 16] (within each 32-lane half) / v[i ^ 32]: returns the two sides for a commutative combine
__device__ __forceinline__ void agg_swap16(float v, float& a, float& b) {
  typedef unsigned u2_t __attribute__((ext_vector_type(2)));
  const unsigned x = __builtin_bit_cast(unsigned, v);
  const u2_t r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
  const unsigned rx = r.x, ry = r.y;      // (bit-casting a vector ELEMENT reads element 0 both times: go through scalars)
  a = __uint_as_float(rx); b = __uint_as_float(ry);
}
__device__ __forceinline__ void agg_swap32(float v, float& a, float& b) {
  typedef unsigned u2_t __attribute__((ext_vector_type(2)));
  const unsigned x = __builtin_bit_cast(unsigned, v);
  const u2_t r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  const unsigned rx = r.x, ry = r.y;
  a = __uint_as_float(rx); b = __uint_as_float(ry);
}
// reductions over the lanes of a wave that share (lane & 1): quad xor 2, row rotations by 4 and 8 (parity preserving), then rows
struct AggMax { static __device__ __forceinline__ float op(float a, float b) { return fmaxf(a, b); } };
struct AggMin { static __device__ __forceinline__ float op(float a, float b) { return fminf(a, b); } };
struct AggSum { static __device__ __forceinline__ float op(float a, float b) { return a + b; } };
// One-instruction DPP steps (v8): v_min/max/add_f32_dpp read the permuted operand directly.  Through __builtin_amdgcn_update_dpp
// the compiler emits v_mov_dpp + a canonicalising v_max + the operation.  The two wait states a DPP read needs after a VALU
// write of its source are inside the string (hipcc pads nothing inside an asm statement).
#define AGG_DPP1(NAME, INSTR, CTRL)                                                                   \
  __device__ __forceinline__ float NAME(float v) {                                                    \
    float r;                                                                                          \
    asm("s_nop 1\n\t" INSTR " %0, %1, %1 " CTRL " row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v));  \
    return r;                                                                                         \
  }
AGG_DPP1(agg_min_q1, "v_min_f32_dpp", "quad_perm:[1,0,3,2]")
AGG_DPP1(agg_min_q2, "v_min_f32_dpp", "quad_perm:[2,3,0,1]")
AGG_DPP1(agg_min_r4, "v_min_f32_dpp", "row_ror:4")
AGG_DPP1(agg_min_r8, "v_min_f32_dpp", "row_ror:8")
AGG_DPP1(agg_max_q1, "v_max_f32_dpp", "quad_perm:[1,0,3,2]")
AGG_DPP1(agg_max_q2, "v_max_f32_dpp", "quad_perm:[2,3,0,1]")
AGG_DPP1(agg_max_r4, "v_max_f32_dpp", "row_ror:4")
AGG_DPP1(agg_max_r8, "v_max_f32_dpp", "row_ror:8")
AGG_DPP1(agg_add_q2, "v_add_f32_dpp", "quad_perm:[2,3,0,1]")
AGG_DPP1(agg_add_r4, "v_add_f32_dpp", "row_ror:4")
AGG_DPP1(agg_add_r8, "v_add_f32_dpp", "row_ror:8")
template <int CTRL> __device__ __forceinline__ int agg8_dpp_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
__device__ __forceinline__ int agg8_wave_sum_i32(int v) {      // over all 64 lanes, every lane gets it
  typedef unsigned u2_t __attribute__((ext_vector_type(2)));
  v += agg8_dpp_i32<0xB1>(v);       // quad_perm:[1,0,3,2]
  v += agg8_dpp_i32<0x4E>(v);       // quad_perm:[2,3,0,1]
  v += agg8_dpp_i32<0x124>(v);      // row_ror:4
  v += agg8_dpp_i32<0x128>(v);      // row_ror:8
  u2_t q = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
  unsigned qx = q.x, qy = q.y;
  v = (int)(qx + qy);
  q = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
  qx = q.x; qy = q.y;
  return (int)(qx + qy);
}
// value of lane K of the caller's 16-lane row, in every lane of the row (v_mov_b32_dpp row_newbcast:K)
template <int K> __device__ __forceinline__ float agg8_row_bcast(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x150 + K, 0xf, 0xf, false));
}
template <int K> __device__ __forceinline__ float4 agg8_row_bcast4(const float4& v) {
  return make_float4(agg8_row_bcast<K>(v.x), agg8_row_bcast<K>(v.y), agg8_row_bcast<K>(v.z), agg8_row_bcast<K>(v.w));
}
__device__ __forceinline__ float agg8_row_min(float v) { return agg_min_r8(agg_min_r4(agg_min_q2(agg_min_q1(v)))); }     // all 16 lanes of a row
__device__ __forceinline__ float agg8_row_max(float v) { return agg_max_r8(agg_max_r4(agg_max_q2(agg_max_q1(v)))); }
__device__ __forceinline__ float agg8_wave_max_parity(float v) {      // over the 32 lanes of a wave with equal (lane & 1)
  v = agg_max_r8(agg_max_r4(agg_max_q2(v)));
  float a, b;
  agg_swap16(v, a, b); v = fmaxf(a, b);
  agg_swap32(v, a, b); return fmaxf(a, b);
}
__device__ __forceinline__ float agg8_wave_sum_parity(float v) {
  v = agg_add_r8(agg_add_r4(agg_add_q2(v)));
  float a, b;
  agg_swap16(v, a, b); v = a + b;
  agg_swap32(v, a, b); return a + b;
}

template <typename OP> __device__ __forceinline__ float agg_row_reduce_parity(float v) {     // over the 8 same-parity lanes of a 16-lane row
  v = OP::op(v, agg_dpp<0x4E>(v));       // quad_perm [2,3,0,1]
  v = OP::op(v, agg_dpp<0x124>(v));      // row_ror:4
  v = OP::op(v, agg_dpp<0x128>(v));      // row_ror:8
  return v;
}
template <typename OP> __device__ __forceinline__ float agg_wave_reduce_parity(float v) {
  v = agg_row_reduce_parity<OP>(v);
  float a, b;
  agg_swap16(v, a, b); v = OP::op(a, b);
  agg_swap32(v, a, b); v = OP::op(a, b);
  return v;
}
template <typename OP> __device__ __forceinline__ float agg_row_reduce(float v) {            // over all 16 lanes of a row
  v = OP::op(v, agg_dpp<0xB1>(v));       // quad_perm [1,0,3,2]
  return agg_row_reduce_parity<OP>(v);
}

__device__ __forceinline__ int agg4_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

#ifdef FAR3D_PROFILING
// tools/agg_phase_times.py: per-wave s_memtime stamps at the phase boundaries of the kernel (never in libfar3d_hip.so)
__device__ long long* g_agg_ts = nullptr;
extern "C" int far3d_prof_set_agg_timestamps(long long* buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_agg_ts), &buf, sizeof(buf)) == hipSuccess ? 0 : -2;
}
#define AGG_TS(i) do { if (g_agg_ts && lane == 0) g_agg_ts[((long)blockIdx.x * 4 + wv) * 16 + (i)] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#else
#define AGG_TS(i) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------
// v7: TWO waves per query, wave 0 owns pyramid levels 0 and 3, wave 1 levels 1 and 2 (64-token patches).
//
// 128 threads per query -> 8 workgroups per CU at 120 VGPRs (every query of a frame resident in one round), both waves build
// (2 levels each, lane = token of a 64-token patch, so only spreads > 64 tokens fall back to per-corner entries), and
// invisible (camera, level) pairs cost nothing: the projection phase leaves a per-camera level-visibility mask and the build
// loop walks its set bits.  Barriers: B1 maxima, B2 sums, B3 cross-wave reduction.
// ------------------------------------------------------------------------------------------
#define AGG7_CAPW 128     // list entries per wave between flushes (2 x 128 x 36 B; 7 workgroups of 22.1 KB fit a CU's 160 KB)

// OPT 1 (variant 11): VALU reductions, early matrix loads, packed FMAs.
// Measured and removed this round (profiles/r3): a scatter-add tap merge through LDS float atomics (52 lanes add their
// 8 group weights into per-token accumulators, ~100 instead of ~340 VALU instructions per patch: build phase 2.2x SLOWER, 35 us per
// launch); patches of 65..128 tokens merged in two passes instead of the per-corner fallback (78 instead of 92 rows per query, but
// 23.2 vs 21.2 us); three / four waves per query with one shared, evenly split work list (24.1 .. 28.3 us).
//
// BATCHED (far3d_aggregate_batched; kernels 7 and 8): a batch of samples in one launch.  A workgroup is still one query of one sample and
// nothing in it knows about the others: the sample is a second index that moves the operand bases, and the body behind the bases is the
// one-sample code, so out[b] has the bits of the one-sample launch on sample b.  The sample is blockIdx.y and gridDim.x stays
// 8 * q_per_xcd: workgroups are dispatched in linear order (x fastest) round-robin over the 8 XCDs, so with gridDim.x a multiple of 8
// `blockIdx.x & 7` still names the blocks that share an XCD and a sample's queries keep the placement of the one-sample launch
// (flattening B * A through q_per_xcd needs a division per workgroup to find the sample and makes the placement a function of B; it
// was not measured).  Placement is a speed heuristic only; no result depends on it.  The per-sample extents are formed in 64 bits
// (B * N * S * C may pass 2^31); inside a sample the 32-bit offsets stay.  No kernel argument is added: the extents come from AggParams,
// and the one-sample instantiations (BATCHED = false) never look at blockIdx.y.  The batched instantiations take AggParamsBatched in
// AggParams' place: the same fields, then the hole of unused query rows per sample (far3d_aggregate_batched_holes, below).
#define AGG_SAMPLE_BASES(b)                                                                                                       \
  do {                                                                                                                            \
    feat += (b) * prm.N * prm.S * 256; ref += (b) * prm.A * 3; offs += (b) * prm.A * prm.ldO; U += (b) * prm.A * prm.ldU;          \
    l2i += (b) * prm.N * 16;                                                                                                      \
    out = reinterpret_cast<char*>(out) + (b) * prm.A * 256 * (prm.out_dt == FAR3D_DT_F32 ? 4 : 2);                                \
  } while (0)
// The hole of a batched launch (AggParamsBatched).  AGG_SAMPLE_HOLE_COUNT fetches the sample's count: one scalar load, uniform per
// workgroup, issued with the query-independent loads at the top of the kernel.  It stands under no branch and behind no select -- a value
// loaded inside a branch is waited for inside it, a round trip in front of the whole load burst -- so the host never passes NULL: without
// a hole the pointer names B readable words of an operand the kernel reads anyway and the hole is the empty [0, 0).  AGG_SAMPLE_HOLE,
// where the slot's row is decided, clamps the count into [0, hole_end - hole_start] and turns slot a0 into ~a0 when it lies in
// [hole_start + count, hole_end); the kernel's own hole exit (the one a perm entry ~a takes) does the rest.
#define AGG_SAMPLE_HOLE_COUNT(b) (prm.hole_count[b])
#define AGG_SAMPLE_HOLE(a, a0, cnt)                                                                                               \
  do {                                                                                                                            \
    const int lo_ = prm.hole_start + min(max(cnt, 0), prm.hole_end - prm.hole_start);                                             \
    if ((a0) >= lo_ && (a0) < prm.hole_end) a = ~(a0);                                                                            \
  } while (0)
// The ends of the two-wave kernels (7, 8, the gather half of variant 13), one definition each.  They are function-like macros with every
// name passed in, not functions: the text reaches the compiler as if written out in the kernel, so the kernels' machine code is what it
// was with three copies (profiles/agg_host/README.md).  Thread t owns channels c = 2t, 2t + 1 of output row a.
//  * AGG_ZERO_ROW2: the row of a slot without a query (perm entry ~a, far3d_agg_order): zeros, no work.
//  * AGG_STORE_ROW2: the finished pair (r0, r1) in the output's type.
//  * AGG_WAVE_PARTIALS: a wave's 256 partial sums into `red` ahead of the cross-wave barrier; on bf16 rows a load fetched two token rows,
//    so the lane halves are added first.  HALVES is how the kernel adds them: kernel 7 with a shuffle, kernel 8 with its permlane swap.
#define AGG_STORE_ROW2(out, out_dt, a, c, r0, r1)                                                                                         \
  do {                                                                                                                                    \
    if ((out_dt) == FAR3D_DT_F32) *reinterpret_cast<float2*>(reinterpret_cast<float*>(out) + (long)(a) * 256 + (c)) = make_float2(r0, r1); \
    else *reinterpret_cast<unsigned*>(reinterpret_cast<bf16_t*>(out) + (long)(a) * 256 + (c)) = pack_bf16x2(r0, r1);                        \
  } while (0)
#define AGG_ZERO_ROW2(out, out_dt, a, c) AGG_STORE_ROW2(out, out_dt, a, c, 0.f, 0.f)
#define AGG_HALVES_SHFL(v) v += __shfl_xor(v, 32)
#define AGG_HALVES_SWAP(v) do { float x, y; agg_swap32(v, x, y); v = x + y; } while (0)
#define AGG_WAVE_PARTIALS(TV, red, acc, lane, HALVES)                                                                                     \
  do {                                                                                                                                    \
    if constexpr (sizeof(TV) == 2) {                                                                                                      \
      _Pragma("unroll") for (int k = 0; k < 8; ++k) HALVES(acc[k]);                                                                       \
      if (lane < 32) {                                                                                                                    \
        *reinterpret_cast<float4*>(red + lane * 8) = make_float4(acc[0], acc[1], acc[2], acc[3]);                                         \
        *reinterpret_cast<float4*>(red + lane * 8 + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);                                     \
      }                                                                                                                                   \
    } else {                                                                                                                              \
      *reinterpret_cast<float4*>(red + lane * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);                                           \
    }                                                                                                                                     \
  } while (0)
// dynamic LDS of aggregate_v7_kernel at CAPW = AGG7_CAPW: its carve-up (w_s .. wt_all below), in bytes
static inline size_t agg7_lds_bytes(int N, int P, int L) {
  const int NP = N * P;
  return (size_t)NP * L * 32 + (size_t)((NP + 1) & ~1) * 8 + AGG4_MAX_N * 16 + 32 * 4 + AGG4_MAX_N * 4 + (size_t)2 * AGG7_CAPW * 36;
}
template <typename TV, int PT, int OPT = 0, int CAPW = AGG7_CAPW, bool BATCHED = false>
__global__ __launch_bounds__(128) void aggregate_v7_kernel(const TV* __restrict__ feat, const float* __restrict__ ref,
                                                           const float* __restrict__ offs, const float* __restrict__ l2i,
                                                           const float* __restrict__ U, const float* __restrict__ Vc,
                                                           const int* __restrict__ perm, void* __restrict__ out, AggParamsOf<BATCHED> prm) {
  const int a0 = (blockIdx.x & 7) * prm.q_per_xcd + (blockIdx.x >> 3);
  if (a0 >= prm.A) return;
  int a = a0;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);   // wave index: scalar
  const int P = PT ? PT : prm.P, L = prm.L, N = prm.N;
  const int NP = N * P, J = L * P, NLP = NP * L;
  [[maybe_unused]] int hole_cnt = 0;
  if constexpr (BATCHED) {
    const long b = blockIdx.y;
    hole_cnt = AGG_SAMPLE_HOLE_COUNT(b);      // first: its pointer comes with the kernel's first argument loads, its value with the burst
    AGG_SAMPLE_BASES(b);
    Vc += b * N * (J * 8);
  }
  float* w_s = reinterpret_cast<float*>(smem);                            // [NLP][8] exp(logit - max): UN-normalised weights
  float2* uv_s = reinterpret_cast<float2*>(w_s + NLP * 8);                // [NP] normalised image coordinates
  float4* bb_s = reinterpret_cast<float4*>(uv_s + ((NP + 1) & ~1));       // [AGG4_MAX_N] (umin, umax, vmin, vmax) per camera
  float* stat_s = reinterpret_cast<float*>(bb_s + AGG4_MAX_N);            // [2][2][8]: per-wave max, per-wave sum, by group
  int* vis_s = reinterpret_cast<int*>(stat_s + 32);                       // [AGG4_MAX_N] bit l: level l of the camera is touched
  int* off_all = vis_s + AGG4_MAX_N;                                      // [2][CAPW] row offsets, then [2][CAPW][8] weights
  float* wt_all = reinterpret_cast<float*>(off_all + 2 * CAPW);
  int* off_s = off_all + wv * CAPW;
  float* wt_s = wt_all + wv * CAPW * 8;

  AGG_TS(0);
  // ---- logits (float4 index i4 covers groups (i4&1)*4..+3 of one (camera, level*P+point) row); loads issued first
  constexpr int NV = AGG_MAX_NLP * 2 / 128;     // 6 float4 per thread
  const int n4 = NLP * 2, J2 = J * 2;
  float4 lg[NV];
  // the camera part of the logits does not depend on the query: its loads go out before the (dependent) perm lookup returns
  {
    const float4* V4 = reinterpret_cast<const float4*>(Vc);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int i4 = i * 128 + t;
      lg[i] = i4 < n4 ? V4[i4] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    }
  }
  // OPT: the projection matrix of this lane's camera does not depend on the query either: loaded before the perm lookup returns
  float4 pm0 = make_float4(0.f, 0.f, 0.f, 0.f), pm1 = pm0, pm2 = pm0;
  if constexpr ((OPT & 1) != 0 && PT >= 1 && PT <= 16) {
    if ((t >> 4) < N) {
      const float4* m = reinterpret_cast<const float4*>(l2i + (t >> 4) * 16);
      pm0 = m[0]; pm1 = m[1]; pm2 = m[2];
    }
  }
  if (perm) a = perm[a0];
  if constexpr (BATCHED) AGG_SAMPLE_HOLE(a, a0, hole_cnt);
  if (a < 0) {      // ~a: row a holds no query (far3d_agg_order marks the hole of the fixed-capacity proposal mode): zero row, no work
    a = ~a;
    const int c = t * 2;
    AGG_ZERO_ROW2(out, prm.out_dt, a, c);
    return;
  }
  // query-dependent loads, all issued together: reference point, this lane's key-point offset, the query part of the logits
  const float rf0 = ref[a * 3], rf1 = ref[a * 3 + 1], rf2 = ref[a * 3 + 2];
  float of0 = 0.f, of1 = 0.f, of2 = 0.f;
  if constexpr (PT >= 1 && PT <= 16) {
    if ((t & 15) < P) { const float* o = offs + (long)a * prm.ldO + (t & 15) * 3; of0 = o[0]; of1 = o[1]; of2 = o[2]; }
  }
  {
    int cam = t / J2, rem = t - cam * J2;
    const float4* U4 = reinterpret_cast<const float4*>(U + (long)a * prm.ldU);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int i4 = i * 128 + t;
      if (i4 < n4) {
        const float4 u = U4[rem];
        lg[i] = make_float4(lg[i].x + u.x, lg[i].y + u.y, lg[i].z + u.z, lg[i].w + u.w);
      }
      rem += 128;
      while (rem >= J2) { rem -= J2; ++cam; }
    }
  }

  AGG_TS(8);
  // ---- projection (detr3d_transformer.py:524-525,547-552), per-camera bounding box and level-visibility mask
  {
    const float r0 = rf0 * prm.pc_span[0] + prm.pc_lo[0], r1 = rf1 * prm.pc_span[1] + prm.pc_lo[1], r2 = rf2 * prm.pc_span[2] + prm.pc_lo[2];
    auto project3 = [&](int n, float k0, float k1, float k2, float& u, float& v) __attribute__((always_inline)) {
      const float* m = l2i + n * 16;
      const float x = m[0] * k0 + m[1] * k1 + m[2] * k2 + m[3];
      const float y = m[4] * k0 + m[5] * k1 + m[6] * k2 + m[7];
      const float z = m[8] * k0 + m[9] * k1 + m[10] * k2 + m[11];
      const float zc = fmaxf(z, 1e-5f);
      u = (x / zc) / prm.pad_w; v = (y / zc) / prm.pad_h;
    };
    auto level_mask = [&](float umin, float umax, float vmin, float vmax) __attribute__((always_inline)) {
      int m = 0;
#pragma unroll
      for (int l = 0; l < AGG_MAX_L; ++l) {
        const float Wf = (float)prm.W[l], Hf = (float)prm.H[l];
        const float fx0 = fmaxf(floorf(umin * Wf - 0.5f), 0.f), fx1 = fminf(floorf(umax * Wf - 0.5f) + 1.f, Wf - 1.f);
        const float fy0 = fmaxf(floorf(vmin * Hf - 0.5f), 0.f), fy1 = fminf(floorf(vmax * Hf - 0.5f) + 1.f, Hf - 1.f);
        if (l < L && fx1 >= fx0 && fy1 >= fy0) m |= 1 << l;     // false for NaN / empty
      }
      return m;
    };
    if constexpr (PT >= 1 && PT <= 16) {          // 8 cameras x 16 lanes per pass
      for (int c0 = 0; c0 < N; c0 += 8) {
        const int n = c0 + (t >> 4), p = t & 15;
        const bool act = n < N && p < P;
        float u = 0.f, v = 0.f;
        if (act) {
          if ((OPT & 1) != 0 && c0 == 0) {     // matrices already in registers
            const float k0 = r0 + of0, k1 = r1 + of1, k2 = r2 + of2;
            const float x = pm0.x * k0 + pm0.y * k1 + pm0.z * k2 + pm0.w;
            const float y = pm1.x * k0 + pm1.y * k1 + pm1.z * k2 + pm1.w;
            const float z = pm2.x * k0 + pm2.y * k1 + pm2.z * k2 + pm2.w;
            const float zc = fmaxf(z, 1e-5f);
            u = (x / zc) / prm.pad_w; v = (y / zc) / prm.pad_h;
          } else {
            project3(n, r0 + of0, r1 + of1, r2 + of2, u, v);
          }
          uv_s[n * P + p] = make_float2(u, v);
        }
        float umin = act ? u : INFINITY, umax = act ? u : -INFINITY, vmin = act ? v : INFINITY, vmax = act ? v : -INFINITY;
        if constexpr (OPT) {
          umin = agg_row_reduce<AggMin>(umin); umax = agg_row_reduce<AggMax>(umax);
          vmin = agg_row_reduce<AggMin>(vmin); vmax = agg_row_reduce<AggMax>(vmax);
        } else {
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) {
            umin = fminf(umin, __shfl_xor(umin, o)); umax = fmaxf(umax, __shfl_xor(umax, o));
            vmin = fminf(vmin, __shfl_xor(vmin, o)); vmax = fmaxf(vmax, __shfl_xor(vmax, o));
          }
        }
        if (p == 0 && n < N) {
          bb_s[n] = make_float4(umin, umax, vmin, vmax);
          vis_s[n] = level_mask(umin, umax, vmin, vmax);
        }
      }
    } else {
      for (int idx = t; idx < NP; idx += 128) {
        const int n = idx / P, p = idx - n * P;
        const float* o = offs + (long)a * prm.ldO + p * 3;
        float u, v;
        project3(n, r0 + o[0], r1 + o[1], r2 + o[2], u, v);
        uv_s[idx] = make_float2(u, v);
      }
      __syncthreads();
      if (t < N) {
        float umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
        for (int p = 0; p < P; ++p) {
          const float2 q = uv_s[t * P + p];
          umin = fminf(umin, q.x); umax = fmaxf(umax, q.x);
          vmin = fminf(vmin, q.y); vmax = fmaxf(vmax, q.y);
        }
        bb_s[t] = make_float4(umin, umax, vmin, vmax);
        vis_s[t] = level_mask(umin, umax, vmin, vmax);
      }
    }
  }

  AGG_TS(9);
  // ---- softmax statistics (detr3d_transformer.py:539-540): wave-local by shuffles, across the two waves through LDS
  const int gh = (lane & 1) * 4;          // this lane's 4 groups
  {
    float4 mx = lg[0];
#pragma unroll
    for (int i = 1; i < NV; ++i) {
      mx.x = fmaxf(mx.x, lg[i].x); mx.y = fmaxf(mx.y, lg[i].y); mx.z = fmaxf(mx.z, lg[i].z); mx.w = fmaxf(mx.w, lg[i].w);
    }
    if constexpr (OPT) {
      mx.x = agg_wave_reduce_parity<AggMax>(mx.x); mx.y = agg_wave_reduce_parity<AggMax>(mx.y);
      mx.z = agg_wave_reduce_parity<AggMax>(mx.z); mx.w = agg_wave_reduce_parity<AggMax>(mx.w);
    } else {
#pragma unroll
      for (int o = 2; o < 64; o <<= 1) {      // lanes with equal (lane & 1) hold the same 4 groups
        mx.x = fmaxf(mx.x, __shfl_xor(mx.x, o)); mx.y = fmaxf(mx.y, __shfl_xor(mx.y, o));
        mx.z = fmaxf(mx.z, __shfl_xor(mx.z, o)); mx.w = fmaxf(mx.w, __shfl_xor(mx.w, o));
      }
    }
    if (lane < 2) *reinterpret_cast<float4*>(stat_s + wv * 8 + gh) = mx;
  }
  AGG_TS(1);
  __syncthreads();                                                                        // B1: maxima, uv_s, bb_s, vis_s
  AGG_TS(2);
  {
    const float4 m0 = *reinterpret_cast<const float4*>(stat_s + gh), m1 = *reinterpret_cast<const float4*>(stat_s + 8 + gh);
    const float4 mx = make_float4(fmaxf(m0.x, m1.x), fmaxf(m0.y, m1.y), fmaxf(m0.z, m1.z), fmaxf(m0.w, m1.w));
    float4 sm = make_float4(0.f, 0.f, 0.f, 0.f);
    float4* w4 = reinterpret_cast<float4*>(w_s);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int i4 = i * 128 + t;
      if (i4 < n4) {
        const float4 e = make_float4(__expf(lg[i].x - mx.x), __expf(lg[i].y - mx.y), __expf(lg[i].z - mx.z), __expf(lg[i].w - mx.w));
        sm.x += e.x; sm.y += e.y; sm.z += e.z; sm.w += e.w;
        w4[i4] = e;
      }
    }
    if constexpr (OPT) {
      sm.x = agg_wave_reduce_parity<AggSum>(sm.x); sm.y = agg_wave_reduce_parity<AggSum>(sm.y);
      sm.z = agg_wave_reduce_parity<AggSum>(sm.z); sm.w = agg_wave_reduce_parity<AggSum>(sm.w);
    } else {
#pragma unroll
      for (int o = 2; o < 64; o <<= 1) {
        sm.x += __shfl_xor(sm.x, o); sm.y += __shfl_xor(sm.y, o); sm.z += __shfl_xor(sm.z, o); sm.w += __shfl_xor(sm.w, o);
      }
    }
    if (lane < 2) *reinterpret_cast<float4*>(stat_s + 16 + wv * 8 + gh) = sm;
  }
  __syncthreads();                                                                        // B2: weights, sums
  AGG_TS(3);

  // ---- per wave: levels wv, wv+2 of every camera that touches them -> merged row list -> gather
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  int cnt = 0;
  auto append = [&](bool hit, int off, const float (&wa)[8]) __attribute__((always_inline)) {
    const unsigned long long m = __ballot(hit);
    const int c = __popcll(m);
    if (cnt + c > CAPW) {                 // wave-uniform; the list is private to the wave (LDS is in order per wave)
      agg7_gather<TV, 4, OPT>(feat, off_s, wt_s, cnt, lane, acc);
      cnt = 0;
    }
    if (hit) {
      const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
      off_s[pos] = off;
      *reinterpret_cast<float4*>(wt_s + pos * 8) = make_float4(wa[0], wa[1], wa[2], wa[3]);
      *reinterpret_cast<float4*>(wt_s + pos * 8 + 4) = make_float4(wa[4], wa[5], wa[6], wa[7]);
    }
    cnt += c;
  };
  const int myvis = lane < N ? vis_s[lane] : 0;
  for (int l = 0; l < L; ++l) {
    if (((l ^ (l >> 1)) & 1) != wv) continue;       // wave 0: levels 0, 3; wave 1: levels 1, 2 (finest + coarsest together)
    const int Wl = prm.W[l], Hl = prm.H[l];
    const float Wf = (float)Wl, Hf = (float)Hl;
    unsigned long long cams = __ballot((myvis >> l) & 1);          // cameras whose points touch level l: walk the set bits
    while (cams) {
      const int n = __builtin_ctzll(cams);
      cams &= cams - 1ull;
      const float4 bb = bb_s[n];
      const float fx0 = fmaxf(floorf(bb.x * Wf - 0.5f), 0.f), fx1 = fminf(floorf(bb.y * Wf - 0.5f) + 1.f, Wf - 1.f);
      const float fy0 = fmaxf(floorf(bb.z * Hf - 0.5f), 0.f), fy1 = fminf(floorf(bb.w * Hf - 0.5f) + 1.f, Hf - 1.f);
      const int x0 = (int)fx0, y0 = (int)fy0, spanx = (int)(fx1 - fx0) + 1, spany = (int)(fy1 - fy0) + 1;   // wave-uniform values
      const int lw = (spanx > 1) + (spanx > 2) + (spanx > 4) + (spanx > 8) + (spanx > 16) + (spanx > 32);   // 1 << lw >= spanx
      const int rowbase = n * prm.S + prm.start[l];
      const float* wrow = w_s + ((n * L + l) * P) * 8;
      if (agg4_uni((spanx <= 64 && spany <= (64 >> lw)) ? 1 : 0)) {
        // -- patch: lane T owns token (x0 + T % pw, y0 + T / pw) and merges the P points' corner weights onto it (tent form)
        const int tx = x0 + (lane & ((1 << lw) - 1)), ty = y0 + (lane >> lw);
        const bool active = tx < x0 + spanx && ty < y0 + spany;
        const float ftx = (float)tx, fty = (float)ty;
        float wa[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) wa[k] = 0.f;
        float any = 0.f;
#pragma unroll 4
        for (int p = 0; p < P; ++p) {
          const float2 q = uv_s[n * P + p];
          const float px = q.x * Wf - 0.5f, py = q.y * Hf - 0.5f;
          const float w = fmaxf(1.f - fabsf(px - ftx), 0.f) * fmaxf(1.f - fabsf(py - fty), 0.f);
          const float4 a0 = *reinterpret_cast<const float4*>(wrow + p * 8), a1 = *reinterpret_cast<const float4*>(wrow + p * 8 + 4);
          any = fmaxf(any, w);
          if constexpr (OPT) {            // four v_pk_fma_f32 instead of eight v_fma_f32
            const agg_f2 b0 = {a0.x, a0.y}, b1 = {a0.z, a0.w}, b2 = {a1.x, a1.y}, b3 = {a1.z, a1.w};
            agg_f2 c0 = {wa[0], wa[1]}, c1 = {wa[2], wa[3]}, c2 = {wa[4], wa[5]}, c3 = {wa[6], wa[7]};
            c0 = b0 * w + c0; c1 = b1 * w + c1; c2 = b2 * w + c2; c3 = b3 * w + c3;
            wa[0] = c0.x; wa[1] = c0.y; wa[2] = c1.x; wa[3] = c1.y; wa[4] = c2.x; wa[5] = c2.y; wa[6] = c3.x; wa[7] = c3.y;
          } else {
            wa[0] += w * a0.x; wa[1] += w * a0.y; wa[2] += w * a0.z; wa[3] += w * a0.w;
            wa[4] += w * a1.x; wa[5] += w * a1.y; wa[6] += w * a1.z; wa[7] += w * a1.w;
          }
        }
        append(active && any > 0.f, (rowbase + ty * Wl + tx) * 256, wa);
      } else {
        // -- spread wider than 64 tokens: one entry per (point, corner), mmcv's bilinear arithmetic as is
        for (int i0 = 0; i0 < P * 4; i0 += 64) {
          const int idx = i0 + lane;
          bool hit = false;
          int off = 0;
          float wa[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) wa[k] = 0.f;
          if (idx < P * 4) {
            const int p = idx >> 2, tap = idx & 3;
            const float2 q = uv_s[n * P + p];
            const float h_im = q.y * Hf - 0.5f, w_im = q.x * Wf - 0.5f;
            if (h_im > -1.f && w_im > -1.f && h_im < Hf && w_im < Wf) {
              const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
              const float lh = h_im - h_low, lw_ = w_im - w_low;
              const int ty = h_low + (tap >> 1), tx = w_low + (tap & 1);
              const float bw = ((tap >> 1) ? lh : 1.f - lh) * ((tap & 1) ? lw_ : 1.f - lw_);
              hit = ty >= 0 && ty <= Hl - 1 && tx >= 0 && tx <= Wl - 1 && bw != 0.f;
              off = (rowbase + ty * Wl + tx) * 256;
              const float4 a0 = *reinterpret_cast<const float4*>(wrow + p * 8), a1 = *reinterpret_cast<const float4*>(wrow + p * 8 + 4);
              wa[0] = bw * a0.x; wa[1] = bw * a0.y; wa[2] = bw * a0.z; wa[3] = bw * a0.w;
              wa[4] = bw * a1.x; wa[5] = bw * a1.y; wa[6] = bw * a1.z; wa[7] = bw * a1.w;
            }
          }
          append(hit, off, wa);
        }
      }
    }
  }
  AGG_TS(4);
  agg7_gather<TV, 4, OPT>(feat, off_s, wt_s, cnt, lane, acc);
  AGG_TS(5);
#ifdef FAR3D_PROFILING
  if (g_agg_ts && lane == 0) g_agg_ts[((long)blockIdx.x * 4 + wv) * 16 + 7] = cnt;
#endif

  // ---- cross-wave sum: partial sums go into the wave's own (now dead) list region; 1/S[g] applied once here
  float* red = wt_s;                       // 256 floats: CAPW * 8 >= 256
  AGG_WAVE_PARTIALS(TV, red, acc, lane, AGG_HALVES_SHFL);
  __syncthreads();                                                                        // B3
  AGG_TS(6);
  {
    const int c = t * 2, g = c >> 5;       // channels 2t, 2t+1 belong to group 2t / 32
    const float inv = 1.f / (stat_s[16 + g] + stat_s[24 + g]);
    const float2 p0 = *reinterpret_cast<const float2*>(wt_all + c), p1 = *reinterpret_cast<const float2*>(wt_all + CAPW * 8 + c);
    const float r0 = (p0.x + p1.x) * inv, r1 = (p0.y + p1.y) * inv;
    AGG_STORE_ROW2(out, prm.out_dt, a, c, r0, r1);
  }
}

// ------------------------------------------------------------------------------------------
// v8 (default since round 4): the tap-merging algorithm of v7 with a FACTORED softmax and SPECIALISED front ends.
//
// What the round-3 stamps said about v7 (profiles/r3/agg_phase_times.txt, profiles/r4): 40 % of a wave's life is its front end
// (2 x 6 float4 logit loads, 24 exp, two block barriers for the softmax statistics), the launch lasts as long as its slowest wave,
// and with the benchmark's metre-scale key-point offsets 65 % of the level-0 (camera, level) items spread over more than 64
// tokens.  v8 therefore
//  * factors the 364-way softmax.  logit[n][j][g] = U[a][j][g] + V[n][j][g] (j = level * P + point), so
//      exp(logit - m) = exp(U + mV - m') * exp(V[n] - mV),   mV[j][g] = max_n V[n][j][g].
//    The camera factor eV[n] = exp(V[n] - mV) in (0, 1], its camera sum EV = sum_n eV[n] and mV depend on the layer and the frame
//    only: far3d_agg_tables computes them once per frame for all layers.  Per query that leaves 2 float4 loads of U, 8 exp per lane
//    and S[g] = sum_j eU[j][g] * EV[j][g]; the largest term is exactly 1 (same overflow / underflow behaviour as the plain
//    max-subtracted softmax).  Weights are formed only for the (camera, level) items that are visible: w = eU * eV[n].
//  * specialises the two waves' front ends: wave 0 projects the 91 (camera, point) pairs, builds the item descriptors and deals
//    the items; wave 1 computes the softmax statistics; they swap results through each other's (still unused) row-list regions
//    and meet at ONE barrier (v7: two barriers with both waves doing both halves; a fully redundant front end without any
//    barrier was built first and is 6 % slower: profiles/r4/agg_live_specialised_front_ab.jsonl);
//  * deals the visible (camera, level) items to the two waves by estimated work (greedy, by wave 0) instead
//    of by level parity, and raises the issue priority of waves that got a lot of it (the launch ends with its slowest wave);
//  * projects with one v_rcp instead of four IEEE divisions, stores PIXEL coordinates per (camera, level, point) for the build
//    loops, evaluates the tent weights with clamp modifiers, pads the row list so that the gather needs no bounds checks, and
//    addresses rows as 32-bit byte offsets from a scalar base.
// Limits: N <= 8, P <= 16, L <= 4, value maps < 4 GiB; other shapes take v7.
// ------------------------------------------------------------------------------------------
#define AGG8_CAPW 128
#define AGG8_PAD 16
#define AGG8_WSLOTS 4
#define AGG8_WCAM 104      // float4 per hinted camera row in sorted mode (L * P * 2 <= 104: P <= 13 at L = 4)
#define AGG8_LDS (8 * 4 * 16 * 8 + 64 + 2 * AGG8_WSLOTS * 32 * 16 + 256 + 2 * (AGG8_CAPW + AGG8_PAD) * 36)      // + 256: sorted mode's weight layout

template <typename TV, int NB>     // NB loads in flight per buffer, two buffers
__device__ __forceinline__ void agg8_gather(const TV* __restrict__ feat, const unsigned* off_s, const float* wt_s, int cnt, int lane,
                                            float (&acc)[8]) {
  // cnt is a multiple of 2 NB (bf16 rows: 2 per load) / NB (fp32 rows); padding entries carry weight 0 and offset 0
  if (cnt <= 0) return;
  typedef unsigned g8_u32x4 __attribute__((ext_vector_type(4)));
  const char* base = reinterpret_cast<const char*>(feat);
  if constexpr (sizeof(TV) == 2) {
    const int l31 = lane & 31, hi = lane >> 5, g = l31 >> 2;
    const unsigned lo = (unsigned)l31 * 16u;
    const unsigned* op = off_s + hi;
    const float* wp = wt_s + hi * 8 + g;
    g8_u32x4 va[NB], vb[NB];
    float wa[NB], wb[NB];
    auto issue = [&](int k0, g8_u32x4 (&v)[NB], float (&w)[NB]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        v[i] = *reinterpret_cast<const g8_u32x4*>(base + (size_t)(op[k0 + 2 * i] + lo));
        w[i] = wp[(k0 + 2 * i) * 8];
      }
    };
    auto consume = [&](const g8_u32x4 (&v)[NB], const float (&w)[NB]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const agg_f2 x = {__uint_as_float(v[i][k] << 16), __uint_as_float(v[i][k] & 0xffff0000u)};
          agg_f2 a = {acc[2 * k], acc[2 * k + 1]};
          a = x * w[i] + a;
          acc[2 * k] = a.x; acc[2 * k + 1] = a.y;
        }
      }
    };
    constexpr int E = 2 * NB;      // entries per buffer
    issue(0, va, wa);
    for (int k0 = E; ; k0 += 2 * E) {
      if (k0 < cnt) issue(k0, vb, wb);
      consume(va, wa);
      if (k0 >= cnt) break;
      if (k0 + E < cnt) issue(k0 + E, va, wa);
      consume(vb, wb);
      if (k0 + E >= cnt) break;
    }
  } else {
    const int g = lane >> 3;
    const unsigned lo = (unsigned)lane * 16u;
    const float* wp = wt_s + g;
    float4 va[NB], vb[NB];
    float wa[NB], wb[NB];
    auto issue = [&](int k0, float4 (&v)[NB], float (&w)[NB]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        v[i] = *reinterpret_cast<const float4*>(base + (size_t)(off_s[k0 + i] + lo));
        w[i] = wp[(k0 + i) * 8];
      }
    };
    auto consume = [&](const float4 (&v)[NB], const float (&w)[NB]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        acc[0] += w[i] * v[i].x; acc[1] += w[i] * v[i].y; acc[2] += w[i] * v[i].z; acc[3] += w[i] * v[i].w;
      }
    };
    issue(0, va, wa);
    for (int k0 = NB; ; k0 += 2 * NB) {
      if (k0 < cnt) issue(k0, vb, wb);
      consume(va, wa);
      if (k0 >= cnt) break;
      if (k0 + NB < cnt) issue(k0 + NB, va, wa);
      consume(vb, wb);
      if (k0 + NB >= cnt) break;
    }
  }
}

// Measured A/B of this kernel's knobs (profiles/r4/agg_live_*_ab.jsonl, live operands of a benchmark frame, bf16 rows): without the
// work-dependent s_setprio 17.9-19.2 us against 16.9-17.8; a flatter work estimate 17.5-18.8; 8 instead of 4 loads per buffer in the
// in-loop gather spills (128 VGPRs) 23-30 us; 192-entry lists (22.6 KB of LDS: 7 workgroups per CU, no longer every query resident
// with margin) 17.8-21.1 us; an "early" gather buffer (an item's first 8 rows requested before the next item is built, consumed after it:
// 128 VGPRs + 12 B of scratch) 17.9-18.2 us against 17.3-17.9 -- the build and the gather do not wait for each other.
// SPLIT (variant 9, round 5): the launch ends with its slowest wave, and the slowest waves belong to the queries two cameras see (twice
// the (camera, level) items).  far3d_agg_order marks those queries and appends one SIBLING entry per marked query to perm; the extra
// workgroups at the end of the grid take them.  Both workgroups of a marked query run the same front end and deal its items into FOUR
// shares (same greedy rule), workgroup `part` taking shares 2 part and 2 part + 1; each publishes its unnormalised 256-float sum with
// device-scope stores and draws a ticket; the one that arrives second adds the two partials in part order (part 0 + part 1 whoever
// merges: deterministic), applies 1 / S and writes the row.  An unmarked query takes the two-share path, bit-identical to variant 8.
// SORTED (round 6): U / offs hold the query of perm entry e at ROW e and qbase[e][n] = lidar2img_n [ref_m, 1] comes from
// far3d_agg_order -- every operand load is issued in the first burst, from the block index alone; perm[e] is read for the hole test
// and the output row only (before: perm[e] -> ref / offs / U rows, a dependent round trip in front of the first useful instruction,
// profiles/r5/agg_phase_times.txt).  Same fmaf chains in both forms (csrc/agg_tables.hpp): bit-identical rows.
// DEAL: how the visible (camera, level) items are dealt to the waves: 1 (round 6) = ranked by work estimate and dealt in snake order
// (deal_snake below); 0 = round 4's greedy rule in arrival order (every item to the least loaded share: a serial scalar chain of ~15
// instructions per item on the front end's critical path; kept as variant 12 for A/B).  A contiguous split of the items in lane order
// (lane-parallel, no loop at all) was built first and measured: -2 % on bf16 rows, +8 % on fp32 rows -- the balance of the two waves'
// gathers is worth more than the dealing's own latency.
// PHASE = 1 (round 6, variant 13, A/B only): the LIST-BUILD half of a two-kernel split -- everything up to the row lists, which go to a
// global workspace (per wave: AGG_GCAP entries of offset + 8 weights, count; per slot: the 8 softmax denominators) instead of being
// gathered; aggregate_gather_kernel below is the other half.  VERDICT r5 item 3 (c) asked for the split to be measured.
#define AGG_GCAP 1024
// BATCHED: far3d_aggregate_batched's instantiations, blockIdx.y = sample (AGG_SAMPLE_BASES above kernel 7); without perm, SPLIT, SORTED;
// a sample's hole of unused query rows comes from AggParamsBatched (AGG_SAMPLE_HOLE) and leaves through hole_row like a perm entry ~a.
template <typename TV, int PT, int PRIO = 1, int LOOPNB = 4, int CAP = AGG8_CAPW, bool SPLIT = false, bool SORTED = false, int DEAL_ = -1, int PHASE = 0,
          bool BATCHED = false>
__global__ __launch_bounds__(128, 4) void aggregate_v8_kernel(const TV* __restrict__ feat, const float* __restrict__ ref,
                                                           const float* __restrict__ offs, const float* __restrict__ l2i,
                                                           const float* __restrict__ U, const float* __restrict__ tab,
                                                           const int* __restrict__ perm, void* __restrict__ out, AggParamsOf<BATCHED> prm,
                                                           const float4* __restrict__ qbase) {
  // default dealing: snake on bf16 rows; greedy on fp32 rows, where the snake measured no gain (the gathers, twice the bytes, dominate)
  // and the in-tolerance engine keeps the summation order its parity evidence was taken with
  constexpr int DEAL = DEAL_ >= 0 ? DEAL_ : (sizeof(TV) == 2 ? 1 : 0);
  int a0 = (blockIdx.x & 7) * prm.q_per_xcd + (blockIdx.x >> 3);
  bool sibling = false;
  if constexpr (SPLIT) {
    const int nmain = 8 * prm.q_per_xcd;
    if ((int)blockIdx.x >= nmain) { sibling = true; a0 = prm.A + ((int)blockIdx.x - nmain); }
  }
  if (!sibling && a0 >= prm.A) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int P = PT ? PT : prm.P, L = prm.L, N = prm.N;
  const int n4 = L * P * 2;                                               // float4 per camera row of the tables (<= 128)
  [[maybe_unused]] int hole_cnt = 0;
  if constexpr (BATCHED) {
    static_assert(!SPLIT && !SORTED && PHASE == 0, "the batched launch has no sibling split, sorted mode or list-build phase");
    const long b = blockIdx.y;
    hole_cnt = AGG_SAMPLE_HOLE_COUNT(b);      // first: its pointer comes with the kernel's first argument loads, its value with the burst
    AGG_SAMPLE_BASES(b);
    tab += b * (2 + N) * (n4 * 4);
  }
  constexpr int CAPT = CAP + AGG8_PAD;
  float2* pxy_s = reinterpret_cast<float2*>(smem);                        // [8][4][16] pixel coordinates per (camera, level, point)
  float* stat_s = reinterpret_cast<float*>(pxy_s + 8 * 4 * 16);           // [8] softmax denominators (+ 8 pad)
  float4* w_all = reinterpret_cast<float4*>(stat_s + 16);                 // [2 waves][WSLOTS][16 points x 2] item weights
  // sorted mode lays the same 4352 bytes out as [2 hinted cameras][<= 104 float4: the query's weights against that camera, all levels]
  // + [2 waves][32] for an item of any other camera (AGG8_WCAM float4 per camera row: L * P * 2 <= 104)
  unsigned* off_all = reinterpret_cast<unsigned*>(w_all + 2 * AGG8_WSLOTS * 32 + 16);     // [2][CAPT] row byte offsets
  float* wt_all = reinterpret_cast<float*>(off_all + 2 * CAPT);           // [2][CAPT][8] merged weights
  float4* w_s = w_all + wv * AGG8_WSLOTS * 32;
  unsigned* off_s = off_all + wv * CAPT;
  float* wt_s = wt_all + wv * CAPT * 8;

  AGG_TS(0);
  // ---- loads that do not depend on the query: table rows (mV, EV) and the projection matrices of this lane's two cameras.  Round 6: each
  // wave loads what ITS half of the specialised front end reads -- wave 0 (projection, dealing) the matrices, the reference point and the
  // key-point offsets, wave 1 (softmax statistics) the table rows and the query's logits; before, both waves loaded everything: 26 KB
  // of vector-memory requests per workgroup, of which 13 KB were never read, in the one phase where all 3 088 waves of the launch load at
  // once.  No branch: the ADDRESSES are selected per wave (scalar selects) and the same six loads are issued by both waves -- values
  // loaded inside a branch and used behind the join are waited for (and copied) inside the branch, which serialises the round trips.
  // A slot the wave does not need reads tab[0] in every lane: one cache line.
  const float4 NEG4 = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY), Z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4* T4 = reinterpret_cast<const float4*>(tab);
  // (every load is unconditional with a clamped index and the selection happens on registers: a load under a lane condition is
  // split into dword loads behind exec-mask branches, and a load inside a branch is waited for inside it)
  const bool v0 = lane < n4, v1 = lane + 64 < n4;
  const int i0 = min(lane, n4 - 1), i1 = min(lane + 64, n4 - 1);
  const int r = lane >> 4, p = lane & 15;
  const bool w0 = wv == 0;                                    // wave-uniform
  const float4* mA = reinterpret_cast<const float4*>(l2i + min(r, N - 1) * 16);
  const float4* mB = reinterpret_cast<const float4*>(l2i + min(r + 4, N - 1) * 16);
  float4 mA0, mA1, mA2, mB0, mB1, mB2;        // wave 0: rows 0..2 of the projection matrices of cameras r and r + 4
  float4 mv0, mv1, es0, es1;                  // wave 1: table rows mV and EV
  float4 eu0, eu1;                            // wave 1: the query's logits
  float rm0, rm1, rm2;                        // wave 0: the reference point in metres
  float of0, of1, of2;
  int a;
  int cam0 = 0, cam1 = 0;                     // sorted mode: the two cameras whose weights wave 1 forms in front of the barrier
  if constexpr (SORTED) {
    a = perm[a0];                             // needed behind the front end's barrier only (hole test, output row)
    const int hint = reinterpret_cast<const int*>(qbase + a0)[3];      // qbase[e].w: camera hint of far3d_agg_order (scalar load)
    cam0 = min(hint & 0xff, N - 1); cam1 = min((hint >> 8) & 0xff, N - 1);
  } else {
    const float4 ld0 = *(w0 ? mA : T4 + i0), ld1 = *(w0 ? mA + 1 : T4 + i1), ld2 = *(w0 ? mA + 2 : T4 + n4 + i0);
    const float4 ld3 = *(w0 ? mB : T4 + n4 + i1), ld4 = *(w0 ? mB + 1 : T4), ld5 = *(w0 ? mB + 2 : T4);
    mA0 = ld0; mA1 = ld1; mA2 = ld2; mB0 = ld3; mB1 = ld4; mB2 = ld5;        // wave 0's reading of the six slots
    mv0 = ld0; mv1 = ld1;                                                    // wave 1's
    es0 = ld2; es1 = ld3;
    a = perm ? perm[a0] : a0;
    if constexpr (BATCHED) AGG_SAMPLE_HOLE(a, a0, hole_cnt);
  }
  bool split = false;
  if constexpr (SPLIT) {
    if (sibling && a == AGG_NO_SIBLING) return;      // unused sibling slot
  }
  auto hole_row = [&]() __attribute__((always_inline)) {      // ~a: row a holds no query (far3d_agg_order): zero row, no work
    a = ~a;
    const int c = t * 2;
    AGG_ZERO_ROW2(out, prm.out_dt, a, c);
  };
  // (sorted mode tests for the hole BEHIND the front end's barrier: a test here would make the whole load burst wait for perm[e] --
  // the compiler sinks the loads below the branch -- and a hole slot's operands are finite rows like any other)
  if constexpr (!SORTED) {
    if (a < 0) { hole_row(); return; }
  }
  if constexpr (SPLIT) {
    split = (a & AGG_SPLIT_FLAG) != 0;
    a &= AGG_ROW_MASK;
  }
  const int part = sibling ? 1 : 0;
  if constexpr (!SORTED) {
    const float rf0 = ref[a * 3], rf1 = ref[a * 3 + 1], rf2 = ref[a * 3 + 2];
    const float* op_ = offs + (long)a * prm.ldO + min(p, P - 1) * 3;
    of0 = op_[0]; of1 = op_[1]; of2 = op_[2];
    const float4* U4 = reinterpret_cast<const float4*>(U + (long)a * prm.ldU);
    eu0 = *(w0 ? T4 : U4 + i0); eu1 = *(w0 ? T4 : U4 + i1);
    // the reference point in metres, as far3d_agg_order computes it for the sorted mode (same fma: same bits)
    rm0 = agg_base_metre(rf0, prm.pc_span[0], prm.pc_lo[0]); rm1 = agg_base_metre(rf1, prm.pc_span[1], prm.pc_lo[1]);
    rm2 = agg_base_metre(rf2, prm.pc_span[2], prm.pc_lo[2]);
  }
  if constexpr (!SORTED) {
    if (!v0) mv0 = NEG4;         // lanes past the row: logit -inf -> weight 0 (register selects)
    if (!v1) mv1 = NEG4;
  }
  AGG_TS(8);

  // ---- projection (detr3d_transformer.py:524-525,547-552) of the P key points into cameras r and r + 4, per-camera bounding box,
  // per (camera, level) item descriptor in lane (r, level)
  // level sizes of level (lane & 15), as floats, without indexing the kernel arguments by a VGPR
  float Wf0 = prm.Wf[0], Wf1 = prm.Wf[1], Wf2 = prm.Wf[2], Wf3 = prm.Wf[3], Hf0 = prm.Hf[0], Hf1 = prm.Hf[1], Hf2 = prm.Hf[2], Hf3 = prm.Hf[3];
  asm volatile("" : "+s"(Wf0), "+s"(Wf1), "+s"(Wf2), "+s"(Wf3), "+s"(Hf0), "+s"(Hf1), "+s"(Hf2), "+s"(Hf3));   // in SGPRs here: selects, not branches around loads
  const float Wme = p == 0 ? Wf0 : p == 1 ? Wf1 : p == 2 ? Wf2 : Wf3;
  const float Hme = p == 0 ? Hf0 : p == 1 ? Hf1 : p == 2 ? Hf2 : Hf3;
  const float WfL[AGG_MAX_L] = {Wf0, Wf1, Wf2, Wf3}, HfL[AGG_MAX_L] = {Hf0, Hf1, Hf2, Hf3};
  // key point = reference point in metres + learned offset, then lidar2img: the REFERENCE's operation order (detr3d_transformer.py:
  // 524-525, 547-552).  Round 6 also built the hoisted form M [ref_m, 1] + M3 off (per-frame table of far3d_agg_order, 128 B per slot)
  // and withdrew it: its rounding is independent of the reference's, ~2e-4 px of pixel-coordinate noise that moved the streaming
  // witness's worst logit across the 1e-3 bar, it cost far3d_agg_order 8 us, and it bought no time.
  auto project = [&](const float4& m0, const float4& m1, const float4& m2, int n, int& d0, int& d1, int& est, bool& is_patch) __attribute__((always_inline)) {
    const bool act = n < N && p < P;
    const float k0 = rm0 + of0, k1 = rm1 + of1, k2 = rm2 + of2;      // (the sorted mode's operands arrive inside wave 0's arm)
    // The evaluation order of the three dot products, spelled out (contraction off): left to the compiler, the packed-math vectoriser
    // commutes the adds and the contraction then fuses a different product in x than in y -- and differently again in another
    // instantiation of this kernel (the sorted and the unsorted form would stop agreeing bit for bit).  The order below is the one the
    // kernel had when the in-tolerance engine's streaming parity evidence was taken (decoded from that build's ISA): the engine's worst
    // logit on the fourth streaming frame sits AT the 1e-3 bar, and three other orders of these nine products -- each as valid -- put it
    // at 1.01e-3, 1.03e-3 and 1.08e-3 against this one's 0.94e-3.
    float x, y, z;
    {
#pragma clang fp contract(off)
      x = __builtin_fmaf(m0.z, k2, __builtin_fmaf(m0.y, k1, m0.x * k0)) + m0.w;
      y = __builtin_fmaf(m1.z, k2, __builtin_fmaf(m1.x, k0, m1.y * k1)) + m1.w;
      const float zq = m2.z * k2;
      z = (__builtin_fmaf(m2.x, k0, m2.y * k1) + zq) + m2.w;
    }
    const float rz = __builtin_amdgcn_rcpf(fmaxf(z, 1e-5f));
    const float u = (x * rz) * prm.ipw, v = (y * rz) * prm.iph;
    float umin = act ? u : INFINITY, umax = act ? u : -INFINITY, vmin = act ? v : INFINITY, vmax = act ? v : -INFINITY;
    umin = agg8_row_min(umin); umax = agg8_row_max(umax);
    vmin = agg8_row_min(vmin); vmax = agg8_row_max(vmax);
    // item (camera n, level = lane & 15): token rectangle touched by the P bilinear footprints
    const float fx0 = fmaxf(floorf(fmaf(umin, Wme, -0.5f)), 0.f), fx1 = fminf(floorf(fmaf(umax, Wme, -0.5f)) + 1.f, Wme - 1.f);
    const float fy0 = fmaxf(floorf(fmaf(vmin, Hme, -0.5f)), 0.f), fy1 = fminf(floorf(fmaf(vmax, Hme, -0.5f)) + 1.f, Hme - 1.f);
    const bool vis = n < N && p < L && fx1 >= fx0 && fy1 >= fy0;           // false for NaN / empty
    const int x0 = vis ? (int)fx0 : 0, y0 = vis ? (int)fy0 : 0;
    const int spanx = vis ? (int)(fx1 - fx0) + 1 : 1, spany = vis ? (int)(fy1 - fy0) + 1 : 1;
    const int lw = (spanx > 1) + (spanx > 2) + (spanx > 4) + (spanx > 8) + (spanx > 16) + (spanx > 32);
    is_patch = vis && spanx <= 64 && spany <= (64 >> lw);
    d0 = x0 | (y0 << 16);
    d1 = spanx | (spany << 16);
    // work estimate in list entries: rows to gather + the build's own cost (a patch build is ~25 rows' worth, the per-corner one ~10)
    // (a flatter formula -- items cost about the same, profiles/r4 -- was measured and is not faster: agg_live_est_formula_ab.jsonl;
    // round 6: rows weighted 2x for fp32 value rows, priority thresholds scaled: 18.25 against 18.37 us, inside the noise, not kept)
    est = is_patch ? min(spanx * spany, 4 * P) + 25 : 4 * P + 10;
    // pixel coordinates of this lane's point on every level of camera n (read back by the build loops)
    if (act) {
#pragma unroll
      for (int l = 0; l < AGG_MAX_L; ++l)
        if (l < L) pxy_s[(n * 4 + l) * 16 + p] = make_float2(fmaf(u, WfL[l], -0.5f), fmaf(v, HfL[l], -0.5f));
    }
    return vis;
  };
  int dA0 = 0, dA1 = 0, estA = 0, dB0 = 0, dB1 = 0, estB = 0;
  unsigned long long visA, visB, patchA, patchB, mineA = 0ull, mineB = 0ull;
  int myload = 0;
  float4 S4 = make_float4(0.f, 0.f, 0.f, 0.f);
  auto softmax_stats = [&]() __attribute__((always_inline)) {
    // eU = exp(U + mV - max), S[g] = sum_j eU[j][g] EV[j][g]  (detr3d_transformer.py:539-540, factored)
    constexpr float LOG2E = 1.4426950408889634f;
    eu0 = make_float4(eu0.x + mv0.x, eu0.y + mv0.y, eu0.z + mv0.z, eu0.w + mv0.w);
    eu1 = make_float4(eu1.x + mv1.x, eu1.y + mv1.y, eu1.z + mv1.z, eu1.w + mv1.w);
    float4 mx = make_float4(fmaxf(eu0.x, eu1.x), fmaxf(eu0.y, eu1.y), fmaxf(eu0.z, eu1.z), fmaxf(eu0.w, eu1.w));
    mx.x = agg8_wave_max_parity(mx.x); mx.y = agg8_wave_max_parity(mx.y);
    mx.z = agg8_wave_max_parity(mx.z); mx.w = agg8_wave_max_parity(mx.w);
    eu0 = make_float4(__builtin_amdgcn_exp2f((eu0.x - mx.x) * LOG2E), __builtin_amdgcn_exp2f((eu0.y - mx.y) * LOG2E),
                      __builtin_amdgcn_exp2f((eu0.z - mx.z) * LOG2E), __builtin_amdgcn_exp2f((eu0.w - mx.w) * LOG2E));
    eu1 = make_float4(__builtin_amdgcn_exp2f((eu1.x - mx.x) * LOG2E), __builtin_amdgcn_exp2f((eu1.y - mx.y) * LOG2E),
                      __builtin_amdgcn_exp2f((eu1.z - mx.z) * LOG2E), __builtin_amdgcn_exp2f((eu1.w - mx.w) * LOG2E));
    S4 = make_float4(eu0.x * es0.x + eu1.x * es1.x, eu0.y * es0.y + eu1.y * es1.y, eu0.z * es0.z + eu1.z * es1.z, eu0.w * es0.w + eu1.w * es1.w);
    S4.x = agg8_wave_sum_parity(S4.x); S4.y = agg8_wave_sum_parity(S4.y);
    S4.z = agg8_wave_sum_parity(S4.z); S4.w = agg8_wave_sum_parity(S4.w);
  };
  // greedy on the running work estimates into nsh shares (2, or 4 for a split query): an item goes to the least loaded share, ties to
  // the lower one; returned are the items and loads of shares s0 and s1 (the two waves of this workgroup).  nsh = 2, (s0, s1) = (0, 1)
  // is variant 8's dealing, decision for decision.
  auto deal2 = [&](int nsh, int s0, int s1, unsigned long long& a0m, unsigned long long& b0m, int& l0, unsigned long long& a1m,
                   unsigned long long& b1m, int& l1) __attribute__((always_inline)) {
    int ld0 = 0, ld1 = 0, ld2 = 0, ld3 = 0;
    a0m = 0ull; b0m = 0ull; a1m = 0ull; b1m = 0ull;
    const int big = nsh > 2 ? 0 : 0x3fffffff;        // shares 2 and 3 never win a two-share deal
    // every update is a select on scalars (an `if (best == k) ld_k += e` chain is turned into a scratch array indexed by `best`)
    auto place = [&](int e) __attribute__((always_inline)) -> int {
      const int c2 = ld2 + big, c3 = ld3 + big;
      int best = 0, lb = ld0;
      best = ld1 < lb ? 1 : best; lb = min(lb, ld1);
      best = c2 < lb ? 2 : best; lb = min(lb, c2);
      best = c3 < lb ? 3 : best;
      ld0 += best == 0 ? e : 0; ld1 += best == 1 ? e : 0; ld2 += best == 2 ? e : 0; ld3 += best == 3 ? e : 0;
      return best;
    };
    for (unsigned long long m = visA; m; m &= m - 1ull) {
      const int b = __builtin_ctzll(m);
      const int sh = place(__builtin_amdgcn_readlane(estA, b));
      a0m |= sh == s0 ? 1ull << b : 0ull;
      a1m |= sh == s1 ? 1ull << b : 0ull;
    }
    for (unsigned long long m = visB; m; m &= m - 1ull) {
      const int b = __builtin_ctzll(m);
      const int sh = place(__builtin_amdgcn_readlane(estB, b));
      b0m |= sh == s0 ? 1ull << b : 0ull;
      b1m |= sh == s1 ? 1ull << b : 0ull;
    }
    l0 = s0 == 0 ? ld0 : s0 == 1 ? ld1 : s0 == 2 ? ld2 : ld3;
    l1 = s1 == 0 ? ld0 : s1 == 1 ? ld1 : s1 == 2 ? ld2 : ld3;
  };
  // snake deal (DEAL = 1): rank the items by work estimate (descending; ties: cameras 0-3 first, then the lower lane) and deal the
  // ranks 0 1 1 0 0 1 1 0 ... (four shares: 0 1 2 3 3 2 1 0 ...): the sorted order balances better than arrival order, and the loop
  // carries no scalar dependency chain -- one v_readlane and two compare-and-count pairs per item.
  auto deal_snake = [&](bool vA, bool vB, int nsh, int s0, int s1, unsigned long long& a0m, unsigned long long& b0m, int& l0,
                        unsigned long long& a1m, unsigned long long& b1m, int& l1) __attribute__((always_inline)) {
    const int eA = vA ? estA : -1, eB = vB ? estB : -1;
    int rkA = 0, rkB = 0;
    for (unsigned long long m = visA; m; m &= m - 1ull) {
      const int b = __builtin_ctzll(m), e = __builtin_amdgcn_readlane(estA, b);
      rkA += (e > eA || (e == eA && b < lane)) ? 1 : 0;
      rkB += e >= eB ? 1 : 0;
    }
    for (unsigned long long m = visB; m; m &= m - 1ull) {
      const int b = __builtin_ctzll(m), e = __builtin_amdgcn_readlane(estB, b);
      rkA += e > eA ? 1 : 0;
      rkB += (e > eB || (e == eB && b < lane)) ? 1 : 0;
    }
    int shA, shB;
    if (nsh == 2) { shA = ((rkA + 1) >> 1) & 1; shB = ((rkB + 1) >> 1) & 1; }
    else { const int tA = rkA & 7, tB = rkB & 7; shA = tA < 4 ? tA : 7 - tA; shB = tB < 4 ? tB : 7 - tB; }
    a0m = __ballot(vA && shA == s0); a1m = __ballot(vA && shA == s1);
    b0m = __ballot(vB && shB == s0); b1m = __ballot(vB && shB == s1);
    l0 = __builtin_amdgcn_readfirstlane(agg8_wave_sum_i32((vA && shA == s0 ? estA : 0) + (vB && shB == s0 ? estB : 0)));
    l1 = __builtin_amdgcn_readfirstlane(agg8_wave_sum_i32((vA && shA == s1 ? estA : 0) + (vB && shB == s1 ? estB : 0)));
  };
  {
    // SPECIALISED front end: wave 0 projects and deals, wave 1 computes the softmax statistics; they swap results through the
    // (still unused) row-list regions of each other and meet at one barrier
    int4* xd = reinterpret_cast<int4*>(wt_all + CAPT * 8);       // wave 1's list region <- wave 0: descriptors, dealing
    float4* xe = reinterpret_cast<float4*>(wt_all);              // wave 0's list region <- wave 1: eU
    if (wv == 0) {
      if constexpr (SORTED) {
        // SORTED front end, wave 0: ONE 16-byte load per lane fetches everything the projection needs that is uniform over a 16-lane
        // row -- lane (r, k) reads row k of camera r's matrix (k < 3), row k - 3 of camera r + 4's (k < 6), the slot's reference point
        // in metres qbase[e] (k = 6) -- and 27 row broadcasts (v_mov_dpp row_newbcast) hand every lane of the row its copies; plus the
        // lane's key-point offset.  2 vector-memory instructions instead of 9: with 12 waves of a CU starting at once, the texture
        // addresser's 16 cycles per 64 x 16-byte request were what the slowest wave waited for (round 6, s2/phase_8s.txt).
        const int k = min(p, 6);
        const float4* src = k < 3 ? mA + k : k < 6 ? mB + (k - 3) : qbase + a0;
        const float4 pk = *src;
        const float* op_ = offs + (long)a0 * prm.ldO + min(p, P - 1) * 3;
        of0 = op_[0]; of1 = op_[1]; of2 = op_[2];
        mA0 = agg8_row_bcast4<0>(pk); mA1 = agg8_row_bcast4<1>(pk); mA2 = agg8_row_bcast4<2>(pk);
        mB0 = agg8_row_bcast4<3>(pk); mB1 = agg8_row_bcast4<4>(pk); mB2 = agg8_row_bcast4<5>(pk);
        rm0 = agg8_row_bcast<6>(pk.x); rm1 = agg8_row_bcast<6>(pk.y); rm2 = agg8_row_bcast<6>(pk.z);
      }
      bool patA, patB;
      const bool visA_ = project(mA0, mA1, mA2, r, dA0, dA1, estA, patA);
      const bool visB_ = project(mB0, mB1, mB2, r + 4, dB0, dB1, estB, patB);
      visA = __ballot(visA_); visB = __ballot(visB_); patchA = __ballot(patA); patchB = __ballot(patB);
      AGG_TS(1);
      unsigned long long oA, oB;
      int oload;
      if constexpr (DEAL == 1) deal_snake(visA_, visB_, split ? 4 : 2, 2 * part, 2 * part + 1, mineA, mineB, myload, oA, oB, oload);
      else deal2(split ? 4 : 2, 2 * part, 2 * part + 1, mineA, mineB, myload, oA, oB, oload);
      xd[lane] = make_int4(dA0, dA1, dB0, dB1);
      if (lane == 0) {
        unsigned long long* q = reinterpret_cast<unsigned long long*>(xd + 64);
        q[0] = oA; q[1] = oB; q[2] = patchA; q[3] = patchB; q[4] = (unsigned long long)oload;
      }
      AGG_TS(2);
    } else {
      if constexpr (SORTED) {
        // wave 1: the table rows and the query's logits, nothing else (6 requests; before, 3 more that only wave 0 read)
        const float4* U4 = reinterpret_cast<const float4*>(U + (long)a0 * prm.ldU);
        mv0 = T4[i0]; mv1 = T4[i1]; es0 = T4[n4 + i0]; es1 = T4[n4 + i1];
        eu0 = U4[i0]; eu1 = U4[i1];
        if (!v0) mv0 = NEG4;
        if (!v1) mv1 = NEG4;
      }
      float4 c0a, c0b, c1a, c1b;
      if constexpr (SORTED) {
        // the camera factors of the two hinted cameras, for this lane's two pieces of the row: requested behind the hint's scalar load,
        // in flight under the softmax statistics
        c0a = T4[(2 + cam0) * n4 + i0]; c0b = T4[(2 + cam0) * n4 + i1];
        c1a = T4[(2 + cam1) * n4 + i0]; c1b = T4[(2 + cam1) * n4 + i1];
      }
      softmax_stats();
      AGG_TS(1);
      xe[lane] = eu0; xe[64 + lane] = eu1;
      if (lane < 2) *reinterpret_cast<float4*>(stat_s + (lane & 1) * 4) = S4;
      if constexpr (SORTED) {
        // w = e^U * eV[camera] for the whole row of both hinted cameras: the items behind the barrier read their level's slice
        if (v0) {
          w_all[lane] = make_float4(eu0.x * c0a.x, eu0.y * c0a.y, eu0.z * c0a.z, eu0.w * c0a.w);
          w_all[AGG8_WCAM + lane] = make_float4(eu0.x * c1a.x, eu0.y * c1a.y, eu0.z * c1a.z, eu0.w * c1a.w);
        }
        if (v1) {
          w_all[64 + lane] = make_float4(eu1.x * c0b.x, eu1.y * c0b.y, eu1.z * c0b.z, eu1.w * c0b.w);
          w_all[AGG8_WCAM + 64 + lane] = make_float4(eu1.x * c1b.x, eu1.y * c1b.y, eu1.z * c1b.z, eu1.w * c1b.w);
        }
      }
      AGG_TS(2);
    }
    __syncthreads();
    if constexpr (SORTED) {
      if (a < 0) {      // block-uniform
        if constexpr (PHASE == 1) { if (lane == 0) prm.split_tick[(long)a0 * 2 + wv] = 0; }      // (the gather half writes the zero row)
        else hole_row();
        return;
      }
    }
    if (wv == 0) {
      eu0 = xe[lane]; eu1 = xe[64 + lane];
    } else {
      const int4 d = xd[lane];
      dA0 = d.x; dA1 = d.y; dB0 = d.z; dB1 = d.w;
      const unsigned long long* q = reinterpret_cast<const unsigned long long*>(xd + 64);
      mineA = q[0]; mineB = q[1]; patchA = q[2]; patchB = q[3]; myload = (int)q[4];
      visA = mineA; visB = mineB;
    }
  }
  // the launch ends with its slowest wave: waves that drew a lot of work get the issue slots first
  if constexpr (PRIO) {
    if (myload > 200) __builtin_amdgcn_s_setprio(3);
    else if (myload > 120) __builtin_amdgcn_s_setprio(2);
    else if (myload > 70) __builtin_amdgcn_s_setprio(1);
  }
  AGG_TS(9);

  // ---- items are processed in batches of AGG8_WSLOTS: camera factors eV[n] of the batch (global, L2-resident) -> w = eU * eV -> LDS
  unsigned long long qa = mineA, qb = mineB;
  int items[AGG8_WSLOTS], ni = 0;
  auto take_batch = [&]() __attribute__((always_inline)) {
    ni = 0;
#pragma unroll
    for (int k = 0; k < AGG8_WSLOTS; ++k) {
      items[k] = 0;
      if (qa) { items[k] = __builtin_ctzll(qa); qa &= qa - 1ull; ni = k + 1; }
      else if (qb) { items[k] = 64 + __builtin_ctzll(qb); qb &= qb - 1ull; ni = k + 1; }
    }
  };
  float4 ev[AGG8_WSLOTS];
  auto issue_ev = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < AGG8_WSLOTS; ++k) {
      ev[k] = Z4;
      if (k < ni) {
        const int n = ((items[k] >> 4) & 3) + ((items[k] >> 6) << 2), l = items[k] & 15, base = l * 2 * P;
        const bool in0 = (unsigned)(lane - base) < (unsigned)(2 * P);
        ev[k] = T4[(2 + n) * n4 + (in0 ? lane : min(lane + 64, n4 - 1))];      // unconditional; lanes outside the slice are not used
      }
    }
  };
  if constexpr (!SORTED) {
    take_batch();
    issue_ev();
  }

  AGG_TS(3);

  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  int cnt = 0;
  // gather the listed rows: NB loads per buffer in flight (4 inside the item loop, 8 -- all of a typical list at once -- for the last one)
  int gpos = 0;                                  // PHASE 1: entries this wave has written to its global list
  auto flush_nb = [&](auto nbtag) __attribute__((always_inline)) {
    constexpr int NB = decltype(nbtag)::value;
    constexpr int GRAN = PHASE == 1 ? 16 : (sizeof(TV) == 2 ? 2 * NB : NB);
    const int padn = (-cnt) & (GRAN - 1);
    if (lane < padn) {
      off_s[cnt + lane] = 0u;
      *reinterpret_cast<float4*>(wt_s + (cnt + lane) * 8) = Z4;
      *reinterpret_cast<float4*>(wt_s + (cnt + lane) * 8 + 4) = Z4;
    }
    if constexpr (PHASE == 1) {
      // append the (padded) list to the wave's global list; entries past the capacity are dropped and the count says so (negative)
      const int n = cnt + padn;
      const long wslot = (long)a0 * 2 + wv;
      unsigned* goff = reinterpret_cast<unsigned*>(prm.split_part) + wslot * AGG_GCAP;
      float4* gwt = reinterpret_cast<float4*>(prm.split_part + (long)gridDim.x * 2 * AGG_GCAP) + wslot * AGG_GCAP * 2;
      if (gpos >= 0 && gpos + n <= AGG_GCAP) {
        for (int i = lane; i < n; i += 64) {
          goff[gpos + i] = off_s[i];
          gwt[(gpos + i) * 2] = *reinterpret_cast<const float4*>(wt_s + i * 8);
          gwt[(gpos + i) * 2 + 1] = *reinterpret_cast<const float4*>(wt_s + i * 8 + 4);
        }
        gpos += n;
      } else {
        gpos = -1;
      }
    } else {
      agg8_gather<TV, NB>(feat, off_s, wt_s, cnt + padn, lane, acc);
    }
    cnt = 0;
  };
  auto flush = [&]() __attribute__((always_inline)) { flush_nb(std::integral_constant<int, LOOPNB>{}); };
  auto append = [&](bool hit, unsigned off, const float (&wa)[8]) __attribute__((always_inline)) {
    const unsigned long long m = __ballot(hit);
    const int c = __popcll(m);
    if (hit) {
      const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
      off_s[pos] = off;
      *reinterpret_cast<float4*>(wt_s + pos * 8) = make_float4(wa[0], wa[1], wa[2], wa[3]);
      *reinterpret_cast<float4*>(wt_s + pos * 8 + 4) = make_float4(wa[4], wa[5], wa[6], wa[7]);
    }
    cnt += c;
  };
  constexpr unsigned ROWB = 256u * (unsigned)sizeof(TV);      // bytes per token row

  // one (camera, level) item: its merged row list appended to the wave's list (gathering first what is listed when the list might overflow)
  auto build_item = [&](int it, const float4* wrow) __attribute__((always_inline)) {
#ifdef FAR3D_PROFILING
    const long long ts_item = (long long)__builtin_amdgcn_s_memtime();
#endif
    // one item adds at most 64 rows (a patch's tokens; 4 P <= 64 corners): gather what is listed once fewer might fit.  The only
    // flush site inside the loops (the list is private to the wave: LDS is in order per wave, the test is wave-uniform)
    if (cnt > CAP - 64) flush();
    const int b = it & 63, second = it >> 6;
    const int n = (b >> 4) + (second << 2), l = b & 15;
    const int Wl = prm.W[l], Hl = prm.H[l];
    const unsigned rowbase = (unsigned)(n * prm.S + prm.start[l]);
    const float2* pq = pxy_s + (n * 4 + l) * 16;
    const bool is_patch = (((second ? patchB : patchA) >> b) & 1ull) != 0ull;
    if (is_patch) {
      // merged weights of the patch's tokens as a small matrix product on the (otherwise idle) matrix pipe:
      //   Wt[g][T] = sum_p w[p][g] * tent(T, p),   tent(T, p) = max(0, 1 - |px_p - tx_T|) * max(0, 1 - |py_p - ty_T|)
      // (the tent form of the four mmcv corner weights).  v_mfma_f32_16x16x4_f32 is an exact fp32 fmaf chain: rows = groups (8 of
      // 16 used), columns = 16 tokens, K = 4 points per step, 4 steps.  Lane (kk = lane >> 4, j = lane & 15) supplies
      // A = w[4 s + kk][j] and B = tent(token j of the block, point 4 s + kk): ONE tent per lane and step instead of one per
      // (lane, point), 8 LDS reads per item instead of 39, and a patch of <= 16 tokens costs a quarter of a 64-token one.
      const int d0 = __builtin_amdgcn_readlane(second ? dB0 : dA0, b), d1 = __builtin_amdgcn_readlane(second ? dB1 : dA1, b);
      const int x0 = d0 & 0xffff, y0 = d0 >> 16, spanx = d1 & 0xffff, spany = d1 >> 16;
      const int lw = (spanx > 1) + (spanx > 2) + (spanx > 4) + (spanx > 8) + (spanx > 16) + (spanx > 32);
      const int nblk = ((spany << lw) + 15) >> 4;                       // 16-token blocks of the pw x spany token grid (<= 4)
      const int kk = lane >> 4, jt = lane & 15;
      const float* wf = reinterpret_cast<const float*>(wrow);
      float aw[4];
      float2 pp[4];
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const int pt = 4 * st + kk, ptc = min(pt, P - 1);
        pp[st] = pq[ptc];                                               // a valid point for lanes past P (their A is 0; B must stay finite)
        const float wv_ = wf[ptc * 8 + (jt & 7)];
        aw[st] = (pt < P && jt < 8) ? wv_ : 0.f;
      }
      for (int blk = 0; blk < nblk; ++blk) {
        const int T = blk * 16 + jt;
        const int tx = x0 + (T & ((1 << lw) - 1)), ty = y0 + (T >> lw);
        const float ftx = (float)tx, fty = (float)ty;
        agg8_f4 acc4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < 4; ++st) {
          if (4 * st < P) {
            const float tent = __builtin_amdgcn_fmed3f(1.f - fabsf(pp[st].x - ftx), 0.f, 1.f) *
                               __builtin_amdgcn_fmed3f(1.f - fabsf(pp[st].y - fty), 0.f, 1.f);
            acc4 = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[st], tent, acc4, 0, 0, 0);
          }
        }
        // lane (kk, jt) now holds groups 4 kk .. 4 kk + 3 of token jt (kk < 2); a token is listed when any of its 8 weights is > 0
        float hv = fmaxf(fmaxf(acc4[0], acc4[1]), fmaxf(acc4[2], acc4[3])), ha, hb;
        agg_swap16(hv, ha, hb);
        hv = fmaxf(ha, hb);
        const bool hit = lane < 32 && tx < x0 + spanx && ty < y0 + spany && hv > 0.f;
        const unsigned m16 = (unsigned)__ballot(hit) & 0xffffu;         // rows kk = 0 and kk = 1 carry the same 16-bit pattern
        const int c = __popc(m16);
        if (hit) {
          const int pos = cnt + __popc(m16 & ((1u << jt) - 1u));
          *reinterpret_cast<float4*>(wt_s + pos * 8 + kk * 4) = make_float4(acc4[0], acc4[1], acc4[2], acc4[3]);
          if (kk == 0) off_s[pos] = (rowbase + (unsigned)(ty * Wl + tx)) * ROWB;
        }
        cnt += c;
      }
    } else {
      // spread wider than 64 tokens: one entry per (point, corner), mmcv's bilinear arithmetic as is (4 P <= 64 lanes)
      bool hit = false;
      unsigned off = 0u;
      float wa[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) wa[q] = 0.f;
      {
        const int pt = min(lane >> 2, P - 1), tap = lane & 3;
        const float2 pp = pq[pt];
        const float4 a0 = wrow[pt * 2], a1 = wrow[pt * 2 + 1];
        const float h_im = pp.y, w_im = pp.x;
        const bool inside = lane < P * 4 && h_im > -1.f && w_im > -1.f && h_im < (float)Hl && w_im < (float)Wl;
        const float fh = floorf(h_im), fw = floorf(w_im);
        const float lh = h_im - fh, lw_ = w_im - fw;
        const int ty = (int)fh + (tap >> 1), tx = (int)fw + (tap & 1);
        const float bw = ((tap >> 1) ? lh : 1.f - lh) * ((tap & 1) ? lw_ : 1.f - lw_);
        hit = inside && ty >= 0 && ty <= Hl - 1 && tx >= 0 && tx <= Wl - 1 && bw != 0.f;
        off = hit ? (rowbase + (unsigned)(ty * Wl + tx)) * ROWB : 0u;
        wa[0] = bw * a0.x; wa[1] = bw * a0.y; wa[2] = bw * a0.z; wa[3] = bw * a0.w;
        wa[4] = bw * a1.x; wa[5] = bw * a1.y; wa[6] = bw * a1.z; wa[7] = bw * a1.w;
      }
      append(hit, off, wa);
    }
#ifdef FAR3D_PROFILING
    if (g_agg_ts && lane == 0) {
      long long* q = g_agg_ts + ((long)blockIdx.x * 4 + wv) * 16 + (is_patch ? 12 : 14);
      q[0] += (long long)__builtin_amdgcn_s_memtime() - ts_item; q[1] += 1;
    }
#endif
  };
  if constexpr (SORTED) {
    // sorted mode: the weights of the two hinted cameras were formed by wave 1 in front of the barrier (all levels); an item of another
    // camera (the hint is the two cameras the reference point projects closest to: far3d_agg_order) forms its own here
    float4* w_fb = w_all + 2 * AGG8_WCAM + wv * 32;
    unsigned long long qa = mineA, qb = mineB;
    while (qa | qb) {
      int it;
      if (qa) { it = __builtin_ctzll(qa); qa &= qa - 1ull; }
      else { it = 64 + __builtin_ctzll(qb); qb &= qb - 1ull; }
      const int n = ((it >> 4) & 3) + ((it >> 6) << 2), l = it & 15, base = l * 2 * P;
      const float4* wrow;
      if (n == cam0) wrow = w_all + base;
      else if (n == cam1) wrow = w_all + AGG8_WCAM + base;
      else {
        const bool in0 = (unsigned)(lane - base) < (unsigned)(2 * P), in1 = (unsigned)(lane + 64 - base) < (unsigned)(2 * P);
        const float4 evv = T4[(2 + n) * n4 + (in0 ? lane : min(lane + 64, n4 - 1))];
        // (per component: a select of whole vectors goes through scratch)
        const float ex = in0 ? eu0.x : eu1.x, ey = in0 ? eu0.y : eu1.y, ez = in0 ? eu0.z : eu1.z, ew = in0 ? eu0.w : eu1.w;
        if (in0 || in1) w_fb[(in0 ? lane : lane + 64) - base] = make_float4(ex * evv.x, ey * evv.y, ez * evv.z, ew * evv.w);
        wrow = w_fb;
      }
      build_item(it, wrow);
    }
  } else {
  while (ni > 0) {
    // -- weights of the batch's items: lanes that hold the item's slice of eU multiply it with the camera factor
#pragma unroll
    for (int k = 0; k < AGG8_WSLOTS; ++k) {
      if (k < ni) {
        const int l = items[k] & 15, base = l * 2 * P;
        const bool in0 = (unsigned)(lane - base) < (unsigned)(2 * P), in1 = (unsigned)(lane + 64 - base) < (unsigned)(2 * P);
        const float4 e = in0 ? eu0 : eu1;
        if (in0 || in1)
          w_s[k * 32 + (in0 ? lane : lane + 64) - base] = make_float4(e.x * ev[k].x, e.y * ev[k].y, e.z * ev[k].z, e.w * ev[k].w);
      }
    }
    AGG_TS(11);
    // -- build: merged row list of each item
    for (int k = 0; k < ni; ++k) build_item(items[k], w_s + k * 32);
    take_batch();
    if (ni > 0) issue_ev();
  }
  }
  AGG_TS(4);
#ifdef FAR3D_PROFILING
  const int cnt_last = cnt;
#endif
  flush_nb(std::integral_constant<int, 8>{});
  AGG_TS(5);
#ifdef FAR3D_PROFILING
  if (g_agg_ts && lane == 0) { g_agg_ts[((long)blockIdx.x * 4 + wv) * 16 + 7] = cnt_last; g_agg_ts[((long)blockIdx.x * 4 + wv) * 16 + 10] = myload; }
#endif
  if constexpr (PHASE == 1) {
    static_assert(SORTED && !SPLIT, "the list-build half exists for the sorted mode only");
    if (lane == 0) prm.split_tick[(long)a0 * 2 + wv] = gpos;
    if (wv == 0 && lane < 8) (prm.split_part + (long)gridDim.x * 2 * AGG_GCAP * 9)[(long)a0 * 8 + lane] = stat_s[lane];
    return;
  }

  // ---- cross-wave sum: partial sums go into the wave's own (now dead) list region; 1/S[g] applied once here
  float* red = wt_s;                       // 256 floats: CAPT * 8 >= 256
  AGG_WAVE_PARTIALS(TV, red, acc, lane, AGG_HALVES_SWAP);
  __builtin_amdgcn_s_setprio(0);
  __syncthreads();                                                                        // the second and last barrier
  AGG_TS(6);
  {
    const int c = t * 2, g = c >> 5;       // channels 2t, 2t+1 belong to group 2t / 32
    const float inv = 1.f / stat_s[g];
    const float2 p0 = *reinterpret_cast<const float2*>(wt_all + c), p1 = *reinterpret_cast<const float2*>(wt_all + CAPT * 8 + c);
    float s0 = p0.x + p1.x, s1 = p0.y + p1.y;
    if constexpr (SPLIT) {
      if (split) {
        // publish this workgroup's unnormalised sums (device-scope 8-byte stores: through to where the sibling, on any XCD, reads them),
        // make sure they have landed, draw a ticket; the second arrival merges in part order
        unsigned long long* mine = reinterpret_cast<unsigned long long*>(prm.split_part + ((long)a * 2 + part) * 256 + c);
        const unsigned long long* other = reinterpret_cast<const unsigned long long*>(prm.split_part + ((long)a * 2 + (1 - part)) * 256 + c);
        __hip_atomic_store(mine, (unsigned long long)__float_as_uint(s0) | ((unsigned long long)__float_as_uint(s1) << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        // Publish order (MI355X guide, inter-workgroup visibility): the partials above are `sc1` write-through stores
        // (relaxed agent-scope atomic stores of 8 bytes), so no L2 write-back is needed -- but the ticket must not become visible
        // before EVERY wave's stores have left the CU: each wave drains its own vmcnt (inline asm: the compiler cannot drop it),
        // then the barrier, then thread 0 draws the ticket.  A workgroup-scope fence orders nothing another CU can observe.  The
        // merger reads the sibling's partials with `sc1` loads (they bypass its L1), valid because the producer stored `sc1`.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int* tk = reinterpret_cast<int*>(stat_s + 12);
        if (t == 0) *tk = __hip_atomic_fetch_add(prm.split_tick + a, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (*tk == 0) return;                        // first to arrive: the sibling finishes the row
        const unsigned long long o = __hip_atomic_load(other, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float o0 = __uint_as_float((unsigned)(o & 0xffffffffull)), o1 = __uint_as_float((unsigned)(o >> 32));
        s0 = part == 0 ? s0 + o0 : o0 + s0;          // part 0 + part 1, whoever merges
        s1 = part == 0 ? s1 + o1 : o1 + s1;
        if (t == 0) atomicExch(prm.split_tick + a, 0);      // zero at rest for the next launch
      }
    }
    const float r0 = s0 * inv, r1 = s1 * inv;
    AGG_STORE_ROW2(out, prm.out_dt, a, c, r0, r1);
  }
}

// The GATHER half of the two-kernel split (variant 13, A/B only): one workgroup per slot, each wave gathers the list its counterpart of
// the list-build launch wrote (staged through LDS a chunk at a time, as the fused kernel holds it), then the same cross-wave sum,
// normalisation and store as the fused kernel -- same entries in the same order (bit-identical on bf16 rows; on fp32 rows the compiler
// contracts this kernel's accumulate differently: 1 ulp).  Measured: +55 % (bf16 rows) / +115 % (fp32 rows, this kernel spills 21 dwords)
// against the fused launch (profiles/r6/agg_sorted_ab.txt).
template <typename TV>
__global__ __launch_bounds__(128, 4) void aggregate_gather_kernel(const TV* __restrict__ feat, const int* __restrict__ perm, void* __restrict__ out,
                                                               AggParams prm) {
  const int a0 = (blockIdx.x & 7) * prm.q_per_xcd + (blockIdx.x >> 3);
  if (a0 >= prm.A) return;
  __shared__ __attribute__((aligned(16))) float red_s[2 * 256];
  __shared__ __attribute__((aligned(16))) unsigned loff_s[2][AGG8_CAPW];      // the wave's list, a chunk at a time (as the fused kernel holds it)
  __shared__ __attribute__((aligned(16))) float lwt_s[2][AGG8_CAPW * 8];
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const long wslot = (long)a0 * 2 + wv;
  const int n = prm.split_tick[wslot];
  const unsigned* goff = reinterpret_cast<const unsigned*>(prm.split_part) + wslot * AGG_GCAP;
  const float* gwt = prm.split_part + (long)gridDim.x * 2 * AGG_GCAP + wslot * AGG_GCAP * 8;
  const float* gstat = prm.split_part + (long)gridDim.x * 2 * AGG_GCAP * 9 + (long)a0 * 8;
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  // (a hole slot's count is 0; the count is a multiple of 16, a chunk holds up to 128 entries)
  for (int base = 0; base < n; base += AGG8_CAPW) {
    const int m = min(AGG8_CAPW, n - base);
    for (int i = lane; i < m; i += 64) loff_s[wv][i] = goff[base + i];
    for (int i = lane; i < m * 2; i += 64)
      reinterpret_cast<float4*>(lwt_s[wv])[i] = reinterpret_cast<const float4*>(gwt)[(long)base * 2 + i];
    agg8_gather<TV, 8>(feat, loff_s[wv], lwt_s[wv], m, lane, acc);      // (LDS is in order per wave: no barrier between the copy and the reads)
  }
  int a = perm[a0];
  const int c = t * 2, g = c >> 5;
  if (a < 0) {
    a = ~a;
    AGG_ZERO_ROW2(out, prm.out_dt, a, c);
    return;
  }
  const float sden = gstat[g];
  float* red = red_s + wv * 256;
  AGG_WAVE_PARTIALS(TV, red, acc, lane, AGG_HALVES_SWAP);
  __syncthreads();
  const float inv = 1.f / sden;
  const float2 p0 = *reinterpret_cast<const float2*>(red_s + c), p1 = *reinterpret_cast<const float2*>(red_s + 256 + c);
  const float r0 = (p0.x + p1.x) * inv, r1 = (p0.y + p1.y) * inv;
  AGG_STORE_ROW2(out, prm.out_dt, a, c, r0, r1);
}

// far3d_agg_tables: the softmax factors of csrc/agg_tables.hpp for `layers` decoder layers, block = layer.
__global__ __launch_bounds__(256) void agg_tables_kernel(const float* __restrict__ Vc, float* __restrict__ tab, int N, int J) {
  agg_tables_body(Vc + (long)blockIdx.x * N * J, tab + (long)blockIdx.x * (2 + N) * J, N, J, threadIdx.x, blockDim.x);
}

extern "C" int far3d_agg_tables(const float* Vc, float* tables, int layers, int N, int J, void* stream) {
  FAR3D_CHECK_ARG(Vc && tables && layers > 0 && N > 0 && J > 0 && J % 4 == 0, "far3d_agg_tables: bad arguments (layers=%d N=%d J=%d)", layers, N, J);
  hipLaunchKernelGGL(agg_tables_kernel, dim3(layers), dim3(256), 0, (hipStream_t)stream, Vc, tables, N, J);
  FAR3D_CHECK_LAUNCH("far3d_agg_tables");
  return FAR3D_OK;
}

// ------------------------------------------------------------------------------------------
// Host side of the fused aggregation: far3d_aggregate_forward and far3d_aggregate_batched (with far3d_aggregate_batched_holes) share ONE copy of the argument checks, the
// AggParams fill, the "kernel 8 applies" rule and the dispatch over row type and point count; the dynamic-LDS sizes stand beside the
// carve-ups they mirror (agg3_lds_bytes, agg7_lds_bytes, AGG8_LDS).  The checks are several functions that take the entry's name (as in
// csrc/attn_core.hpp) because each entry runs them in an order of its own, and the order decides which message a call with two faults
// gets: forward tests the pointers first and the output dtype last; batched the sizes, then B, returns on an empty batch, then the pointers.
// ------------------------------------------------------------------------------------------
static inline int agg_check_pointers(const char* who, const void* feat, const float* ref, const float* offsets, const float* lidar2img,
                                     const float* U, const float* Vc, const float* cam_tables, const void* out, const int32_t* level_hw,
                                     const int32_t* level_start, const float* pc_range) {
  FAR3D_CHECK_ARG(feat && ref && offsets && lidar2img && U && (Vc || cam_tables) && out && level_hw && level_start && pc_range,
                  "%s: null pointer argument", who);
  return FAR3D_OK;
}
static inline int agg_check_shape(const char* who, int C, int G, int L, int N, int P, int feat_dtype) {
  FAR3D_CHECK_ARG(C == 256 && G == 8, "%s: fused kernel is built for C=256,G=8 (got C=%d G=%d)", who, C, G);
  FAR3D_CHECK_ARG(L >= 1 && L <= AGG_MAX_L, "%s: L=%d out of range [1,%d]", who, L, AGG_MAX_L);
  FAR3D_CHECK_ARG(N >= 1 && N <= AGG4_MAX_N && P >= 1 && N * P <= 256 && N * P * L <= AGG_MAX_NLP,
                  "%s: N=%d (<=%d), N*P=%d (<=256) or N*P*L=%d (<=%d) too large", who, N, AGG4_MAX_N, N * P, N * P * L, AGG_MAX_NLP);
  FAR3D_CHECK_ARG(feat_dtype == FAR3D_DT_F32 || feat_dtype == FAR3D_DT_BF16, "%s: unsupported feature dtype %d", who, feat_dtype);
  return FAR3D_OK;
}
static inline int agg_check_out_dtype(const char* who, int out_dt) {
  FAR3D_CHECK_ARG(out_dt == FAR3D_DT_F32 || out_dt == FAR3D_DT_BF16, "%s: unsupported output dtype %d", who, out_dt);
  return FAR3D_OK;
}
// `nsc`: the entry's name for the extent that has to fit 32 bits ("N*S*C", "N*S*C of one sample")
static inline int agg_check_extent(const char* who, int A, int N, int S, int C, const char* nsc) {
  FAR3D_CHECK_ARG(A >= 0 && S > 0 && (long)N * S * C < (1L << 31), "%s: bad sizes A=%d S=%d (%s must fit int32)", who, A, S, nsc);
  return FAR3D_OK;
}
// Variant 0 runs kernel 8 (factored softmax) where this holds, else kernel 7: the one statement of the rule (ops.aggregate_kernel8_applies)
static inline bool agg_kernel8_applies(const float* cam_tables, int N, int P, int L, int S, int C, size_t esz) {
  return cam_tables && N <= 8 && P <= 16 && L <= AGG_MAX_L && (size_t)N * S * C * esz < (1ull << 32);
}
// The level table (checked against S), the kernel parameters, the stride / alignment check of U and the offsets.  The sibling-split
// fields are left empty (variant 9 sets them).
static inline int agg_fill_params(const char* who, AggParams& prm, int A, int N, int S, int G, int P, int L, const int32_t* level_hw,
                                  const int32_t* level_start, const float* pc_range, float pad_h, float pad_w, const float* U, int ldU,
                                  int ldOffs, int out_dt) {
  prm.A = A; prm.N = N; prm.S = S; prm.P = P; prm.L = L;
  for (int l = 0; l < AGG_MAX_L; ++l) {
    prm.H[l] = l < L ? level_hw[2 * l] : 1;
    prm.W[l] = l < L ? level_hw[2 * l + 1] : 1;
    prm.start[l] = l < L ? level_start[l] : 0;
    if (l < L)
      FAR3D_CHECK_ARG(prm.H[l] > 0 && prm.W[l] > 0 && prm.start[l] >= 0 && prm.start[l] + prm.H[l] * prm.W[l] <= S,
                      "%s: level %d (%dx%d @%d) exceeds S=%d", who, l, prm.H[l], prm.W[l], prm.start[l], S);
  }
  for (int d = 0; d < 3; ++d) { prm.pc_lo[d] = pc_range[d]; prm.pc_span[d] = pc_range[3 + d] - pc_range[d]; }
  prm.pad_w = pad_w; prm.pad_h = pad_h;
  prm.ipw = 1.f / pad_w; prm.iph = 1.f / pad_h;
  for (int l = 0; l < AGG_MAX_L; ++l) { prm.Wf[l] = (float)prm.W[l]; prm.Hf[l] = (float)prm.H[l]; }
  prm.q_per_xcd = cdiv(A, 8);
  prm.split_part = nullptr; prm.split_tick = nullptr; prm.split_extra = 0;
  prm.out_dt = out_dt;
  prm.ldU = ldU > 0 ? ldU : L * P * G;
  prm.ldO = ldOffs > 0 ? ldOffs : P * 3;
  FAR3D_CHECK_ARG(prm.ldU >= L * P * G && prm.ldU % 4 == 0 && ((uintptr_t)U % 16) == 0 && prm.ldO >= P * 3,
                  "%s: U rows must be 16-byte aligned (ldU=%d) and strides >= row length", who, prm.ldU);
  return FAR3D_OK;
}

// What every launch of kernels 7 / 8 takes: grid, stream and the operands the two kernels have in common.
struct AggLaunch {
  dim3 grid; hipStream_t st; const void* feat; int feat_dtype; const float *ref, *offs, *l2i, *U; const int* perm; void* out;
};
// The row type TV in {float, bf16_t} and the point count PT in {13: the model's, unrolled; 0: any, read from AggParams} are chosen HERE,
// once: `f` is a generic lambda that gets a value of type TV and std::integral_constant<int, PT>.  ANY_P = false: only PT = 13 exists
// (variant 13, whose caller has checked P == 13).
template <bool ANY_P = true, typename F>
static inline void agg_for_row_and_points(int feat_dtype, int P, F f) {
  auto rows = [&](auto pt) { if (feat_dtype == FAR3D_DT_F32) f(float(), pt); else f(bf16_t(), pt); };
  if constexpr (ANY_P) { if (P != 13) return rows(std::integral_constant<int, 0>{}); }
  rows(std::integral_constant<int, 13>{});
}
template <bool SPLIT, bool SORTED, int DEAL, int PHASE = 0, bool BATCHED = false>
static inline void agg_launch_v8(const AggLaunch& k, const float* cam_tables, const AggParamsOf<BATCHED>& prm, const float4* qbase) {
  agg_for_row_and_points<PHASE == 0>(k.feat_dtype, prm.P, [&](auto row, auto pt) {
    using TV = decltype(row);
    hipLaunchKernelGGL((aggregate_v8_kernel<TV, decltype(pt)::value, 1, 4, AGG8_CAPW, SPLIT, SORTED, DEAL, PHASE, BATCHED>), k.grid, dim3(128), AGG8_LDS, k.st, (const TV*)k.feat, k.ref, k.offs, k.l2i, k.U, cam_tables, k.perm, k.out, prm, qbase);
  });
}
template <int OPT, bool BATCHED = false>
static inline void agg_launch_v7(const AggLaunch& k, const float* Vc, const AggParamsOf<BATCHED>& prm) {
  agg_for_row_and_points(k.feat_dtype, prm.P, [&](auto row, auto pt) {
    using TV = decltype(row);
    hipLaunchKernelGGL((aggregate_v7_kernel<TV, decltype(pt)::value, OPT, AGG7_CAPW, BATCHED>), k.grid, dim3(128), agg7_lds_bytes(prm.N, prm.P, prm.L), k.st, (const TV*)k.feat, k.ref, k.offs, k.l2i, k.U, Vc, k.perm, k.out, prm);
  });
}

extern "C" int far3d_aggregate_forward(const void* feat, int feat_dtype, const float* ref,
                                       const float* offsets, const float* lidar2img, const float* U,
                                       const float* Vc, const float* cam_tables, const int32_t* perm, void* out, int out_dt, int A, int N,
                                       int S, int C, int G, int P, int L, const int32_t* level_hw, const int32_t* level_start,
                                       const float* pc_range, float pad_h, float pad_w, int ldU, int ldOffs, int variant,
                                       float* split_partials, int32_t* split_tickets, int split_extra, const float* qbase,
                                       void* stream) {
  const char* who = "far3d_aggregate_forward";
  if (const int rc = agg_check_pointers(who, feat, ref, offsets, lidar2img, U, Vc, cam_tables, out, level_hw, level_start, pc_range)) return rc;
  if (const int rc = agg_check_shape(who, C, G, L, N, P, feat_dtype)) return rc;
  if (const int rc = agg_check_extent(who, A, N, S, C, "N*S*C")) return rc;
  FAR3D_CHECK_ARG(variant == 0 || variant == 3 || variant == 7 || variant == 8 || variant == 9 || variant == 11 || variant == 12 || variant == 13,
                  "far3d_aggregate_forward: unknown kernel variant %d (0 = default: 8 where it applies, else 7; 9 = 8 + sibling workgroups for heavy queries; 12 = 8 with the greedy dealing of round 4; 13 = 8 as TWO launches (list build, gather: A/B, sorted mode, workspace in split_partials / split_tickets); 3 = round-1 kernel, 11 = 7 + VALU reductions / packed FMAs)", variant);
  FAR3D_CHECK_ARG(variant != 9 || (perm && split_partials && split_tickets && split_extra > 0),
                  "far3d_aggregate_forward: variant 9 needs perm (A main + split_extra sibling entries from far3d_agg_order), split_partials, split_tickets and split_extra > 0");
  const bool v8_ok = agg_kernel8_applies(cam_tables, N, P, L, S, C, feat_dtype == FAR3D_DT_F32 ? 4 : 2);
  if (variant == 0) variant = v8_ok ? 8 : 7;
  FAR3D_CHECK_ARG(variant != 9 || v8_ok, "far3d_aggregate_forward: variant 9 needs what variant 8 needs (cam_tables, N <= 8, P <= 16)");
  FAR3D_CHECK_ARG((variant != 8 && variant != 12 && variant != 13) || v8_ok, "far3d_aggregate_forward: variant 8 needs cam_tables (far3d_agg_tables), N <= 8, P <= 16 and value maps < 4 GiB (N=%d P=%d)", N, P);
  FAR3D_CHECK_ARG(variant == 8 || variant == 9 || variant == 12 || variant == 13 || Vc, "far3d_aggregate_forward: variant %d needs Vc", variant);
  FAR3D_CHECK_ARG(variant != 13 || (qbase && v8_ok && perm && P == 13 && split_partials && split_tickets && ((uintptr_t)split_partials % 16) == 0),
                  "far3d_aggregate_forward: variant 13 (two-kernel split, A/B) needs the sorted mode's operands (qbase, perm), P = 13 and the workspace "
                  "FAR3D_AGG_LISTS_FLOATS(A) floats in split_partials + 2 * ceil8(A) int32 in split_tickets");
  FAR3D_CHECK_ARG(!qbase || ((variant == 8 || variant == 13) && perm && ((uintptr_t)qbase % 16) == 0 && L * P * 2 <= AGG8_WCAM),
                  "far3d_aggregate_forward: qbase (sorted mode) needs kernel 8 (variant %d after defaulting), perm, 16-byte alignment and L * P <= %d",
                  variant, AGG8_WCAM / 2);
  if (A == 0) return FAR3D_OK;
  AggParams prm;
  if (const int rc = agg_fill_params(who, prm, A, N, S, G, P, L, level_hw, level_start, pc_range, pad_h, pad_w, U, ldU, ldOffs, out_dt)) return rc;
  if (const int rc = agg_check_out_dtype(who, out_dt)) return rc;
  prm.split_part = split_partials; prm.split_tick = split_tickets; prm.split_extra = variant == 9 ? split_extra : 0;
  const AggLaunch k = {dim3(8 * prm.q_per_xcd + prm.split_extra), (hipStream_t)stream, feat, feat_dtype, ref, offsets, lidar2img, U, perm, out};
  const float4* qb = reinterpret_cast<const float4*>(qbase);
  if (variant == 11) agg_launch_v7<1>(k, Vc, prm);     // v7 with DPP / permlane reductions, early matrix loads, packed FMAs; A/B
  else if (variant == 8 && qbase) agg_launch_v8<false, true, -1>(k, cam_tables, prm, qb);      // the default kernel in sorted mode: operands in launch order
  else if (variant == 8) agg_launch_v8<false, false, -1>(k, cam_tables, prm, nullptr);      // factored softmax, specialised front ends, work-dealt items (default)
  else if (variant == 12) agg_launch_v8<false, false, 0>(k, cam_tables, prm, nullptr);     // kernel 8 with round 4's greedy dealing (A/B of the round-6 contiguous split)
  else if (variant == 9) agg_launch_v8<true, false, -1>(k, cam_tables, prm, nullptr);      // variant 8 + sibling workgroups (grid: + split_extra) for the queries far3d_agg_order marked as heavy
  else if (variant == 7) agg_launch_v7<0>(k, Vc, prm);     // 2 waves per query, levels split by parity, softmax over all 7 cameras
  else if (variant == 3) {     // workgroup-per-query kernel with per-sample row-pair gather (round 1)
    if (feat_dtype == FAR3D_DT_F32) hipLaunchKernelGGL((aggregate_v3_kernel<float, 2>), k.grid, dim3(256), agg3_lds_bytes(N, P, L), k.st, (const float*)feat, ref, offsets, lidar2img, U, Vc, perm, out, prm);
    else hipLaunchKernelGGL((aggregate_v3_kernel<bf16_t, 2, 1>), k.grid, dim3(256), agg3_lds_bytes(N, P, L), k.st, (const bf16_t*)feat, ref, offsets, lidar2img, U, Vc, perm, out, prm);
  } else if (variant == 13) {     // A/B: the sorted-mode kernel as two launches -- list build (global lists), then a pure gather
    agg_launch_v8<false, true, -1, 1>(k, cam_tables, prm, qb);
    if (feat_dtype == FAR3D_DT_F32) hipLaunchKernelGGL((aggregate_gather_kernel<float>), k.grid, dim3(128), 0, k.st, (const float*)feat, perm, out, prm);
    else hipLaunchKernelGGL((aggregate_gather_kernel<bf16_t>), k.grid, dim3(128), 0, k.st, (const bf16_t*)feat, perm, out, prm);
  }
  FAR3D_CHECK_LAUNCH("far3d_aggregate_forward");
  return FAR3D_OK;
}

// A batch of samples through kernel 8 / kernel 7 in one launch (include/far3d_hip.h).  The checks are far3d_aggregate_forward's, per
// sample; what belongs to the engine's one-sample call (perm, sorted mode, sibling split, A/B variants) has no batched form.  The one
// host path of far3d_aggregate_batched (no hole) and far3d_aggregate_batched_holes; `who` is the entry's name in the messages.
static int agg_batched(const char* who, const void* feat, int feat_dtype, const float* ref, const float* offsets,
                       const float* lidar2img, const float* U, const float* Vc, const float* cam_tables,
                       void* out, int out_dt, int B, int A, int N, int S, int C, int G, int P, int L,
                       const int32_t* level_hw, const int32_t* level_start, const float* pc_range,
                       float pad_h, float pad_w, int ldU, int ldOffs, const int32_t* hole_count, int hole_start, int hole_end,
                       void* stream) {
  if (const int rc = agg_check_shape(who, C, G, L, N, P, feat_dtype)) return rc;
  if (const int rc = agg_check_out_dtype(who, out_dt)) return rc;
  FAR3D_CHECK_ARG(B >= 0 && B <= 65535, "%s: B=%d out of range [0,65535] (the sample is the grid's y index)", who, B);
  if (const int rc = agg_check_extent(who, A, N, S, C, "N*S*C of one sample")) return rc;
  if (B == 0 || A == 0) return FAR3D_OK;
  if (const int rc = agg_check_pointers(who, feat, ref, offsets, lidar2img, U, Vc, cam_tables, out, level_hw, level_start, pc_range)) return rc;
  const bool v8 = agg_kernel8_applies(cam_tables, N, P, L, S, C, feat_dtype == FAR3D_DT_F32 ? 4 : 2);     // far3d_aggregate_forward's variant 0
  FAR3D_CHECK_ARG(v8 || Vc, "%s: kernel 7 (no cam_tables, N=%d > 8, P=%d > 16 or a sample's value maps >= 4 GiB) needs Vc", who, N, P);
  FAR3D_CHECK_ARG(!hole_count || (hole_start >= 0 && hole_start <= hole_end && hole_end <= A),
                  "%s: hole rows [%d + count, %d) must lie in the A=%d query rows (0 <= hole_start <= hole_end <= A)", who, hole_start, hole_end, A);
  AggParamsBatched prm;
  if (const int rc = agg_fill_params(who, prm, A, N, S, G, P, L, level_hw, level_start, pc_range, pad_h, pad_w, U, ldU, ldOffs, out_dt)) return rc;
  // no hole: the empty [0, 0), and as the count's address B words the kernel may read (the tables / Vc hold at least N * J floats per sample)
  prm.hole_count = hole_count ? hole_count : reinterpret_cast<const int*>(v8 ? cam_tables : Vc);
  prm.hole_start = hole_count ? hole_start : 0; prm.hole_end = hole_count ? hole_end : 0;
  // grid x: a multiple of 8 (blockIdx.x & 7 = XCD), y: the sample; no perm
  const AggLaunch k = {dim3(8 * prm.q_per_xcd, B), (hipStream_t)stream, feat, feat_dtype, ref, offsets, lidar2img, U, nullptr, out};
  if (v8) agg_launch_v8<false, false, -1, 0, true>(k, cam_tables, prm, nullptr);
  else agg_launch_v7<0, true>(k, Vc, prm);
  FAR3D_CHECK_LAUNCH(who);
  return FAR3D_OK;
}
extern "C" int far3d_aggregate_batched(const void* feat, int feat_dtype, const float* ref, const float* offsets,
                                       const float* lidar2img, const float* U, const float* Vc, const float* cam_tables,
                                       void* out, int out_dt, int B, int A, int N, int S, int C, int G, int P, int L,
                                       const int32_t* level_hw, const int32_t* level_start, const float* pc_range,
                                       float pad_h, float pad_w, int ldU, int ldOffs, void* stream) {
  return agg_batched("far3d_aggregate_batched", feat, feat_dtype, ref, offsets, lidar2img, U, Vc, cam_tables, out, out_dt, B, A, N, S, C, G, P, L,
                     level_hw, level_start, pc_range, pad_h, pad_w, ldU, ldOffs, nullptr, 0, 0, stream);
}
extern "C" int far3d_aggregate_batched_holes(const void* feat, int feat_dtype, const float* ref, const float* offsets,
                                             const float* lidar2img, const float* U, const float* Vc, const float* cam_tables,
                                             void* out, int out_dt, int B, int A, int N, int S, int C, int G, int P, int L,
                                             const int32_t* level_hw, const int32_t* level_start, const float* pc_range,
                                             float pad_h, float pad_w, int ldU, int ldOffs, const int32_t* hole_count, int hole_start,
                                             int hole_end, void* stream) {
  return agg_batched("far3d_aggregate_batched_holes", feat, feat_dtype, ref, offsets, lidar2img, U, Vc, cam_tables, out, out_dt, B, A, N, S, C, G,
                     P, L, level_hw, level_start, pc_range, pad_h, pad_w, ldU, ldOffs, hole_count, hole_start, hole_end, stream);
}

