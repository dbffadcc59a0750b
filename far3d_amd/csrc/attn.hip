// Decoder self-attention core: softmax(q k^T / sqrt(32)) v for 8 heads of dim 32,
// 1544 queries x 2312 keys, flash-style (the 1544 x 2312 x 8 score tensor never exists).
// Replaces the bmm/softmax/bmm inside torch.nn.MultiheadAttention as wrapped by mmcv MultiheadAttention
// (reference cfg projects/configs/far3d.py:112-116; in-tree statement models/utils/petr_transformer.py:286-326).
//
// Two kernels, both for one sample or (STREAMS below) for B samples in one launch:
//   attn_fwd_kernel         bf16 (and the fp32 A/B variants 2 / 4): K/V tiles of 64 keys go through LDS once per workgroup, the next
//                           tile's global loads are in flight during the MFMAs;
//   attn_f32_direct_kernel  fp32: a wave feeds its MFMAs from registers it loads itself, no LDS and no barrier in the key loop.
// The fragment layouts (S^T = K Q^T, one query per lane column -> the row max / row sum are 15 in-register ops + one cross-half shuffle
// and the running max / rescale are per-lane scalars), the Q load, the K/V staging, the scores and PV steps and the merge of the key
// parts are the shared pieces of attn_core.hpp, which attn_batch.hip (far3d_attention_batched) composes too.  What is written here is
// what only these kernels have: the key hole, each kernel's online-softmax step, the register-fed key loop, and the launchers.
#include "attn_core.hpp"
#include <atomic>

// STREAMS (far3d_attention_streams; both kernels below): B samples in one launch.  A workgroup is still (query block, head) of ONE sample
// and nothing in it knows about the others: the sample is one more grid index that moves the q / k / v / out bases by b times a
// per-sample stride (64-bit, elements) and selects hole_count[b]; the body behind the bases is the one-sample code, so out[b] has the
// bits of the one-sample launch on sample b.  The strides arrive as ONE trailing kernel argument that only the streams instantiations
// have (BS = AttnStreams; the one-sample instantiations have an empty pack: their argument list, and their code, are what they were).
struct AttnStreams { long bsq, bsk, bsv, bso; };
__device__ __forceinline__ const AttnStreams& attn_streams_arg(const AttnStreams& s) { return s; }
template <typename T>
__device__ __forceinline__ void attn_sample_bases(long b, const AttnStreams& s, int out_dt, const T* __restrict__& Q, const T* __restrict__& K,
                                                  const T* __restrict__& V, void* __restrict__& O, const int* __restrict__& hole_count) {
  Q += b * s.bsq; K += b * s.bsk; V += b * s.bsv;
  O = reinterpret_cast<char*>(O) + b * s.bso * (out_dt == FAR3D_DT_F32 ? 4 : 2);
  if (hole_count) hole_count += b;
}

template <typename T, int NS, typename... BS>     // NS: key-range parts per workgroup (2 waves each); BS: AttnStreams (blockIdx.z = sample) or nothing
__global__ __launch_bounds__(128 * NS) void attn_fwd_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                            const T* __restrict__ V, void* __restrict__ O, int out_dt, int Aq,
                                                            int Nk, int ldq, int ldk, int ldv, int ldo, float scale,
                                                            const int* __restrict__ hole_count, int hole_start, int hole_end, BS... bs) {
  if constexpr (sizeof...(BS) > 0) {
    const long b = blockIdx.z;
    attn_sample_bases(b, attn_streams_arg(bs...), out_dt, Q, K, V, O, hole_count);
  }
  // Workgroup = 64 queries of one head, 2*NS waves.  Waves 2p, 2p+1 walk part p of the keys for queries [0,32) / [32,64)
  // (flash-decoding style split); the NS partial (max, sum, O) states are merged through LDS at the end.  The loop is a chain
  // of latencies (global load -> LDS -> MFMA -> exp -> MFMA, ~1.7 us per 64-key tile), and 200 workgroups of 4 waves leave most
  // SIMDs with a single wave: more parts = fewer serial tiles per wave and more waves per SIMD (bf16: NS = 4, 9 tiles per wave
  // at 2312 keys; fp32 keeps NS = 2, its tiles do not fit four times into the static LDS budget).
  constexpr int KBYTES = AttCfg<T>::KBYTES, VBYTES = AttCfg<T>::VBYTES;
  // static LDS up to the 64 KB static limit (the shipped NS = 2 / 4 instantiations, unchanged); the 8-part variant's 78 KB are dynamic
  constexpr int LDS_TOTAL = NS * KBYTES + NS * VBYTES;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_dyn[];
  __shared__ __attribute__((aligned(16))) unsigned char smem_st[LDS_TOTAL <= 65536 ? LDS_TOTAL : 16];
  unsigned char* smem = LDS_TOTAL <= 65536 ? smem_st : smem_dyn;
  static_assert((NS - 1) * 2 * 18 * 64 * 4 <= NS * (KBYTES + VBYTES), "merge buffer must fit the tile buffers");
  unsigned char* KsAll = smem;
  unsigned char* VsAll = smem + NS * KBYTES;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l31 = lane & 31, hi = lane >> 5;
  const int half = wv >> 1;                     // key part of this wave, 0..NS-1
  const int head = blockIdx.y;
  const int q = blockIdx.x * 64 + (wv & 1) * 32 + l31;
  const bool q_ok = q < Aq;
  const int ntiles = (Nk + ATT_KT - 1) / ATT_KT;
  const int htiles = (ntiles + NS - 1) / NS;    // tiles per part; the last parts may have fewer (or none)
  // keys [hole_lo, hole_end) hold no query (fixed-capacity proposal mode): masked like keys past Nk; their K / V rows must be
  // finite (the producer zero-fills them) because a masked probability is an exact 0 that still multiplies V
  const int hole_lo = hole_count ? hole_start + min(max(*hole_count, 0), hole_end - hole_start) : hole_end;
  unsigned char* Ks = KsAll + half * KBYTES;
  unsigned char* Vs = VsAll + half * VBYTES;

  ATT_LOAD_Q(T, qf, Q + (long)q * ldq + head * ATT_D, q_ok, hi, scale);
  ATT_STAGE(T, NS, gload, lstore, kreg, vreg, K, V, ldk, ldv, head, Nk, ntiles, htiles, t, KsAll, VsAll);

  f32x16_t o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  gload(0);
  lstore();
  __syncthreads();
  for (int it = 0; it < htiles; ++it) {
    const bool more = it + 1 < htiles;
    if (more) gload(it + 1);
    const int tile = it + half * htiles;
    if (tile < ntiles && !(tile * ATT_KT >= hole_lo && (tile + 1) * ATT_KT <= hole_end)) {   // wave-uniform; tiles inside the hole are skipped
      ATT_SCORES(T, s, Ks, qf, l31, hi);
      // ---- online softmax (per-lane query)
      const int kbase = tile * ATT_KT + 4 * hi;
      float mloc = -INFINITY;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = s[u][r];
          if constexpr (sizeof(T) == 2) v *= scale;
          const int key = kbase + u * 32 + (r & 3) + 8 * (r >> 2);
          v = (key < Nk && !(key >= hole_lo && key < hole_end)) ? v : -INFINITY;
          s[u][r] = v;
          mloc = fmaxf(mloc, v);
        }
      mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
      const float m_new = fmaxf(m_run, mloc);
      const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
      const float alpha = (sizeof(T) == 2) ? __expf(m_run - m_use) : expf(m_run - m_use);   // m_run = -inf -> 0
      float psum = 0.f;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = (sizeof(T) == 2) ? __expf(s[u][r] - m_use) : expf(s[u][r] - m_use);
          s[u][r] = p;
          psum += p;
        }
      l_run = l_run * alpha + psum;
      m_run = m_new;
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] *= alpha;
      ATT_PV(T, o, s, Vs, l31, hi);
    }
    __syncthreads();
    if (more) lstore();
    __syncthreads();
  }

  // ---- merge the key parts: waves of parts 1..NS-1 publish (m, l, O) per lane, waves 0,1 combine in part order and store
  float l_tot = l_run + __shfl_xor(l_run, 32);   // both lane halves of a query share m_run
  float* mb = reinterpret_cast<float*>(smem);    // [NS-1 parts][2 waves][18][64 lanes]
  if (half >= 1) ATT_MERGE_PUBLISH(mb, (half - 1) * 2 + (wv & 1), lane, o, m_run, l_tot);
  __syncthreads();
  if (half == 0 && q_ok)
    ATT_MERGE_STORE(NS, mb, (p - 1) * 2 + (wv & 1), lane, o, m_run, l_tot, ATT_EXPF_DIFF, O, (long)q * ldo + head * ATT_D + 4 * hi, out_dt);
}

// fp32, round 6: the key loop WITHOUT LDS and without barriers.  The staged kernel above walks its 64-key tiles in lockstep (two workgroup
// barriers per tile: every wave of a SIMD is in its MFMA phase, then every wave in its exp phase), so the exact-fp32 MFMA pipe -- the
// bound of this kernel: 3.7 GFLOP at 256 FLOP / cycle / CU -- idles half the time.  Here a wave owns (32 queries, one part of the keys)
// and feeds the MFMAs from registers it loads itself: the A operand of S^T = K Q^T is lane (key, hi)'s 16 bytes of its key row, the A
// operand of O^T += V^T P^T one float of a value row per lane (128 contiguous bytes per half-wave) -- both are plain coalesced global
// loads of L2-resident rows (a head's K and V are 590 KB; workgroup id % heads = head, so with 8 heads an XCD's L2 holds ONE head).  The
// next 32-key tile's 20 loads are in flight under the current tile's 32 MFMAs; waves run free of each other until the merge of the key
// parts (one barrier).  Same arithmetic as the staged kernel per 32-key tile: exact products, fp32 accumulation, online softmax.
// BS: AttnStreams (blockIdx.y = sample, see STREAMS above) or nothing
template <int QB, int NS, int QW = 1, typename... BS>     // QB query blocks per workgroup, NS key parts (waves = QB * NS); a wave owns QW x 32 queries
__global__ __launch_bounds__(64 * QB * NS) void attn_f32_direct_kernel(const float* __restrict__ Q, const float* __restrict__ K,
                                                                      const float* __restrict__ V, void* __restrict__ O, int out_dt, int Aq,
                                                                      int Nk, int heads, int ldq, int ldk, int ldv, int ldo, float scale,
                                                                      const int* __restrict__ hole_count, int hole_start, int hole_end, BS... bs) {
  if constexpr (sizeof...(BS) > 0) {
    const long b = blockIdx.y;
    attn_sample_bases(b, attn_streams_arg(bs...), out_dt, Q, K, V, O, hole_count);
  }
  // QW = 2: one set of K / V fragments feeds two independent MFMA chains (queries l31 and 32 + l31 of the block): half the loads per
  // product and a second chain to issue while the first one's result is on its way
  __shared__ float mb[(NS - 1) * QB * QW * 18 * 64];
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6), l31 = lane & 31, hi = lane >> 5;
  const int part = wv / QB, qb = wv % QB;
  const int head = blockIdx.x % heads, qblk = blockIdx.x / heads;
  const int q0 = (qblk * QB + qb) * 32 * QW + l31;          // this lane's query of chain w: q0 + 32 w
  const int ntiles = (Nk + 31) >> 5;                       // 32-key tiles
  const int ptiles = (ntiles + NS - 1) / NS;
  const int t0 = part * ptiles, t1 = min(ntiles, t0 + ptiles);
  const int hole_lo = hole_count ? hole_start + min(max(*hole_count, 0), hole_end - hole_start) : hole_end;
  u32x4_t qf[QW][4];
#pragma unroll
  for (int w = 0; w < QW; ++w)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      qf[w][kk] = u32x4_t{0u, 0u, 0u, 0u};
      if (q0 + 32 * w < Aq) {
        const float4 v = *reinterpret_cast<const float4*>(Q + (long)(q0 + 32 * w) * ldq + head * ATT_D + kk * 8 + hi * 4);
        qf[w][kk] = u32x4_t{__float_as_uint(v.x * scale), __float_as_uint(v.y * scale), __float_as_uint(v.z * scale), __float_as_uint(v.w * scale)};
      }
    }
  const float* Kh = K + head * ATT_D + hi * 4;
  const float* Vh = V + head * ATT_D + l31;
  u32x4_t kf[2][4];
  float vf[2][16];
  auto fetch = [&](int tile, u32x4_t (&kd)[4], float (&vd)[16]) __attribute__((always_inline)) {
    const int k0 = tile * 32;
    const float* kr = Kh + (long)min(k0 + l31, Nk - 1) * ldk;           // rows past Nk: a valid row, masked below
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) kd[kk] = *reinterpret_cast<const u32x4_t*>(kr + kk * 8);
#pragma unroll
    for (int r = 0; r < 16; ++r) vd[r] = Vh[(long)min(k0 + (r & 3) + 8 * (r >> 2) + 4 * hi, Nk - 1) * ldv];
  };
  f32x16_t o[QW];
  float m_run[QW], l_run[QW];
#pragma unroll
  for (int w = 0; w < QW; ++w) {
#pragma unroll
    for (int r = 0; r < 16; ++r) o[w][r] = 0.f;
    m_run[w] = -INFINITY; l_run[w] = 0.f;
  }
  auto compute = [&](int tile, const u32x4_t (&kd)[4], const float (&vd)[16]) __attribute__((always_inline)) {
    if (tile * 32 >= hole_lo && (tile + 1) * 32 <= hole_end) return;      // wave-uniform: a tile inside the hole
    f32x16_t s[QW];
#pragma unroll
    for (int w = 0; w < QW; ++w)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[w][r] = 0.f;
    // exact-fp32 MFMAs of the chains interleaved: consecutive instructions do not wait for each other's accumulator
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const float ka[4] = {__uint_as_float(kd[kk].x), __uint_as_float(kd[kk].y), __uint_as_float(kd[kk].z), __uint_as_float(kd[kk].w)};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int w = 0; w < QW; ++w) {
          const float qe = __uint_as_float(e == 0 ? qf[w][kk].x : e == 1 ? qf[w][kk].y : e == 2 ? qf[w][kk].z : qf[w][kk].w);
          s[w] = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[e], qe, s[w], 0, 0, 0);
        }
    }
    const int kbase = tile * 32 + 4 * hi;
    const bool ragged = (tile + 1) * 32 > Nk || ((tile + 1) * 32 > hole_lo && tile * 32 < hole_end);     // wave-uniform: only a ragged tile is masked
    // e^(s - m) as the hardware's 2^x of one fma (1 ulp, the accuracy of expf without its ~18 instructions: per 32-key tile the exp phase
    // was as long as the 32 exact-fp32 MFMAs, profiles/r6/attn_f32_ab.txt)
    constexpr float LOG2E = 1.4426950408889634f;
#pragma unroll
    for (int w = 0; w < QW; ++w) {
      if (ragged) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kbase + (r & 3) + 8 * (r >> 2);
          s[w][r] = (key < Nk && !(key >= hole_lo && key < hole_end)) ? s[w][r] : -INFINITY;
        }
      }
      float mloc = fmaxf(fmaxf(fmaxf(s[w][0], s[w][1]), fmaxf(s[w][2], s[w][3])), fmaxf(fmaxf(s[w][4], s[w][5]), fmaxf(s[w][6], s[w][7])));
      mloc = fmaxf(mloc, fmaxf(fmaxf(fmaxf(s[w][8], s[w][9]), fmaxf(s[w][10], s[w][11])), fmaxf(fmaxf(s[w][12], s[w][13]), fmaxf(s[w][14], s[w][15]))));
      mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
      const float m_new = fmaxf(m_run[w], mloc);
      const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
      const float mneg = -m_use * LOG2E;
      const float alpha = __builtin_amdgcn_exp2f(fmaf(m_run[w], LOG2E, mneg));      // m_run = -inf -> 0
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(fmaf(s[w][r], LOG2E, mneg));
        s[w][r] = p;
        psum += p;
      }
      l_run[w] = l_run[w] * alpha + psum;
      m_run[w] = m_new;
      if (__ballot(alpha != 1.f)) {                                                // the running maximum moved for some query of the wave
#pragma unroll
        for (int r = 0; r < 16; ++r) o[w][r] *= alpha;
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
      for (int w = 0; w < QW; ++w) o[w] = __builtin_amdgcn_mfma_f32_32x32x2f32(vd[r], s[w][r], o[w], 0, 0, 0);
  };
  if (t0 < t1) {
    fetch(t0, kf[0], vf[0]);
    for (int tile = t0; tile < t1; tile += 2) {
      if (tile + 1 < t1) fetch(tile + 1, kf[1], vf[1]);
      compute(tile, kf[0], vf[0]);
      if (tile + 1 >= t1) break;
      if (tile + 2 < t1) fetch(tile + 2, kf[0], vf[0]);
      compute(tile + 1, kf[1], vf[1]);
    }
  }
  // ---- merge the key parts in part order, per chain w
  float l_tot[QW];
#pragma unroll
  for (int w = 0; w < QW; ++w) l_tot[w] = l_run[w] + __shfl_xor(l_run[w], 32);
  if (part >= 1) {
#pragma unroll
    for (int w = 0; w < QW; ++w) ATT_MERGE_PUBLISH(mb, ((part - 1) * QB + qb) * QW + w, lane, o[w], m_run[w], l_tot[w]);
  }
  __syncthreads();
  if (part != 0) return;
#pragma unroll
  for (int w = 0; w < QW; ++w) {
    const int q = q0 + 32 * w;
    if (q >= Aq) continue;
    ATT_MERGE_STORE(NS, mb, ((p - 1) * QB + qb) * QW + w, lane, o[w], m_run[w], l_tot[w], ATT_EXPF_DIFF, O, (long)q * ldo + head * ATT_D + 4 * hi, out_dt);
  }
}

template <int QB, int NS, int QW = 1>
static void launch_attn_f32_direct(const float* q, const float* k, const float* v, void* out, int out_dt, int Aq, int Nk, int heads, int ldq,
                                   int ldk, int ldv, int ldo, float scale, const int* hole_count, int hole_start, int hole_end, hipStream_t st) {
  const int nqb = (Aq + 32 * QB * QW - 1) / (32 * QB * QW);
  hipLaunchKernelGGL((attn_f32_direct_kernel<QB, NS, QW>), dim3(nqb * heads), dim3(64 * QB * NS), 0, st, q, k, v, out, out_dt, Aq, Nk, heads, ldq,
                     ldk, ldv, ldo, scale, hole_count, hole_start, hole_end);
}

// A/B switch of the fp32 instantiation (far3d_attention_f32_variant; tools/probe/attn_f32_ab.py): 0 = default
static std::atomic<int> g_attn_f32_variant{0};
extern "C" int far3d_attention_f32_variant(int variant) {
  if (variant < 0) return g_attn_f32_variant.load(std::memory_order_relaxed);
  return g_attn_f32_variant.exchange(variant, std::memory_order_relaxed);
}

// the key hole of the two entries below: inside [0, Nk]; without a count there is none
static int attn_check_hole(const char* who, const int32_t* hole_count, int& hole_start, int& hole_end, int Nk) {
  FAR3D_CHECK_ARG(!hole_count || (0 <= hole_start && hole_start <= hole_end && hole_end <= Nk), "%s: bad key hole [%d, %d) for Nk=%d", who,
                  hole_start, hole_end, Nk);
  if (!hole_count) hole_start = hole_end = 0;
  return FAR3D_OK;
}

extern "C" int far3d_attention_forward(const void* q, const void* k, const void* v, int dtype, void* out, int out_dt, int Aq,
                                       int Nk, int heads, int head_dim, int ldq, int ldk, int ldv, int ldo,
                                       float scale, const int32_t* hole_count, int hole_start, int hole_end, void* stream) {
  const char* who = "far3d_attention_forward";
  if (const int rc = attn_check_operands(who, q, k, v, out, head_dim, false, 1, Aq, Nk, heads)) return rc;
  if (const int rc = attn_check_dtype(who, dtype)) return rc;
  if (const int rc = attn_check_hole(who, hole_count, hole_start, hole_end, Nk)) return rc;
  if (const int rc = attn_check_layout(who, q, k, v, out, dtype, out_dt, ldq, ldk, ldv, ldo, nullptr)) return rc;
  dim3 grid((Aq + 63) / 64, heads);
  hipStream_t st = (hipStream_t)stream;
  // key parts per workgroup (2 waves each): fp32 2, bf16 4 (an 8-part bf16 instantiation was measured in round 4 -- 27.4 vs 28 us,
  // profiles/r4/attn_parts8.txt: the per-tile MFMA -> exp -> MFMA chain is what a wave waits on -- and removed)
  if (dtype == FAR3D_DT_F32) {
    // fp32 (the in-tolerance engine's decoder): the register-fed kernel (attn_f32_direct_kernel) since round 6; the staged kernel with 4
    // key parts (its four fp32 K / V tile pairs, 72 KB, are dynamic LDS) or 2 (round 5) stays selectable for A/B.
    // far3d_attention_f32_variant (A/B): 0 the default; 10 * QB + NS (+ 100: 64 queries per wave) a register-fed instantiation; 2 / 4 the
    // staged kernel with that many key parts (round 5 / earlier in round 6)
    const int parts = g_attn_f32_variant.load(std::memory_order_relaxed);
    const float* qf_ = (const float*)q; const float* kf_ = (const float*)k; const float* vf_ = (const float*)v;
#define FAR3D_ATTN_DIRECT(QB_, NS_, QW_) launch_attn_f32_direct<QB_, NS_, QW_>(qf_, kf_, vf_, out, out_dt, Aq, Nk, heads, ldq, ldk, ldv, ldo, scale, \
                                                                              (const int*)hole_count, hole_start, hole_end, st)
    // measured at 1544 x 2312 x 8 heads (profiles/r6/attn_f32_ab.txt): staged 4 parts 80 us; register-fed with expf 75; with the one-fma
    // exp2 62-63 in every shape tried (2 x 4, 1 x 4, 1 x 8 with 64 queries per wave) -- the exact-fp32 MFMA runs at the VECTOR fp32 rate
    // (MI355X guide) and shares its time with the softmax's VALU work; 200-392 workgroups on 256 CUs leave a quarter of the chip idle
    if (parts == 0 || parts == 24) FAR3D_ATTN_DIRECT(2, 4, 1);
    else if (parts == 14) FAR3D_ATTN_DIRECT(1, 4, 1);
    else if (parts == 118) FAR3D_ATTN_DIRECT(1, 8, 2);      // 64 queries per wave
#undef FAR3D_ATTN_DIRECT
    else if (parts == 4) {
      constexpr int lds = 4 * (AttCfg<float>::KBYTES + AttCfg<float>::VBYTES);
      static std::atomic<unsigned long long> lds_ok{0};
      if (const int rc = far3d_allow_lds(reinterpret_cast<const void*>(&attn_fwd_kernel<float, 4>), lds, lds_ok, "far3d_attention_forward")) return rc;
      hipLaunchKernelGGL((attn_fwd_kernel<float, 4>), grid, dim3(512), lds, st, (const float*)q, (const float*)k, (const float*)v, out, out_dt,
                         Aq, Nk, ldq, ldk, ldv, ldo, scale, (const int*)hole_count, hole_start, hole_end);
    } else {
      FAR3D_CHECK_ARG(parts == 2, "far3d_attention_forward: far3d_attention_f32_variant(%d) names no fp32 instantiation", parts);
      hipLaunchKernelGGL((attn_fwd_kernel<float, 2>), grid, dim3(256), 0, st, (const float*)q, (const float*)k, (const float*)v, out, out_dt,
                         Aq, Nk, ldq, ldk, ldv, ldo, scale, (const int*)hole_count, hole_start, hole_end);
    }
  } else {
    hipLaunchKernelGGL((attn_fwd_kernel<bf16_t, 4>), grid, dim3(512), 0, st, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v,
                       out, out_dt, Aq, Nk, ldq, ldk, ldv, ldo, scale, (const int*)hole_count, hole_start, hole_end);
  }
  FAR3D_CHECK_LAUNCH("far3d_attention_forward");
  return FAR3D_OK;
}

// far3d_attention_forward for B samples in one launch: the streams instantiations (STREAMS above) of the two kernels that entry launches
// by default -- bf16: the staged kernel with 4 key parts, grid (query blocks, heads, B); fp32: the register-fed kernel 2 x 4, grid
// (query blocks * heads, B).  far3d_attention_f32_variant is not read: a batch always takes the default fp32 form.
extern "C" int far3d_attention_streams(const void* q, const void* k, const void* v, int dtype, void* out, int out_dt, int B, int Aq, int Nk,
                                       int heads, int head_dim, int ldq, int ldk, int ldv, int ldo, long bsq, long bsk, long bsv, long bso,
                                       float scale, const int32_t* hole_count, int hole_start, int hole_end, void* stream) {
  const char* who = "far3d_attention_streams";
  const long strides[4] = {bsq, bsk, bsv, bso};
  if (const int rc = attn_check_operands(who, q, k, v, out, head_dim, true, B, Aq, Nk, heads)) return rc;
  FAR3D_CHECK_ARG(B <= 65535 && heads <= 65535, "%s: B=%d / heads=%d above the grid limit 65535", who, B, heads);
  if (const int rc = attn_check_dtype(who, dtype)) return rc;
  if (const int rc = attn_check_hole(who, hole_count, hole_start, hole_end, Nk)) return rc;
  if (const int rc = attn_check_layout(who, q, k, v, out, dtype, out_dt, ldq, ldk, ldv, ldo, strides)) return rc;
  const AttnStreams bs{bsq, bsk, bsv, bso};
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FAR3D_DT_F32) {
    constexpr int QB = 2, NS = 4, QW = 1;
    const int nqb = (Aq + 32 * QB * QW - 1) / (32 * QB * QW);
    hipLaunchKernelGGL((attn_f32_direct_kernel<QB, NS, QW, AttnStreams>), dim3(nqb * heads, B), dim3(64 * QB * NS), 0, st, (const float*)q,
                       (const float*)k, (const float*)v, out, out_dt, Aq, Nk, heads, ldq, ldk, ldv, ldo, scale, (const int*)hole_count, hole_start,
                       hole_end, bs);
  } else {
    hipLaunchKernelGGL((attn_fwd_kernel<bf16_t, 4, AttnStreams>), dim3((Aq + 63) / 64, heads, B), dim3(512), 0, st, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)v, out, out_dt, Aq, Nk, ldq, ldk, ldv, ldo, scale, (const int*)hole_count, hole_start,
                       hole_end, bs);
  }
  FAR3D_CHECK_LAUNCH(who);
  return FAR3D_OK;
}
