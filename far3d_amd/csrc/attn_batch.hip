// Batched, masked multi-head attention core (far3d_attention_batched): per sample b and head h
//   out[b] = softmax(q[b] k[b]^T * scale + M[b,h] + P[b]) v[b],   head_dim 32, flash-style (no score tensor in HBM).
// The attention half of a decoder layer run OUTSIDE the engine: any batch, the `attn_mask` of torch.nn.MultiheadAttention (bool / byte
// or additive f32, shared (Aq, Nk) or per (sample, head)) and its `key_padding_mask`.  far3d_attention_forward (attn.hip: one sample, the
// engine's key hole) stays the engine's kernel.
//
// gfx950 mapping: the LDS-staged structure of attn.hip's attn_fwd_kernel, built from the same pieces (attn_core.hpp: fragment layouts, Q
// load, K/V staging, the scores and PV steps, the merge of the key parts).  Workgroup = 64 queries of one (sample, head), 2 * NS waves;
// waves 2p, 2p + 1 walk part p of the 64-key tiles for queries [0,32) / [32,64); scores are computed transposed (S^T = K Q^T), so a lane
// column is one query and the running max / sum are per-lane scalars; the NS partial states are merged through LDS in part order.  One
// launch covers every (query block, head, sample): grid (ceil(Aq / 64), heads, B).  The bits of a sample depend on its own operands only.
// What is written here is what only this kernel has: the masks and its online-softmax step.
//
// Masks.  Exclusions (byte mask, key padding, keys past Nk) are gathered with the KEY on the lane: for each of the wave's 32 query rows
// the 64 lanes read 64 consecutive mask bytes (one 64-byte segment per row) and a ballot turns them into the row's 64-bit exclusion
// word, kept by the lane that owns the row.  An additive f32 mask goes through a wave-private LDS piece of 32 rows x 16 keys: lanes read
// 16 consecutive floats of 4 rows per instruction and each lane picks its query's values in the S^T register order.  Excluded scores are
// -inf; m_use = (m == -inf ? 0 : m) keeps a fully excluded tile from touching a row's state, and a row without any key ends as 0 / 0 =
// NaN like torch's softmax.  Probabilities and rescale factors are exp2((s - m) * log2e): the subtraction comes first, so the error does
// not grow with |m| (additive masks make |s| large).
#include "attn_core.hpp"

#define ATB_MROW 17                  // floats per row of the additive-mask piece (16 keys + 1: the per-query column reads hit 32 banks)
#define ATB_MPIECE (32 * ATB_MROW)   // floats per wave

#define FAR3D_MASK_NONE 0
#define FAR3D_MASK_BYTES 1
#define FAR3D_MASK_F32 2

// e^(a - b) with the subtraction first: one rounding of the difference, then the hardware's 2^x (1 ulp).  a = -inf -> 0.
__device__ __forceinline__ float atb_exp_diff(float a, float b) { return __builtin_amdgcn_exp2f((a - b) * 1.4426950408889634f); }

// LDS operations of one wave execute in order; this keeps the compiler from moving them across the hand-over between lanes
__device__ __forceinline__ void atb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct AtbArgs {
  const void *q, *k, *v;
  void* out;
  int out_dt, Aq, Nk, ldq, ldk, ldv, ldo;
  long bsq, bsk, bsv, bso;
  float scale;
  const void* mask;        // bytes (kind 1) or f32 (kind 2); NULL: none
  int ldm;
  long mask_bs;            // elements between the matrices of consecutive (sample, head) pairs; 0: one matrix for all
  const uint8_t* kpad;     // (B, Nk) bytes, contiguous; NULL: none
};

template <typename T, int NS, int MK>     // NS: key-range parts per workgroup (2 waves each); MK: the mask kind (0 none, 1 bytes, 2 f32)
__global__ __launch_bounds__(128 * NS) void attn_batch_kernel(const AtbArgs a) {
  constexpr bool MF32 = MK == FAR3D_MASK_F32, MBYTE = MK == FAR3D_MASK_BYTES;
  constexpr int KBYTES = AttCfg<T>::KBYTES, VBYTES = AttCfg<T>::VBYTES;
  constexpr int MBYTES = MF32 ? 2 * NS * ATB_MPIECE * 4 : 0;
  constexpr int LDS_TOTAL = NS * KBYTES + NS * VBYTES + MBYTES;
  static_assert(LDS_TOTAL <= 65536, "static LDS");
  static_assert((NS - 1) * 2 * 18 * 64 * 4 <= NS * (KBYTES + VBYTES), "merge buffer must fit the tile buffers");
  __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_TOTAL];
  unsigned char* KsAll = smem;
  unsigned char* VsAll = smem + NS * KBYTES;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l31 = lane & 31, hi = lane >> 5;
  const int half = wv >> 1;                     // key part of this wave, 0..NS-1
  const int head = blockIdx.y, b = blockIdx.z;
  const int Aq = a.Aq, Nk = a.Nk;
  const int qw0 = blockIdx.x * 64 + (wv & 1) * 32;      // first query row of this wave
  const int q = qw0 + l31;
  const bool q_ok = q < Aq;
  const int ntiles = (Nk + ATT_KT - 1) / ATT_KT;
  const int htiles = (ntiles + NS - 1) / NS;    // tiles per part; the last parts may have fewer (or none)
  const T* Q = reinterpret_cast<const T*>(a.q) + b * a.bsq;
  const T* K = reinterpret_cast<const T*>(a.k) + b * a.bsk;
  const T* V = reinterpret_cast<const T*>(a.v) + b * a.bsv;
  const long mask_off = ((long)b * gridDim.y + head) * a.mask_bs;
  const uint8_t* Mb = MBYTE ? reinterpret_cast<const uint8_t*>(a.mask) + mask_off : nullptr;
  const float* Mf = MF32 ? reinterpret_cast<const float*>(a.mask) + mask_off : nullptr;
  const uint8_t* Pb = a.kpad ? a.kpad + (long)b * Nk : nullptr;
  const float scale = a.scale;
  unsigned char* Ks = KsAll + half * KBYTES;
  unsigned char* Vs = VsAll + half * VBYTES;
  float* Ms = reinterpret_cast<float*>(smem + NS * (KBYTES + VBYTES)) + wv * ATB_MPIECE;    // MF32 only

  ATT_LOAD_Q(T, qf, Q + (long)q * a.ldq + head * ATT_D, q_ok, hi, scale);
  ATT_STAGE(T, NS, gload, lstore, kreg, vreg, K, V, a.ldk, a.ldv, head, Nk, ntiles, htiles, t, KsAll, VsAll);

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
    if (tile < ntiles) {   // wave-uniform
      // ---- exclusion word of this lane's query: bit j = key tile * 64 + j is excluded.  The key is on the lane while it is gathered.
      // Every load is unconditional (row and key clamped into the matrix: a key past Nk is excluded below whatever was read, a row
      // past Aq is never stored) and issued before the MFMAs that hide its latency.
      const int mkey = tile * ATT_KT + lane;
      const bool k_in = mkey < Nk;
      const int mkey_c = min(mkey, Nk - 1);
      const uint8_t pbyte = Pb ? Pb[mkey_c] : (uint8_t)0;
      uint8_t mbytes[32];
      if constexpr (MBYTE) {
#pragma unroll
        for (int i = 0; i < 32; ++i) mbytes[i] = Mb[(long)min(qw0 + i, Aq - 1) * a.ldm + mkey_c];
      }

      ATT_SCORES(T, s, Ks, qf, l31, hi);
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) s[u][r] *= scale;
      }
      unsigned long long ex = __ballot(!k_in || pbyte != 0);
      if constexpr (MBYTE) {
#pragma unroll
        for (int i = 0; i < 32; ++i) {
          const unsigned long long bits = __ballot(mbytes[i] != 0);
          if (l31 == i) ex |= bits;
        }
      }
      ex >>= 4 * hi;      // bit of register (u, r): 32 u + (r & 3) + 8 (r >> 2)
      const uint32_t exw[2] = {(uint32_t)ex, (uint32_t)(ex >> 32)};
      // ---- additive mask: four pieces of 32 rows x 16 keys through this wave's LDS piece
      if constexpr (MF32) {
        const int pk = lane & 15, pr = lane >> 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int key = min(tile * ATT_KT + 16 * j + pk, Nk - 1);      // clamped like the byte mask's loads
          float mv[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) mv[i] = Mf[(long)min(qw0 + 4 * i + pr, Aq - 1) * a.ldm + key];
          atb_wave_sync();     // the previous piece has been read
#pragma unroll
          for (int i = 0; i < 8; ++i) Ms[(4 * i + pr) * ATB_MROW + pk] = mv[i];
          atb_wave_sync();
#pragma unroll
          for (int rr = 0; rr < 8; ++rr) {
            const int r = 8 * (j & 1) + rr;
            s[j >> 1][r] += Ms[l31 * ATB_MROW + (rr & 3) + 8 * (rr >> 2) + 4 * hi];
          }
        }
      }
      // ---- online softmax (per-lane query)
      float mloc = -INFINITY;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = ((exw[u] >> ((r & 3) + 8 * (r >> 2))) & 1u) ? -INFINITY : s[u][r];
          s[u][r] = v;
          mloc = fmaxf(mloc, v);
        }
      mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
      const float m_new = fmaxf(m_run, mloc);
      const float m_use = (m_new == -INFINITY) ? 0.f : m_new;    // a tile without a key for this row leaves its state untouched
      const float alpha = atb_exp_diff(m_run, m_use);            // m_run = -inf -> 0
      float psum = 0.f;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = atb_exp_diff(s[u][r], m_use);
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
    ATT_MERGE_STORE(NS, mb, (p - 1) * 2 + (wv & 1), lane, o, m_run, l_tot, atb_exp_diff, a.out,
                    b * a.bso + (long)q * a.ldo + head * ATT_D + 4 * hi, a.out_dt);
}

extern "C" int far3d_attention_batched(const void* q, const void* k, const void* v, int dtype, void* out, int out_dt, int B, int Aq, int Nk,
                                       int heads, int head_dim, int ldq, int ldk, int ldv, int ldo, long bsq, long bsk, long bsv, long bso,
                                       float scale, const void* attn_mask, int mask_kind, int ldm, long mask_bstride,
                                       const uint8_t* key_padding, void* stream) {
  const char* who = "far3d_attention_batched";
  const long strides[4] = {bsq, bsk, bsv, bso};
  if (const int rc = attn_check_operands(who, q, k, v, out, head_dim, true, B, Aq, Nk, heads)) return rc;
  FAR3D_CHECK_ARG(B <= 65535 && heads <= 65535, "%s: B=%d / heads=%d above the grid limit 65535", who, B, heads);
  if (const int rc = attn_check_dtype(who, dtype)) return rc;
  FAR3D_CHECK_ARG(out_dt == FAR3D_DT_F32 || out_dt == FAR3D_DT_BF16, "%s: unsupported output dtype %d", who, out_dt);
  FAR3D_CHECK_ARG(mask_kind == FAR3D_MASK_NONE || mask_kind == FAR3D_MASK_BYTES || mask_kind == FAR3D_MASK_F32,
                  "%s: unknown mask_kind %d (0 none, 1 bytes, 2 f32 additive)", who, mask_kind);
  if (mask_kind != FAR3D_MASK_NONE) {
    FAR3D_CHECK_ARG(attn_mask, "%s: mask_kind %d without an attn_mask pointer", who, mask_kind);
    FAR3D_CHECK_ARG(ldm >= Nk, "%s: mask row stride ldm=%d below Nk=%d", who, ldm, Nk);
    FAR3D_CHECK_ARG(mask_bstride >= 0, "%s: negative mask batch stride", who);
    FAR3D_CHECK_ARG(mask_kind != FAR3D_MASK_F32 || (uintptr_t)attn_mask % 4 == 0, "%s: f32 mask pointer not 4-byte aligned", who);
  }
  FAR3D_CHECK_ARG(ldq >= heads * ATT_D && ldk >= heads * ATT_D && ldv >= heads * ATT_D && ldo >= heads * ATT_D,
                  "%s: a row stride is below heads * 32 = %d", who, heads * ATT_D);
  if (const int rc = attn_check_layout(who, q, k, v, out, dtype, out_dt, ldq, ldk, ldv, ldo, strides)) return rc;
  AtbArgs a;
  a.q = q; a.k = k; a.v = v; a.out = out; a.out_dt = out_dt; a.Aq = Aq; a.Nk = Nk;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.bsq = bsq; a.bsk = bsk; a.bsv = bsv; a.bso = bso; a.scale = scale;
  a.mask = mask_kind == FAR3D_MASK_NONE ? nullptr : attn_mask; a.ldm = ldm; a.mask_bs = mask_bstride;
  a.kpad = key_padding;
  const dim3 grid((Aq + 63) / 64, heads, B);
  hipStream_t st = (hipStream_t)stream;
  // key parts per workgroup (2 waves each) as far3d_attention_forward's staged kernel ships them: fp32 2, bf16 4
  if (dtype == FAR3D_DT_F32) {
    if (mask_kind == FAR3D_MASK_F32) hipLaunchKernelGGL((attn_batch_kernel<float, 2, FAR3D_MASK_F32>), grid, dim3(256), 0, st, a);
    else if (mask_kind == FAR3D_MASK_BYTES) hipLaunchKernelGGL((attn_batch_kernel<float, 2, FAR3D_MASK_BYTES>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((attn_batch_kernel<float, 2, FAR3D_MASK_NONE>), grid, dim3(256), 0, st, a);
  } else {
    if (mask_kind == FAR3D_MASK_F32) hipLaunchKernelGGL((attn_batch_kernel<bf16_t, 4, FAR3D_MASK_F32>), grid, dim3(512), 0, st, a);
    else if (mask_kind == FAR3D_MASK_BYTES) hipLaunchKernelGGL((attn_batch_kernel<bf16_t, 4, FAR3D_MASK_BYTES>), grid, dim3(512), 0, st, a);
    else hipLaunchKernelGGL((attn_batch_kernel<bf16_t, 4, FAR3D_MASK_NONE>), grid, dim3(512), 0, st, a);
  }
  FAR3D_CHECK_LAUNCH(who);
  return FAR3D_OK;
}
