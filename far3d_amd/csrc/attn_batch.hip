// Batched, masked multi-head attention core (far3d_attention_batched): per sample b and head h
//   out[b] = softmax(q[b] k[b]^T * scale + M[b,h] + P[b]) v[b],   head_dim 32, flash-style (no score tensor in HBM).
// The attention half of a decoder layer run OUTSIDE the engine: any batch, the `attn_mask` of torch.nn.MultiheadAttention (bool / byte
// or additive f32, shared (Aq, Nk) or per (sample, head)) and its `key_padding_mask`.  attn.hip (far3d_attention_forward: one sample, the
// engine's key hole) is untouched and stays the engine's kernel.
//
// gfx950 mapping: the LDS-staged structure of attn.hip's attn_fwd_kernel.  Workgroup = 64 queries of one (sample, head), 2 * NS waves;
// waves 2p, 2p + 1 walk part p of the 64-key tiles for queries [0,32) / [32,64); scores are computed transposed (S^T = K Q^T), so a lane
// column is one query and the running max / sum are per-lane scalars; the NS partial states are merged through LDS in part order.  One
// launch covers every (query block, head, sample): grid (ceil(Aq / 64), heads, B).  The bits of a sample depend on its own operands only.
//
// Masks.  Exclusions (byte mask, key padding, keys past Nk) are gathered with the KEY on the lane: for each of the wave's 32 query rows
// the 64 lanes read 64 consecutive mask bytes (one 64-byte segment per row) and a ballot turns them into the row's 64-bit exclusion
// word, kept by the lane that owns the row.  An additive f32 mask goes through a wave-private LDS piece of 32 rows x 16 keys: lanes read
// 16 consecutive floats of 4 rows per instruction and each lane picks its query's values in the S^T register order.  Excluded scores are
// -inf; m_use = (m == -inf ? 0 : m) keeps a fully excluded tile from touching a row's state, and a row without any key ends as 0 / 0 =
// NaN like torch's softmax.  Probabilities and rescale factors are exp2((s - m) * log2e): the subtraction comes first, so the error does
// not grow with |m| (additive masks make |s| large).
#include "common.hpp"

typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 bf16x8_t;
typedef __attribute__((__vector_size__(16 * sizeof(float)))) float f32x16_t;
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

#define ATB_D 32
#define ATB_KT 64
#define ATB_MROW 17                  // floats per row of the additive-mask piece (16 keys + 1: the per-query column reads hit 32 banks)
#define ATB_MPIECE (32 * ATB_MROW)   // floats per wave

#define FAR3D_MASK_NONE 0
#define FAR3D_MASK_BYTES 1
#define FAR3D_MASK_F32 2

template <typename T> struct BCfg;
template <> struct BCfg<bf16_t> { static constexpr int KROW = 80, VROW = 144, KSUB = 2, CH = 1; };   // bytes
template <> struct BCfg<float> { static constexpr int KROW = 144, VROW = 144, KSUB = 4, CH = 2; };

template <typename T>
__device__ __forceinline__ void mma_atb(f32x16_t& acc, const u32x4_t& a, const u32x4_t& b) {
  if constexpr (sizeof(T) == 2) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
  }
}

// position of key k inside a permuted 16-key group: quads 1 and 2 swapped (matches the S^T register order)
__device__ __forceinline__ int atb_vt_pos(int key) {
  const int quad = (key >> 2) & 3;
  const int sw = (quad == 1) ? 2 : ((quad == 2) ? 1 : quad);
  return (key & ~15) | (sw << 2) | (key & 3);
}

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
  constexpr int NT = 128 * NS;
  constexpr bool MF32 = MK == FAR3D_MASK_F32, MBYTE = MK == FAR3D_MASK_BYTES;
  constexpr int KROW = BCfg<T>::KROW, VROW = BCfg<T>::VROW, KSUB = BCfg<T>::KSUB, CH = BCfg<T>::CH;
  constexpr int E = 16 / sizeof(T);
  constexpr int KBYTES = ATB_KT * KROW, VBYTES = (sizeof(T) == 2 ? ATB_D : ATB_KT) * VROW;
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
  const int ntiles = (Nk + ATB_KT - 1) / ATB_KT;
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

  // Q fragments (B operand: column = query), held in registers for the whole key loop
  u32x4_t qf[KSUB];
#pragma unroll
  for (int kk = 0; kk < KSUB; ++kk) {
    qf[kk] = u32x4_t{0u, 0u, 0u, 0u};
    if (q_ok) {
      const T* src = Q + (long)q * a.ldq + head * ATB_D + kk * 2 * E + hi * E;
      qf[kk] = *reinterpret_cast<const u32x4_t*>(src);
      if constexpr (sizeof(T) == 4) {  // torch scales q before the product (F.multi_head_attention_forward)
        qf[kk].x = __float_as_uint(__uint_as_float(qf[kk].x) * scale);
        qf[kk].y = __float_as_uint(__uint_as_float(qf[kk].y) * scale);
        qf[kk].z = __float_as_uint(__uint_as_float(qf[kk].z) * scale);
        qf[kk].w = __float_as_uint(__uint_as_float(qf[kk].w) * scale);
      }
    }
  }

  // cooperative staging of NS K/V tiles per iteration (one per part): chunk id -> (part, key, 16-B piece)
  constexpr int CPK = ATB_D * sizeof(T) / 16;  // 16-B chunks per key row: 4 (bf16) / 8 (f32)
  constexpr int CH2 = 2 * CH;
  u32x4_t kreg[CH2], vreg[CH2];
  auto gload = [&](int it) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < CH2; ++c) {
      const int id = t + c * NT, h = id / (ATB_KT * CPK), rem = id % (ATB_KT * CPK), key = rem / CPK, ck = rem % CPK;
      const int tl = it + h * htiles;
      const int gk = tl * ATB_KT + key;
      kreg[c] = u32x4_t{0u, 0u, 0u, 0u};
      vreg[c] = u32x4_t{0u, 0u, 0u, 0u};
      if (tl < ntiles && gk < Nk) {
        kreg[c] = *reinterpret_cast<const u32x4_t*>(K + (long)gk * a.ldk + head * ATB_D + ck * E);
        vreg[c] = *reinterpret_cast<const u32x4_t*>(V + (long)gk * a.ldv + head * ATB_D + ck * E);
      }
    }
  };
  auto lstore = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < CH2; ++c) {
      const int id = t + c * NT, h = id / (ATB_KT * CPK), rem = id % (ATB_KT * CPK), key = rem / CPK, ck = rem % CPK;
      *reinterpret_cast<u32x4_t*>(KsAll + h * KBYTES + key * KROW + ck * 16) = kreg[c];
      unsigned char* vs = VsAll + h * VBYTES;
      if constexpr (sizeof(T) == 2) {
        const int pos = atb_vt_pos(key);
        const uint32_t w[4] = {vreg[c].x, vreg[c].y, vreg[c].z, vreg[c].w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint16_t val = (uint16_t)((e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu));
          *reinterpret_cast<uint16_t*>(vs + (ck * 8 + e) * VROW + pos * 2) = val;
        }
      } else {
        *reinterpret_cast<u32x4_t*>(vs + key * VROW + ck * 16) = vreg[c];
      }
    }
  };

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
      const int mkey = tile * ATB_KT + lane;
      const bool k_in = mkey < Nk;
      const int mkey_c = min(mkey, Nk - 1);
      const uint8_t pbyte = Pb ? Pb[mkey_c] : (uint8_t)0;
      uint8_t mbytes[32];
      if constexpr (MBYTE) {
#pragma unroll
        for (int i = 0; i < 32; ++i) mbytes[i] = Mb[(long)min(qw0 + i, Aq - 1) * a.ldm + mkey_c];
      }

      // ---- S^T = K Q^T for the two 32-key sub-tiles
      f32x16_t s[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[u][r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < KSUB; ++kk) {
          const u32x4_t ka = *reinterpret_cast<const u32x4_t*>(Ks + (u * 32 + l31) * KROW + kk * 32 + hi * 16);
          mma_atb<T>(s[u], ka, qf[kk]);
        }
      }
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
          const int key = min(tile * ATB_KT + 16 * j + pk, Nk - 1);      // clamped like the byte mask's loads
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

      // ---- O^T += V^T P^T
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            u32x4_t pb;
            pb.x = pack_bf16x2(s[u][8 * g + 0], s[u][8 * g + 1]);
            pb.y = pack_bf16x2(s[u][8 * g + 2], s[u][8 * g + 3]);
            pb.z = pack_bf16x2(s[u][8 * g + 4], s[u][8 * g + 5]);
            pb.w = pack_bf16x2(s[u][8 * g + 6], s[u][8 * g + 7]);
            const u32x4_t va = *reinterpret_cast<const u32x4_t*>(Vs + l31 * VROW + ((u * 32 + 16 * g) + hi * 8) * 2);
            o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, va), __builtin_bit_cast(bf16x8_t, pb), o, 0, 0, 0);
          }
      } else {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = u * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            const float va = *reinterpret_cast<const float*>(Vs + key * VROW + l31 * 4);
            o = __builtin_amdgcn_mfma_f32_32x32x2f32(va, s[u][r], o, 0, 0, 0);
          }
      }
    }
    __syncthreads();
    if (more) lstore();
    __syncthreads();
  }

  // ---- merge the key parts: waves of parts 1..NS-1 publish (m, l, O) per lane, waves 0,1 combine in part order and store
  float l_tot = l_run + __shfl_xor(l_run, 32);   // both lane halves of a query share m_run
  float* mb = reinterpret_cast<float*>(smem);    // [NS-1 parts][2 waves][18][64 lanes]
  if (half >= 1) {
    float* dst = mb + ((half - 1) * 2 + (wv & 1)) * 18 * 64 + lane;
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[r * 64] = o[r];
    dst[16 * 64] = m_run;
    dst[17 * 64] = l_tot;
  }
  __syncthreads();
  if (half == 0 && q_ok) {
    float m = m_run;
#pragma unroll
    for (int p = 1; p < NS; ++p) m = fmaxf(m, mb[((p - 1) * 2 + (wv & 1)) * 18 * 64 + lane + 16 * 64]);
    const float mu = (m == -INFINITY) ? 0.f : m;
    float ap[NS];                                  // a part that saw no key has m = -inf -> weight 0
    ap[0] = atb_exp_diff(m_run, mu);
    float den = l_tot * ap[0];
#pragma unroll
    for (int p = 1; p < NS; ++p) {
      const float* src = mb + ((p - 1) * 2 + (wv & 1)) * 18 * 64 + lane;
      ap[p] = atb_exp_diff(src[16 * 64], mu);
      den += src[17 * 64] * ap[p];
    }
    const float inv = 1.f / den;                   // a row without any key: den = 0 and every element below is 0 * inf = NaN (torch: 0 / 0)
    const long off = b * a.bso + (long)q * a.ldo + head * ATB_D + 4 * hi;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      float acc[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = o[4 * qd + e] * ap[0];
#pragma unroll
      for (int p = 1; p < NS; ++p) {
        const float* src = mb + ((p - 1) * 2 + (wv & 1)) * 18 * 64 + lane;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += src[(4 * qd + e) * 64] * ap[p];
      }
      const float4 r = make_float4(acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);
      if (a.out_dt == FAR3D_DT_F32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.out) + off + 8 * qd) = r;
      else *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(a.out) + off + 8 * qd) = make_uint2(pack_bf16x2(r.x, r.y), pack_bf16x2(r.z, r.w));
    }
  }
}

extern "C" int far3d_attention_batched(const void* q, const void* k, const void* v, int dtype, void* out, int out_dt, int B, int Aq, int Nk,
                                       int heads, int head_dim, int ldq, int ldk, int ldv, int ldo, long bsq, long bsk, long bsv, long bso,
                                       float scale, const void* attn_mask, int mask_kind, int ldm, long mask_bstride,
                                       const uint8_t* key_padding, void* stream) {
  const char* who = "far3d_attention_batched";
  FAR3D_CHECK_ARG(q && k && v && out, "%s: null pointer argument", who);
  FAR3D_CHECK_ARG(head_dim == ATB_D, "%s: head_dim must be %d (got %d)", who, ATB_D, head_dim);
  FAR3D_CHECK_ARG(B >= 1 && Aq >= 1 && Nk >= 1 && heads >= 1, "%s: bad sizes B=%d Aq=%d Nk=%d heads=%d", who, B, Aq, Nk, heads);
  FAR3D_CHECK_ARG(B <= 65535 && heads <= 65535, "%s: B=%d / heads=%d above the grid limit 65535", who, B, heads);
  FAR3D_CHECK_ARG(dtype == FAR3D_DT_F32 || dtype == FAR3D_DT_BF16, "%s: unsupported dtype %d", who, dtype);
  FAR3D_CHECK_ARG(out_dt == FAR3D_DT_F32 || out_dt == FAR3D_DT_BF16, "%s: unsupported output dtype %d", who, out_dt);
  FAR3D_CHECK_ARG(mask_kind == FAR3D_MASK_NONE || mask_kind == FAR3D_MASK_BYTES || mask_kind == FAR3D_MASK_F32,
                  "%s: unknown mask_kind %d (0 none, 1 bytes, 2 f32 additive)", who, mask_kind);
  if (mask_kind != FAR3D_MASK_NONE) {
    FAR3D_CHECK_ARG(attn_mask, "%s: mask_kind %d without an attn_mask pointer", who, mask_kind);
    FAR3D_CHECK_ARG(ldm >= Nk, "%s: mask row stride ldm=%d below Nk=%d", who, ldm, Nk);
    FAR3D_CHECK_ARG(mask_bstride >= 0, "%s: negative mask batch stride", who);
    FAR3D_CHECK_ARG(mask_kind != FAR3D_MASK_F32 || (uintptr_t)attn_mask % 4 == 0, "%s: f32 mask pointer not 4-byte aligned", who);
  }
  const int es = dtype == FAR3D_DT_F32 ? 4 : 2;
  FAR3D_CHECK_ARG(ldq >= heads * ATB_D && ldk >= heads * ATB_D && ldv >= heads * ATB_D && ldo >= heads * ATB_D,
                  "%s: a row stride is below heads * 32 = %d", who, heads * ATB_D);
  FAR3D_CHECK_ARG(bsq >= 0 && bsk >= 0 && bsv >= 0 && bso >= 0, "%s: negative batch stride", who);
  FAR3D_CHECK_ARG(((uintptr_t)q % 16 == 0) && ((uintptr_t)k % 16 == 0) && ((uintptr_t)v % 16 == 0) && ((uintptr_t)out % 16 == 0) &&
                  (ldq * es) % 16 == 0 && (ldk * es) % 16 == 0 && (ldv * es) % 16 == 0 && ldo % 4 == 0 &&
                  (bsq * es) % 16 == 0 && (bsk * es) % 16 == 0 && (bsv * es) % 16 == 0 && bso % 4 == 0,
                  "%s: pointers / row strides / batch strides must be 16-byte aligned", who);
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
