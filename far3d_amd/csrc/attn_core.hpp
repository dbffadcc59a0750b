// Building blocks of the attention kernels: attn.hip (far3d_attention_forward / far3d_attention_streams: the staged attn_fwd_kernel and
// the register-fed attn_f32_direct_kernel) and attn_batch.hip (far3d_attention_batched: attn_batch_kernel).  Each piece exists once,
// here; the kernels are compositions of them around their own online-softmax step, which defines their output bits and stays theirs.
//
// Shared layout (head_dim 32, tiles of 64 keys).  Scores are computed TRANSPOSED, S^T = K Q^T, so the MFMA C layout puts one query per
// lane column: lane (q = lane & 31, hi = lane >> 5) holds 16 of the 32 keys of a sub-tile for ITS query -- register r is key
// (r & 3) + 8 (r >> 2) + 4 hi -- and the partner lane q + 32 the other 16.  O^T = V^T P^T accumulates with the same column = query
// mapping.  A workgroup splits the keys into NS parts (flash-decoding style); the partial (max, sum, O) states meet in an LDS merge
// buffer of 18 x 64 floats per (part >= 1, wave of part 0) slot and are combined in part order.
// T = bf16: v_mfma_f32_32x32x16_bf16.  T = float: exact-fp32 v_mfma_f32_32x32x2_f32 (parity mode).
#pragma once
#include "common.hpp"

typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 bf16x8_t;
typedef __attribute__((__vector_size__(16 * sizeof(float)))) float f32x16_t;
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

#define ATT_D 32
#define ATT_KT 64

// LDS tiles of one key part: K row-major with padded rows of KROW bytes; V transposed (bf16) or row-major (fp32), rows of VROW bytes.
// KSUB: 16-byte Q / K fragments per row; a thread stages 2 * CH 16-byte chunks of K (and as many of V) per iteration
template <typename T> struct AttCfg;
template <> struct AttCfg<bf16_t> { static constexpr int KROW = 80, VROW = 144, KSUB = 2, CH = 1, KBYTES = ATT_KT * KROW, VBYTES = ATT_D * VROW; };
template <> struct AttCfg<float> { static constexpr int KROW = 144, VROW = 144, KSUB = 4, CH = 2, KBYTES = ATT_KT * KROW, VBYTES = ATT_KT * VROW; };

template <typename T>
__device__ __forceinline__ void mma_att(f32x16_t& acc, const u32x4_t& a, const u32x4_t& b) {
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
__device__ __forceinline__ int vt_pos(int key) {
  const int quad = (key >> 2) & 3;
  const int sw = (quad == 1) ? 2 : ((quad == 2) ? 1 : quad);
  return (key & ~15) | (sw << 2) | (key & 3);
}

// The device pieces below are function-like macros, not functions, on purpose: the compiler optimises a __forceinline__ function on its
// own before it inlines it, and every piece behind a call gave the kernels another instruction order and register allocation
// (profiles/attn_core/README.md).  A macro hands the compiler the text it had when the piece was written out in each kernel, so the
// kernels keep the machine code they had.  Every name a macro reads or writes is an argument; T is the kernel's operand type.

// Q fragments (B operand: column = query) of the query whose head slice starts at `row`, held in registers for the whole key loop; a
// query at or beyond Aq (!q_ok) gets zeros.  fp32 only: pre-multiplied by `scale` (torch scales q before the product,
// F.multi_head_attention_forward); bf16 scales the scores.  Declares u32x4_t qf[KSUB].
#define ATT_LOAD_Q(T, qf, row, q_ok, hi, scale)                                                                     \
  u32x4_t qf[AttCfg<T>::KSUB];                                                                                      \
  _Pragma("unroll") for (int kk = 0; kk < AttCfg<T>::KSUB; ++kk) {                                                  \
    qf[kk] = u32x4_t{0u, 0u, 0u, 0u};                                                                               \
    if (q_ok) {                                                                                                     \
      constexpr int E = 16 / sizeof(T);                                                                             \
      const T* src = (row) + kk * 2 * E + hi * E;                                                                   \
      qf[kk] = *reinterpret_cast<const u32x4_t*>(src);                                                              \
      if constexpr (sizeof(T) == 4) {                                                                               \
        qf[kk].x = __float_as_uint(__uint_as_float(qf[kk].x) * scale);                                              \
        qf[kk].y = __float_as_uint(__uint_as_float(qf[kk].y) * scale);                                              \
        qf[kk].z = __float_as_uint(__uint_as_float(qf[kk].z) * scale);                                              \
        qf[kk].w = __float_as_uint(__uint_as_float(qf[kk].w) * scale);                                              \
      }                                                                                                             \
    }                                                                                                               \
  }

// Cooperative staging of NS K/V tiles per iteration (one per part) by the 128 * NS threads of a workgroup: chunk id -> (part, key, 16-B
// piece).  Declares the staging registers kreg / vreg and the pair gload(it) / lstore(): gload fetches tile `it` of every part into
// registers (zeros for keys at or beyond Nk and for tiles a part does not have), lstore writes them to the parts' LDS tiles: K rows as
// they are, V transposed with the key order permuted inside 16-key groups (bf16: the MFMA A-fragment of ATT_PV is ONE ds_read_b128) or
// row-major (fp32).  The callers double-buffer: gload(it + 1) before the MFMAs of tile `it`, lstore() between the two barriers after them.
#define ATT_STAGE(T, NS, gload, lstore, kreg, vreg, K, V, ldk, ldv, head, Nk, ntiles, htiles, t, KsAll, VsAll)      \
  u32x4_t kreg[2 * AttCfg<T>::CH], vreg[2 * AttCfg<T>::CH];                                                         \
  auto gload = [&](int it) __attribute__((always_inline)) {                                                         \
    constexpr int CPK = ATT_D * sizeof(T) / 16, E = 16 / sizeof(T); /* 16-B chunks per key row: 4 (bf16) / 8 (f32) */ \
    _Pragma("unroll") for (int c = 0; c < 2 * AttCfg<T>::CH; ++c) {                                                 \
      const int id = t + c * (128 * NS), h = id / (ATT_KT * CPK), rem = id % (ATT_KT * CPK), key = rem / CPK, ck = rem % CPK; \
      const int tl = it + h * htiles;                                                                               \
      const int gk = tl * ATT_KT + key;                                                                             \
      kreg[c] = u32x4_t{0u, 0u, 0u, 0u};                                                                            \
      vreg[c] = u32x4_t{0u, 0u, 0u, 0u};                                                                            \
      if (tl < ntiles && gk < Nk) {                                                                                 \
        kreg[c] = *reinterpret_cast<const u32x4_t*>(K + (long)gk * ldk + head * ATT_D + ck * E);                    \
        vreg[c] = *reinterpret_cast<const u32x4_t*>(V + (long)gk * ldv + head * ATT_D + ck * E);                    \
      }                                                                                                             \
    }                                                                                                               \
  };                                                                                                                \
  auto lstore = [&]() __attribute__((always_inline)) {                                                              \
    constexpr int CPK = ATT_D * sizeof(T) / 16, KROW = AttCfg<T>::KROW, VROW = AttCfg<T>::VROW;                     \
    _Pragma("unroll") for (int c = 0; c < 2 * AttCfg<T>::CH; ++c) {                                                 \
      const int id = t + c * (128 * NS), h = id / (ATT_KT * CPK), rem = id % (ATT_KT * CPK), key = rem / CPK, ck = rem % CPK; \
      *reinterpret_cast<u32x4_t*>(KsAll + h * AttCfg<T>::KBYTES + key * KROW + ck * 16) = kreg[c];                  \
      unsigned char* vs = VsAll + h * AttCfg<T>::VBYTES;                                                            \
      if constexpr (sizeof(T) == 2) {                                                                               \
        const int pos = vt_pos(key);                                                                                \
        const uint32_t w[4] = {vreg[c].x, vreg[c].y, vreg[c].z, vreg[c].w};                                         \
        _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                                             \
          const uint16_t val = (uint16_t)((e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu));                     \
          *reinterpret_cast<uint16_t*>(vs + (ck * 8 + e) * VROW + pos * 2) = val;                                   \
        }                                                                                                           \
      } else {                                                                                                      \
        *reinterpret_cast<u32x4_t*>(vs + key * VROW + ck * 16) = vreg[c];                                           \
      }                                                                                                             \
    }                                                                                                               \
  }

// S^T = K Q^T of one 64-key tile as two 32-key sub-tiles (Ks: the part's K tile in LDS).  Declares f32x16_t s[2].
#define ATT_SCORES(T, s, Ks, qf, l31, hi)                                                                           \
  f32x16_t s[2];                                                                                                    \
  _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                                                   \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) s[u][r] = 0.f;                                                   \
    _Pragma("unroll") for (int kk = 0; kk < AttCfg<T>::KSUB; ++kk) {                                                \
      const u32x4_t ka = *reinterpret_cast<const u32x4_t*>(Ks + (u * 32 + l31) * AttCfg<T>::KROW + kk * 32 + hi * 16); \
      mma_att<T>(s[u], ka, qf[kk]);                                                                                 \
    }                                                                                                               \
  }

// O^T += V^T P^T of one 64-key tile (Vs: the part's V tile in LDS; s: the probabilities in the S^T register order)
#define ATT_PV(T, o, s, Vs, l31, hi)                                                                                \
  if constexpr (sizeof(T) == 2) {                                                                                   \
    _Pragma("unroll") for (int u = 0; u < 2; ++u)                                                                   \
      _Pragma("unroll") for (int g = 0; g < 2; ++g) {                                                               \
        u32x4_t pb;                                                                                                 \
        pb.x = pack_bf16x2(s[u][8 * g + 0], s[u][8 * g + 1]);                                                       \
        pb.y = pack_bf16x2(s[u][8 * g + 2], s[u][8 * g + 3]);                                                       \
        pb.z = pack_bf16x2(s[u][8 * g + 4], s[u][8 * g + 5]);                                                       \
        pb.w = pack_bf16x2(s[u][8 * g + 6], s[u][8 * g + 7]);                                                       \
        const u32x4_t va = *reinterpret_cast<const u32x4_t*>(Vs + l31 * AttCfg<T>::VROW + ((u * 32 + 16 * g) + hi * 8) * 2); \
        o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, va), __builtin_bit_cast(bf16x8_t, pb), o, 0, 0, 0); \
      }                                                                                                             \
  } else {                                                                                                          \
    _Pragma("unroll") for (int u = 0; u < 2; ++u)                                                                   \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                              \
        const int key = u * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;                                                   \
        const float va = *reinterpret_cast<const float*>(Vs + key * AttCfg<T>::VROW + l31 * 4);                     \
        o = __builtin_amdgcn_mfma_f32_32x32x2f32(va, s[u][r], o, 0, 0, 0);                                          \
      }                                                                                                             \
  }

// Merge of the key parts, in two steps around the workgroup's ONE barrier (the register-fed kernel runs each step once per chain w).
// The merge buffer mb holds one slot of [18][64 lanes] floats -- 16 rows of O, m, l -- per (part >= 1, wave of part 0, chain); `slot`
// is the slot NUMBER, in step 2 an expression in p, the part.
#define ATT_SLOT (18 * 64)

// step 1, waves of parts 1..NS-1: publish (O, m, l) per lane
#define ATT_MERGE_PUBLISH(mb, slot, lane, o, m_run, l_tot)                                                          \
  {                                                                                                                 \
    float* dst = mb + (slot) * ATT_SLOT + lane;                                                                     \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) dst[r * 64] = o[r];                                              \
    dst[16 * 64] = m_run;                                                                                           \
    dst[17 * 64] = l_tot;                                                                                           \
  }

// step 2, waves of part 0, lanes with a query: combine in part order, normalise, store 4 x 4 outputs at (f32 | bf16*) O + off + 8 qd.
// EXPD(a, b) = e^(a - b) in the kernel's exponent form.  A part that saw no key has m = -inf -> weight 0; a row without any key has
// den = 0 and every element is 0 * inf = NaN (torch: 0 / 0).
#define ATT_EXPF_DIFF(a, b) expf((a) - (b))
#define ATT_MERGE_STORE(NS, mb, slot, lane, o, m_run, l_tot, EXPD, O, off_, out_dt)                                 \
  {                                                                                                                 \
    float m = m_run;                                                                                                \
    _Pragma("unroll") for (int p = 1; p < NS; ++p) m = fmaxf(m, mb[(slot) * ATT_SLOT + lane + 16 * 64]);            \
    const float mu = (m == -INFINITY) ? 0.f : m;                                                                    \
    float ap[NS];                                                                                                   \
    ap[0] = EXPD(m_run, mu);                                                                                        \
    float den = l_tot * ap[0];                                                                                      \
    _Pragma("unroll") for (int p = 1; p < NS; ++p) {                                                                \
      const float* src = mb + (slot) * ATT_SLOT + lane;                                                             \
      ap[p] = EXPD(src[16 * 64], mu);                                                                               \
      den += src[17 * 64] * ap[p];                                                                                  \
    }                                                                                                               \
    const float inv = 1.f / den;                                                                                    \
    const long off = off_;                                                                                          \
    _Pragma("unroll") for (int qd = 0; qd < 4; ++qd) {                                                              \
      float acc[4];                                                                                                 \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) acc[e] = o[4 * qd + e] * ap[0];                                 \
      _Pragma("unroll") for (int p = 1; p < NS; ++p) {                                                              \
        const float* src = mb + (slot) * ATT_SLOT + lane;                                                           \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) acc[e] += src[(4 * qd + e) * 64] * ap[p];                     \
      }                                                                                                             \
      const float4 r = make_float4(acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);                         \
      if (out_dt == FAR3D_DT_F32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(O) + off + 8 * qd) = r;       \
      else *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(O) + off + 8 * qd) = make_uint2(pack_bf16x2(r.x, r.y), pack_bf16x2(r.z, r.w)); \
    }                                                                                                               \
  }

// ---- host: the argument checks the three entry points share, in three steps because each entry has checks of its own between them (the
// grid limit, the key hole, the masks) and the order decides which message a call with two faults gets.  `who`: the entry's name.
// `batch`: the entry takes B samples with batch strides bs[4] (q, k, v, out; elements); the one-sample entry passes false, 1, NULL.

// pointers, head_dim, sizes
static inline int attn_check_operands(const char* who, const void* q, const void* k, const void* v, const void* out, int head_dim, bool batch,
                                      int B, int Aq, int Nk, int heads) {
  FAR3D_CHECK_ARG(q && k && v && out, "%s: null pointer argument", who);
  FAR3D_CHECK_ARG(head_dim == ATT_D, "%s: head_dim must be %d (got %d)", who, ATT_D, head_dim);
  if (batch) FAR3D_CHECK_ARG(B > 0 && Aq > 0 && Nk > 0 && heads > 0, "%s: bad sizes B=%d Aq=%d Nk=%d heads=%d", who, B, Aq, Nk, heads);
  else FAR3D_CHECK_ARG(Aq > 0 && Nk > 0 && heads > 0, "%s: bad sizes Aq=%d Nk=%d heads=%d", who, Aq, Nk, heads);
  return FAR3D_OK;
}

static inline int attn_check_dtype(const char* who, int dtype) {
  FAR3D_CHECK_ARG(dtype == FAR3D_DT_F32 || dtype == FAR3D_DT_BF16, "%s: unsupported dtype %d", who, dtype);
  return FAR3D_OK;
}

// batch strides not negative; pointers, row strides and batch strides 16-byte aligned (what the kernels' 16-byte loads and stores need)
static inline int attn_check_layout(const char* who, const void* q, const void* k, const void* v, const void* out, int dtype, int out_dt,
                                    int ldq, int ldk, int ldv, int ldo, const long* bs) {
  const int es = dtype == FAR3D_DT_F32 ? 4 : 2;
  const bool rows_ok = ((uintptr_t)q % 16 == 0) && ((uintptr_t)k % 16 == 0) && ((uintptr_t)v % 16 == 0) && ((uintptr_t)out % 16 == 0) &&
                       (ldq * es) % 16 == 0 && (ldk * es) % 16 == 0 && (ldv * es) % 16 == 0 && ldo % 4 == 0 &&
                       (out_dt == FAR3D_DT_F32 || out_dt == FAR3D_DT_BF16);
  if (!bs) {
    FAR3D_CHECK_ARG(rows_ok, "%s: pointers / row strides must be 16-byte aligned", who);
    return FAR3D_OK;
  }
  FAR3D_CHECK_ARG(bs[0] >= 0 && bs[1] >= 0 && bs[2] >= 0 && bs[3] >= 0, "%s: negative batch stride", who);
  FAR3D_CHECK_ARG(rows_ok && (bs[0] * es) % 16 == 0 && (bs[1] * es) % 16 == 0 && (bs[2] * es) % 16 == 0 && bs[3] % 4 == 0,
                  "%s: pointers / row strides / batch strides must be 16-byte aligned", who);
  return FAR3D_OK;
}
