// Building blocks of the proposal kernels: frontend.hip (far3d_proposal_gather / far3d_proposal_gather_md: prop_gather_kernel,
// far3d_proposal_extra_rows: prop_extra_kernel) and foreign.hip (far3d_proposal_from_boxes: prop_from_boxes_kernel).  Each piece exists
// once, here; the rows and records of the three kernels agree bit for bit because they are made of the same text.
//
// The pieces with a loop or a branch inside are function-like macros with every name passed in, as in attn_core.hpp and for its reason:
// behind a __forceinline__ call each of them gave the kernels another instruction order or register allocation, as a macro they keep
// the machine code the written-out copies had (profiles/prop_host/README.md).  The wave arg-max and the score's log-odds are functions.
#pragma once
#include "common.hpp"

// LID depth bins and the point-cloud range every reference point is normalised by.  GatherParams, FromBoxParams and ExtraParams embed
// it where these eight floats stood.
struct PropGeom { float depth_min, bin_size, pc_lo[3], pc_span[3]; };

static inline void prop_fill_geom(PropGeom& q, float depth_min, float depth_max, int depth_bins, const float* pc_range) {
  q.depth_min = depth_min;
  q.bin_size = 2.f * (depth_max - depth_min) / ((float)depth_bins * (1.f + depth_bins));
  for (int k = 0; k < 3; ++k) { q.pc_lo[k] = pc_range[k]; q.pc_span[k] = pc_range[3 + k] - pc_range[k]; }
}

// log-odds of the score threshold: what the context rows' last column is measured against
static inline float prop_thr_logodds(float score_thr) { return logf(score_thr / (1.f - score_thr)); }

// Depth bin -> normalised reference point (ref farhead.py:748-753): LID un-binning, the pixel centre (bcx, bcy) scaled by the clamped
// depth, the three rows of the camera's img2lidar `m`, the normalisation by the point-cloud range `geo` (a PropGeom).  The point goes to
// out[off + 0 .. 2], registers or memory.
#define PROP_BIN_TO_REF(geo, m, bin, bcx, bcy, out, off)                                              \
  {                                                                                                   \
    const float q_ = (float)(bin) / 0.5f + 1.f;                                                       \
    const float d_ = (geo).depth_min + (geo).bin_size / 8.f * (q_ * q_ - 1.f);                        \
    const float dm_ = fmaxf(d_, 1e-5f);                                                               \
    const float px_ = (bcx) * dm_, py_ = (bcy) * dm_;                                                 \
    const float* m_ = (m);                                                                            \
    _Pragma("unroll") for (int k_ = 0; k_ < 3; ++k_) {                                                \
      const float w_ = m_[4 * k_] * px_ + m_[4 * k_ + 1] * py_ + m_[4 * k_ + 2] * d_ + m_[4 * k_ + 3]; \
      (out)[(off) + k_] = (w_ - (geo).pc_lo[k_]) / (geo).pc_span[k_];                                 \
    }                                                                                                 \
  }

#define PROP_SLOTS 4                          // depth bins per lane: nd <= 256
// Wave arg-max over the lanes' (value, bin) pairs: value descending, lower bin first on ties.  Exact compares only, so every lane
// ends with the same pair.
__device__ __forceinline__ void prop_wave_argmax(float& v, int& i) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

// The K best of a cell's nd depth values (K <= 8, wave-uniform), ranked by value; the top-1 is the first maximum, like argmax.  Bins are
// spread over the lanes (bin = lane + 64 * slot, bin b at dl[b * stride]).  The caller declares float lv[PROP_SLOTS] (the lane's values,
// kept for the record), int bins[8] and float lk[8] (the ranking, the same in every lane).
#define PROP_TOPK_BINS(dl, stride, nd, K, lane, lv, bins, lk)                                         \
  {                                                                                                   \
    _Pragma("unroll") for (int q_ = 0; q_ < PROP_SLOTS; ++q_) {                                       \
      const int b_ = (lane) + 64 * q_;                                                                \
      (lv)[q_] = b_ < (nd) ? (dl)[(long)b_ * (stride)] : -INFINITY;                                   \
    }                                                                                                 \
    unsigned taken_ = 0u;                                                                             \
    _Pragma("unroll") for (int k_ = 0; k_ < 8; ++k_) {                                                \
      if (k_ < (K)) { /* wave-uniform */                                                              \
        float v_ = -INFINITY; int i_ = 0x7fffffff;                                                    \
        _Pragma("unroll") for (int q_ = 0; q_ < PROP_SLOTS; ++q_) {                                   \
          const int b_ = (lane) + 64 * q_;                                                            \
          if (b_ < (nd) && !(taken_ & (1u << q_)) && ((lv)[q_] > v_ || i_ == 0x7fffffff)) { v_ = (lv)[q_]; i_ = b_; } \
        }                                                                                             \
        prop_wave_argmax(v_, i_);                                                                     \
        if ((i_ & 63) == (lane)) taken_ |= 1u << (i_ >> 6);                                           \
        (bins)[k_] = i_; (lk)[k_] = v_;                                                               \
      }                                                                                               \
    }                                                                                                 \
  }

// Multi-depth record of primary `row` of camera n (ref farhead.py:754-805), written by lane 0: camera, the top-K bins, the ratios
// p_k / p_0 that scale the extra rows' log-odds, and the valid flag (top-1 bin >= the bin of range_min).  is_prob: the values are
// probabilities already; otherwise logits, p_k = e_k / s in fp32 with e_k = exp(l_k - max) and s summed slot by slot, then over the
// wave, lane 0's sum broadcast (softmax is monotone, so the ranking is the logits').  g has nd, md_k, md_min_bin, md_flags, md_info.
#define PROP_MD_RECORD(g, lv, bins, lk, lane, n, row, is_prob)                                        \
  {                                                                                                   \
    float s_ = 1.f;                                                                                   \
    if (!(is_prob)) {                                                                                 \
      float e_ = 0.f;                                                                                 \
      _Pragma("unroll") for (int q_ = 0; q_ < PROP_SLOTS; ++q_)                                       \
        if ((lane) + 64 * q_ < (g).nd) e_ += expf((lv)[q_] - (lk)[0]);                                \
      _Pragma("unroll") for (int o_ = 32; o_ >= 1; o_ >>= 1) e_ += __shfl_down(e_, o_);               \
      s_ = __shfl(e_, 0);                                                                             \
    }                                                                                                 \
    if ((lane) == 0) {                                                                                \
      const float p0_ = (is_prob) ? (lk)[0] : expf((lk)[0] - (lk)[0]) / s_;                           \
      int* info_ = (g).md_info + (long)(row) * 2 * (g).md_k;                                          \
      info_[0] = (n);                                                                                 \
      _Pragma("unroll") for (int k_ = 0; k_ < 8; ++k_) {                                              \
        if (k_ < (g).md_k) {                                                                          \
          info_[1 + k_] = (bins)[k_];                                                                 \
          if (k_ > 0) info_[(g).md_k + k_] = __float_as_int(((is_prob) ? (lk)[k_] : expf((lk)[k_] - (lk)[0]) / s_) / p0_); \
        }                                                                                             \
      }                                                                                               \
      (g).md_flags[row] = (bins)[0] >= (g).md_min_bin ? 1 : 0;                                        \
    }                                                                                                 \
  }

// log-odds of a proposal's score.  Static top-K mode can pad a camera with zero-weight (non-peak) cells: clamp so their log-odds stay
// finite (a peak that passed the reference's `> score_thr` test is never below 1e-6, so threshold mode is unchanged)
__device__ __forceinline__ float prop_score_logodds(float sc) {
  const float scc = fmaxf(sc, 1e-6f);
  return logf(scc / (1.f - scc));
}

// The row of a hole (a slot of the fixed-capacity buffers without a proposal): zeros, so that everything computed from it downstream
// stays finite (holes are masked as attention keys, not removed).  One wave per row; g has ref2d, box2d, score, ctx, C.  A macro, like
// PROP_CTX_COPY below and for its reason.
#define PROP_ZERO_ROW(g, row, lane)                                                                   \
  {                                                                                                   \
    if ((lane) < 3) (g).ref2d[(row) * 3 + (lane)] = 0.f;                                              \
    if ((lane) < 4) (g).box2d[(row) * 4 + (lane)] = 0.f;                                              \
    if ((lane) == 0) (g).score[row] = 0.f;                                                            \
    for (int c_ = (lane); c_ <= (g).C; c_ += 64) (g).ctx[(long)(row) * ((g).C + 1) + c_] = 0.f;       \
  }

// The C token features at feat[tok ...] (f32 | bf16) -> the context row at ctx[off ...], one element per lane and step (context rows
// are C + 1 floats: dword-aligned only).  A macro: behind a call the gather kernel's loop came out in another instruction order.
#define PROP_CTX_COPY(feat, feat_dt, tok, ctx, off, C, lane)                                          \
  for (int c_ = (lane); c_ < (C); c_ += 64) {                                                         \
    float fv_;                                                                                        \
    if ((feat_dt) == FAR3D_DT_F32) fv_ = reinterpret_cast<const float*>(feat)[(tok) + c_];            \
    else fv_ = bf16_to_f32(reinterpret_cast<const bf16_t*>(feat)[(tok) + c_]);                        \
    (ctx)[(off) + c_] = fv_;                                                                          \
  }
