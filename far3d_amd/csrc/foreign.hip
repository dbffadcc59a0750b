// Adaptive queries from a FOREIGN 2D head (any detector that hands over the reference's public dict: a boolean token mask, a list
// of boxes, scores and a depth map; ref models/dense_heads/farhead.py:571-610, 711-827):
//   far3d_mask_compact         ordered stream compaction of a (N,S) byte mask -> sel_idx / sel_cnt, the form the proposal kernels of
//                              frontend.hip consume -- replaces the boolean-mask indexing feat_flatten[valid_indices] (:578-579).
//   far3d_proposal_from_boxes  the counterpart of far3d_proposal_gather / far3d_proposal_gather_md that READS the box instead of
//                              decoding it from the regression maps: depth cell, best bin(s), LID un-binning, un-projection,
//                              context row; with topk > 1 the per-primary records far3d_proposal_extra_rows consumes.
// The arithmetic after the box is the building blocks of prop_core.hpp, the ones prop_gather_kernel / md_topk_record (frontend.hip) use:
// fed with that kernel's own boxes, scores and selection, the rows and records are the same bit for bit (tests/test_foreign_props_gpu.py).
#include "common.hpp"
#include "prop_core.hpp"

// ------------------------------------------------------------------------------------------ ordered mask compaction
#define COMPACT_THREADS 1024
#define COMPACT_WAVES (COMPACT_THREADS / 64)

// One workgroup per camera.  The camera's S mask bytes are read as 16-byte words (one per thread and chunk; a chunk = 16384 tokens)
// laid on the 16-byte grid of the ADDRESS -- a row may start anywhere (S is arbitrary) -- so the first and the last word of a row can
// hang over its ends: those two are read byte by byte, inside the row only.  Per chunk: 16-bit mask per thread, popcount, wave
// inclusive scan (shuffles), the 16 wave totals through LDS (double buffered: one barrier per chunk), running base across chunks.
// Every index is written by exactly one thread at a position that depends on the mask alone: no atomics, no order between workgroups.
__global__ __launch_bounds__(COMPACT_THREADS) void mask_compact_kernel(const uint8_t* __restrict__ valid, int* __restrict__ sel_idx,
                                                                       int* __restrict__ sel_cnt, int* __restrict__ overflow_out,
                                                                       int S, int cap) {
  const int n = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint8_t* row = valid + (long)n * S;
  const int lead = (int)(reinterpret_cast<uintptr_t>(row) & 15);      // bytes between the 16-byte grid and the row's first token
  const long nwords = ((long)lead + S + 15) >> 4;
  __shared__ int s_tot[2][COMPACT_WAVES];
  long base = 0;
  int par = 0;
  for (long w0 = 0; w0 < nwords; w0 += COMPACT_THREADS, par ^= 1) {
    const long w = w0 + t;
    const long tok0 = w * 16 - lead;                                   // token of the word's first byte (negative: before the row)
    unsigned m = 0u;
    if (w < nwords) {
      if (tok0 >= 0 && tok0 + 16 <= S) {
        const uint4 q = *reinterpret_cast<const uint4*>(row + tok0);
        const unsigned d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int b = 0; b < 4; ++b) m |= ((d[k] >> (8 * b)) & 0xffu) ? (1u << (4 * k + b)) : 0u;
      } else {
        for (int b = 0; b < 16; ++b) {
          const long i = tok0 + b;
          if (i >= 0 && i < S && row[i]) m |= 1u << b;
        }
      }
    }
    const int c = __popc(m);
    int inc = c;                                                       // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(inc, o);
      if (lane >= o) inc += up;
    }
    if (lane == 63) s_tot[par][wv] = inc;
    __syncthreads();
    int wave_off = 0, chunk = 0;
#pragma unroll
    for (int q = 0; q < COMPACT_WAVES; ++q) { wave_off += q < wv ? s_tot[par][q] : 0; chunk += s_tot[par][q]; }
    long pos = base + wave_off + (inc - c);
    while (m && pos < cap) {
      const int b = __ffs(m) - 1;
      m &= m - 1u;
      sel_idx[(long)n * cap + pos] = (int)(tok0 + b);
      ++pos;
    }
    base += chunk;
  }
  if (t == 0) {
    sel_cnt[n] = (int)(base < cap ? base : cap);
    if (overflow_out && base > cap) *overflow_out = 1;               // zeroed on the stream before the launch; every writer stores 1
  }
}

extern "C" int far3d_mask_compact(const uint8_t* valid, int N, int S, int* sel_idx, int* sel_cnt, int cap, int32_t* overflow_out,
                                  void* stream) {
  FAR3D_CHECK_ARG(valid && sel_idx && sel_cnt, "far3d_mask_compact: null argument");
  FAR3D_CHECK_ARG(N >= 1 && S >= 1 && cap >= 1, "far3d_mask_compact: need N >= 1, S >= 1, cap >= 1 (got N=%d S=%d cap=%d)", N, S, cap);
  FAR3D_CHECK_ARG((long)N * cap <= 0x7fffffffL, "far3d_mask_compact: N * cap = %ld entries do not fit an int32 index", (long)N * cap);
  hipStream_t st = (hipStream_t)stream;
  if (overflow_out) {
    if (hipMemsetAsync(overflow_out, 0, sizeof(int32_t), st) != hipSuccess) {
      far3d_set_error("far3d_mask_compact: clearing the overflow flag failed");
      return FAR3D_ERR_LAUNCH;
    }
  }
  hipLaunchKernelGGL(mask_compact_kernel, dim3(N), dim3(COMPACT_THREADS), 0, st, valid, sel_idx, sel_cnt, (int*)overflow_out, S, cap);
  FAR3D_CHECK_LAUNCH("far3d_mask_compact");
  return FAR3D_OK;
}

// ------------------------------------------------------------------------------------------ rows from given boxes
struct FromBoxParams {
  const float* boxes; const int* box_cnt; const float* scores;        // (rows,4) cxcywh camera-major, (N), (rows)
  const int* sel_idx; const int* sel_cnt;                             // (N,cap), (N)
  const float* depth; long d_img, d_cell, d_bin;                      // depth map: element strides of a camera, a cell and a bin
  const float* img2lidar;                                             // (N,4,4)
  const void* feat; int feat_dt, feat_vec;                            // (N,S,C) token maps; feat_vec: 16-byte reads are possible
  float* ref2d; float* ctx;                                           // (rows,3), (rows,C+1)
  int N, S, cap, C, hd, wd, nd, ds, rows, is_prob;
  PropGeom geo; float thr_logodds;
  int md_k, md_min_bin;
  int* md_flags; int* md_info;                                        // (rows), (rows, 2K): the layout of far3d_proposal_gather_md
  int* mismatch_out;
};

// One wave per (box slot j, camera n).  The j-th box of camera n pairs with token sel_idx[n,j]; its row (input box / score and output)
// is j + the boxes of the cameras before n.
__global__ __launch_bounds__(64) void prop_from_boxes_kernel(FromBoxParams g) {
  const int n = blockIdx.y, j = blockIdx.x, lane = threadIdx.x;
  if (n == 0 && j == 0 && lane == 0 && g.mismatch_out) {
    int bad = 0;
    for (int k = 0; k < g.N; ++k) bad |= g.box_cnt[k] != g.sel_cnt[k];
    *g.mismatch_out = bad;
  }
  const int cnt = min(min(g.box_cnt[n], g.sel_cnt[n]), g.cap);
  if (j >= cnt) return;
  long rowl = j;
  for (int k = 0; k < n; ++k) rowl += max(g.box_cnt[k], 0);
  if (rowl >= g.rows) return;                                          // counts that do not fit the buffers: the host refuses the frame
  const long row = rowl;
  const int s = min(max(g.sel_idx[(long)n * g.cap + j], 0), g.S - 1);
  const float bcx = g.boxes[row * 4 + 0], bcy = g.boxes[row * 4 + 1];
  const float sc = g.scores[row];
  // depth cell at round(centre / ds), clamped (farhead.py:736-747); torch.round = half-to-even = rintf
  int u = (int)rintf(bcx / g.ds), v = (int)rintf(bcy / g.ds);
  u = min(max(u, 0), g.wd - 1); v = min(max(v, 0), g.hd - 1);
  const float* dl = g.depth + (long)n * g.d_img + ((long)v * g.wd + u) * g.d_cell;
  // the K best bins (K = 1: the first maximum, like argmax)
  float lv[PROP_SLOTS], lk[8];
  int bins[8];
  PROP_TOPK_BINS(dl, g.d_bin, g.nd, g.md_k > 1 ? g.md_k : 1, lane, lv, bins, lk)
  if (g.md_k > 1) PROP_MD_RECORD(g, lv, bins, lk, lane, n, row, g.is_prob)
  float c3[3];
  PROP_BIN_TO_REF(g.geo, g.img2lidar + n * 16, bins[0], bcx, bcy, c3, 0)
  float* cr = g.ctx + (long)row * (g.C + 1);
  if (lane == 0) {
    g.ref2d[row * 3 + 0] = c3[0]; g.ref2d[row * 3 + 1] = c3[1]; g.ref2d[row * 3 + 2] = c3[2];
    cr[g.C] = prop_score_logodds(sc) - g.thr_logodds;
  }
  // the token: 16-byte reads (the token rows are 16-byte aligned when C % 8 == 0); the context rows are C + 1 floats: dword stores
  const long tok = ((long)n * g.S + s) * g.C;
  if (g.feat_vec) {
    if (g.feat_dt == FAR3D_DT_F32) {
      const float4* src = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(g.feat) + tok);
      for (int c4 = lane; c4 < g.C / 4; c4 += 64) {
        const float4 x = src[c4];
        cr[4 * c4 + 0] = x.x; cr[4 * c4 + 1] = x.y; cr[4 * c4 + 2] = x.z; cr[4 * c4 + 3] = x.w;
      }
    } else {
      const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(g.feat) + tok);
      for (int c8 = lane; c8 < g.C / 8; c8 += 64) {
        const uint4 x = src[c8];
        const unsigned d4[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          cr[8 * c8 + 2 * k + 0] = __uint_as_float(d4[k] << 16);
          cr[8 * c8 + 2 * k + 1] = __uint_as_float(d4[k] & 0xffff0000u);
        }
      }
    }
  } else {
    PROP_CTX_COPY(g.feat, g.feat_dt, tok, cr, 0, g.C, lane)
  }
}

extern "C" int far3d_proposal_from_boxes(const float* boxes, const int* box_cnt, const float* scores, int rows, const int* sel_idx,
                                         const int* sel_cnt, int cap, int N, int S, const float* depth, int depth_layout,
                                         int depth_is_prob, int hd, int wd, int nd, int depth_stride, float depth_min, float depth_max,
                                         int depth_bins, const float* img2lidar, const void* feat, int feat_dt, int C,
                                         const float* pc_range, float score_thr, float* ref2d, float* ctx, int topk, int range_min_bin,
                                         int32_t* md_flags, int32_t* md_info, int32_t* mismatch_out, void* stream) {
  FAR3D_CHECK_ARG(boxes && box_cnt && scores && sel_idx && sel_cnt && depth && img2lidar && feat && pc_range && ref2d && ctx,
                  "far3d_proposal_from_boxes: null argument");
  FAR3D_CHECK_ARG(N >= 1 && S >= 1 && cap >= 1 && rows >= 1 && C >= 1 && hd >= 1 && wd >= 1 && depth_stride >= 1 && depth_bins >= 1,
                  "far3d_proposal_from_boxes: bad sizes");
  FAR3D_CHECK_ARG(nd >= 1 && nd <= 64 * PROP_SLOTS, "far3d_proposal_from_boxes: depth bins nd=%d (1 ... %d)", nd, 64 * PROP_SLOTS);
  FAR3D_CHECK_ARG(depth_layout == 0 || depth_layout == 1, "far3d_proposal_from_boxes: depth_layout 0 (N,hd,wd,nd) or 1 (N,nd,hd,wd)");
  FAR3D_CHECK_ARG(feat_dt == FAR3D_DT_F32 || feat_dt == FAR3D_DT_BF16, "far3d_proposal_from_boxes: tokens must be f32 or bf16");
  FAR3D_CHECK_ARG(topk == 1 || (topk >= 2 && topk <= 8 && topk <= nd && md_flags && md_info),
                  "far3d_proposal_from_boxes: topk 1, or 2 ... 8 (<= depth bins) with md_flags and md_info");
  FAR3D_CHECK_ARG(N <= 65535, "far3d_proposal_from_boxes: at most 65535 cameras (one grid row each)");
  FromBoxParams g;
  memset(&g, 0, sizeof(g));
  g.boxes = boxes; g.box_cnt = box_cnt; g.scores = scores; g.sel_idx = sel_idx; g.sel_cnt = sel_cnt;
  g.depth = depth;
  g.d_img = (long)hd * wd * nd;
  g.d_cell = depth_layout == 0 ? nd : 1;
  g.d_bin = depth_layout == 0 ? 1 : (long)hd * wd;
  g.img2lidar = img2lidar; g.feat = feat; g.feat_dt = feat_dt;
  g.feat_vec = (C % 8 == 0 && (reinterpret_cast<uintptr_t>(feat) & 15) == 0) ? 1 : 0;
  g.ref2d = ref2d; g.ctx = ctx;
  g.N = N; g.S = S; g.cap = cap; g.C = C; g.hd = hd; g.wd = wd; g.nd = nd; g.ds = depth_stride; g.rows = rows;
  g.is_prob = depth_is_prob ? 1 : 0;
  prop_fill_geom(g.geo, depth_min, depth_max, depth_bins, pc_range);
  g.thr_logodds = prop_thr_logodds(score_thr);
  g.md_k = topk; g.md_min_bin = range_min_bin; g.md_flags = md_flags; g.md_info = md_info;
  g.mismatch_out = mismatch_out;
  hipLaunchKernelGGL(prop_from_boxes_kernel, dim3(cap, N), dim3(64), 0, (hipStream_t)stream, g);
  FAR3D_CHECK_LAUNCH("far3d_proposal_from_boxes");
  return FAR3D_OK;
}
