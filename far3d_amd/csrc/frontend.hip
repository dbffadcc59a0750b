// Per-camera front-end glue kernels (HBM-bound, byte/index work -- no MFMA):
//   far3d_stem_im2col      NCHW fp32 image -> NHWC 32-channel im2col of the 3x3/s2 stem conv (27 taps + 5 zeros) so the
//                          first VoVNet conv (ref models/backbones/vovnet.py:306-311) runs as a K=32 1x1 implicit GEMM.
//   far3d_proposal_scores  sigma(obj)*sigma(max cls) and the 3x3 peak test of YOLOXHeadCustom.get_bboxes
//                          (ref models/dense_heads/yolox_head.py:426-438).
//   far3d_proposal_select  ordered, fixed-capacity selection (score > thr, or the K best per camera) -- replaces the
//                          boolean-mask indexing that forces host syncs in the reference (:435-458).
//   far3d_proposal_gather  2D box decode (:491-501), depth-bin lookup + LID un-binning, un-projection to normalised 3D
//                          reference points and the 257-wide context vector (ref models/dense_heads/farhead.py:571-610,
//                          710-827, 521-531).
#include "common.hpp"
#include "prop_core.hpp"

// ------------------------------------------------------------------------------------------ stem im2col
template <typename T>
__global__ __launch_bounds__(256) void stem_im2col_kernel(const float* __restrict__ img, T* __restrict__ out, int N, int H,
                                                          int W, int Ho, int Wo) {
  // one thread per output pixel: 9 taps x 3 channels gathered from the NCHW image, written as ONE 32-channel row
  // (27 values + 5 zero pad channels) with 16-byte stores
  const long total = (long)N * Ho * Wo;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    long p = i;
    const int ox = (int)(p % Wo); p /= Wo;
    const int oy = (int)(p % Ho);
    const int n = (int)(p / Ho);
    float v[32];
#pragma unroll
    for (int k = 27; k < 32; ++k) v[k] = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int iy = oy * 2 - 1 + tap / 3, ix = ox * 2 - 1 + tap % 3;
      const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[tap * 3 + c] = ok ? img[(((long)n * 3 + c) * H + iy) * W + ix] : 0.f;
    }
    if constexpr (ChanScale<T>::v == 2) {     // pair storage: 32 hi bf16 then 32 lo bf16 (one 128-byte row)
      uint2 h[8], l[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) split4f(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3], h[k], l[k]);
      uint4* dst = reinterpret_cast<uint4*>(out + i * 64);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        dst[k] = make_uint4(h[2 * k].x, h[2 * k].y, h[2 * k + 1].x, h[2 * k + 1].y);
        dst[4 + k] = make_uint4(l[2 * k].x, l[2 * k].y, l[2 * k + 1].x, l[2 * k + 1].y);
      }
      continue;
    }
    T* dst = out + i * 32;
    if constexpr (sizeof(T) == 4) {
#pragma unroll
      for (int k = 0; k < 8; ++k) reinterpret_cast<float4*>(dst)[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        reinterpret_cast<uint4*>(dst)[k] = make_uint4(pack_bf16x2(v[8 * k], v[8 * k + 1]), pack_bf16x2(v[8 * k + 2], v[8 * k + 3]),
                                                       pack_bf16x2(v[8 * k + 4], v[8 * k + 5]), pack_bf16x2(v[8 * k + 6], v[8 * k + 7]));
    }
  }
}

extern "C" int far3d_stem_im2col(const float* img, void* out, int out_dt, int N, int H, int W, void* stream) {
  FAR3D_CHECK_ARG(img && out && N > 0 && H > 0 && W > 0, "far3d_stem_im2col: bad arguments");
  FAR3D_CHECK_ARG(out_dt == FAR3D_DT_F32 || out_dt == FAR3D_DT_BF16 || out_dt == FAR3D_DT_BF16_PAIR, "far3d_stem_im2col: unsupported dtype");
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  const long total = (long)N * Ho * Wo;
  long blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipStream_t st = (hipStream_t)stream;
  if (out_dt == FAR3D_DT_F32)
    hipLaunchKernelGGL(stem_im2col_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, img, (float*)out, N, H, W, Ho, Wo);
  else if (out_dt == FAR3D_DT_BF16_PAIR)
    hipLaunchKernelGGL(stem_im2col_kernel<pair_t>, dim3((unsigned)blocks), dim3(256), 0, st, img, (pair_t*)out, N, H, W, Ho, Wo);
  else
    hipLaunchKernelGGL(stem_im2col_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, img, (bf16_t*)out, N, H, W, Ho, Wo);
  FAR3D_CHECK_LAUNCH("far3d_stem_im2col");
  return FAR3D_OK;
}

// ------------------------------------------------------------------------------------------ 2D proposal scores
#define PROP_MAX_L 4
struct PropLevels {
  int L, S;
  int H[PROP_MAX_L], W[PROP_MAX_L], start[PROP_MAX_L], stride[PROP_MAX_L];
  const float* cls[PROP_MAX_L];   // (N, h, w, ncls) f32
  const float* reg[PROP_MAX_L];   // (N, h, w, nreg>=5) f32: 4 box deltas + objectness
  int ncls, nreg;
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

__global__ __launch_bounds__(256) void prop_score_kernel(PropLevels lv, float* __restrict__ sw, int N) {
  const long total = (long)N * lv.S;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int n = (int)(i / lv.S), s = (int)(i - (long)n * lv.S);
    int l = 0;
#pragma unroll
    for (int k = 1; k < PROP_MAX_L; ++k) if (k < lv.L && s >= lv.start[k]) l = k;
    const long pix = (long)n * lv.H[l] * lv.W[l] + (s - lv.start[l]);
    const float* c = lv.cls[l] + pix * lv.ncls;
    float m = c[0];
    for (int k = 1; k < lv.ncls; ++k) m = fmaxf(m, c[k]);
    sw[i] = sigmoidf_(lv.reg[l][pix * lv.nreg + 4]) * sigmoidf_(m);
  }
}

__global__ __launch_bounds__(256) void prop_peak_kernel(PropLevels lv, const float* __restrict__ sw, float* __restrict__ wgt, int N) {
  const long total = (long)N * lv.S;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int n = (int)(i / lv.S), s = (int)(i - (long)n * lv.S);
    int l = 0;
#pragma unroll
    for (int k = 1; k < PROP_MAX_L; ++k) if (k < lv.L && s >= lv.start[k]) l = k;
    const int H = lv.H[l], W = lv.W[l], r = s - lv.start[l], y = r / W, x = r - y * W;
    const float* base = sw + (long)n * lv.S + lv.start[l];
    const float v = base[r];
    float m = v;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = y + dy, xx = x + dx;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) m = fmaxf(m, base[yy * W + xx]);
      }
    wgt[i] = (v == m) ? v : 0.f;   // sample_weight * (sample_weight == maxpool3x3(sample_weight))
  }
}

// One workgroup per camera.  mode 0: keep w > thr (count <= cap, extra entries dropped in index order);
// mode 1: keep the K (= cap) largest, ties resolved towards the lower index.  Output indices ascending.
__global__ __launch_bounds__(1024) void prop_select_kernel(const float* __restrict__ wgt, int* __restrict__ sel_idx,
                                                           int* __restrict__ sel_cnt, int S, int cap, float thr, int mode) {
  const int n = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
  const float* w = wgt + (long)n * S;
  __shared__ int s_cnt[1024 / 64];
  __shared__ int s_tot;
  __shared__ unsigned s_key;
  // --- mode 1: find the K-th largest value by bisection on the (monotone, w >= 0) float bit pattern.  The camera's S <= 16*nt
  // weights are read ONCE into registers; a pass = register compares + one wave reduction + ONE barrier (partials are double
  // buffered and every thread adds the 16 wave partials itself), 31 passes.
  unsigned kth = __float_as_uint(thr);   // mode 0: strict threshold
  int n_gt = 0;
  constexpr int MAXV = 16;
  unsigned v[MAXV];
  if (mode == 1) {
#pragma unroll
    for (int k = 0; k < MAXV; ++k) v[k] = __float_as_uint(w[min(t + k * nt, S - 1)]);        // clamped index: all loads in flight together
#pragma unroll
    for (int k = 0; k < MAXV; ++k) v[k] = (t + k * nt) < S ? v[k] : 0u;                        // padding 0 never counts (mid >= 1)
    __shared__ int s_part[2][1024 / 64];
    int pass = 0;
#define PROP_COUNT_GE(dst, keyv)                                           \
    {                                                                      \
      int c_ = 0;                        /* wave-uniform: ballot + s_bcnt1, no cross-lane shuffles */ \
      _Pragma("unroll") for (int k = 0; k < MAXV; ++k) c_ += __popcll(__ballot(v[k] >= (keyv))); \
      if ((t & 63) == 0) s_part[pass & 1][t >> 6] = c_;                    \
      __syncthreads();                                                     \
      int tot_ = 0;                                                        \
      for (int k = 0; k < nt / 64; ++k) tot_ += s_part[pass & 1][k];       \
      ++pass;                                                              \
      dst = tot_;                                                          \
    }
    // Round 5: the bisection stops at the first cut that keeps between K and PROP_WIN entries; those few are ranked by counting (value
    // descending, index ascending), the best K kept and put back into index order by a second count -- ~10 passes + 4 barriers instead
    // of 31 passes + 52 barriers of ordered compaction (40 -> us per frame, profiles/r5).  No such cut (fewer than K positive weights:
    // the K-th place is a tie among zeros, or a huge tie group): the loop runs to its end and the exact path below takes over.
    constexpr int PROP_WIN = 256;
    __shared__ __attribute__((aligned(16))) unsigned long long s_ent[PROP_WIN + 4];
    __shared__ int s_kidx[PROP_WIN];
    unsigned lo = 0u, hi = 0x7f800000u;   // invariant: count(w >= lo) >= K, count(w >= hi) < K
    bool window = false;
    while (hi - lo > 1u) {
      const unsigned mid = lo + ((hi - lo) >> 1);
      int c;
      PROP_COUNT_GE(c, mid);
      if (c >= cap && c <= PROP_WIN && cap <= PROP_WIN) { lo = mid; window = true; break; }     // block-uniform
      if (c == cap) { lo = mid; break; }     // `w >= mid` keeps exactly K: the cut need not be an element itself
      if (c > cap) lo = mid; else hi = mid;
    }
    if (window) {
      if (t == 0) s_tot = 0;
      __syncthreads();
#pragma unroll
      for (int k = 0; k < MAXV; ++k) {
        const int i = t + k * nt;
        if (i < S && v[k] >= lo) {
          const int pos = atomicAdd(&s_tot, 1);
          if (pos < PROP_WIN) s_ent[pos] = ((unsigned long long)v[k] << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
        }
      }
      __syncthreads();
      const int c = min(s_tot, PROP_WIN);
      if (t < 4) s_ent[c + t] = 0ull;
      __syncthreads();
      if (t < c) {
        const unsigned long long mine = s_ent[t];
        int r = 0;
#pragma unroll 8
        for (int j = 0; j < c; j += 4) {
          const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(s_ent + j), b = *reinterpret_cast<const ulonglong2*>(s_ent + j + 2);
          r += (a.x > mine ? 1 : 0) + (a.y > mine ? 1 : 0) + (b.x > mine ? 1 : 0) + (b.y > mine ? 1 : 0);
        }
        if (r < cap) s_kidx[r] = (int)(0xffffffffu - (unsigned)(mine & 0xffffffffull));     // the K best, in value order
      }
      __syncthreads();
      if (t < cap) {
        const int mine = s_kidx[t];
        int r = 0;
#pragma unroll 8
        for (int j = 0; j < cap; ++j) r += s_kidx[j] < mine ? 1 : 0;
        sel_idx[(long)n * cap + r] = mine;                                                   // ascending index order
      }
      if (t == 0) sel_cnt[n] = cap;
      return;
    }
    kth = lo;   // the K-th largest element, or a cut between the K-th and the (K+1)-th
    if (kth != 0xffffffffu) PROP_COUNT_GE(n_gt, kth + 1u);   // strictly greater
#undef PROP_COUNT_GE
    __syncthreads();
  }
  // --- ordered compaction, chunk by chunk (chunk = workgroup size)
  // mode 0 keeps w > thr.  mode 1 keeps w > kth first-come AND as many w == kth (in index order) as needed; its values are
  // already in registers (v[k] = chunk k), mode 0 reads each chunk once.
  int base = 0, eq_left = (mode == 1) ? cap - n_gt : 0;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int c0 = k * nt;
    if (c0 < S) {                       // block-uniform
      const int i = c0 + t;
      unsigned bits;
      if (mode == 1) bits = v[k]; else bits = i < S ? __float_as_uint(w[i]) : 0u;
      bool gt = i < S && ((mode == 0) ? (__uint_as_float(bits) > thr) : (bits > kth));
      bool eq = (mode == 1) && i < S && bits == kth;
      // rank of equal-valued entries inside this chunk (needed to cut ties in index order)
      const unsigned long long eqm = __ballot(eq);
      int eq_before = __popcll(eqm & ((1ull << (t & 63)) - 1ull));
      if ((t & 63) == 0) s_cnt[t >> 6] = __popcll(eqm);
      __syncthreads();
      int eq_wave_off = 0, eq_chunk = 0;
      for (int q = 0; q < nt / 64; ++q) { if (q < (t >> 6)) eq_wave_off += s_cnt[q]; eq_chunk += s_cnt[q]; }
      __syncthreads();
      const bool keep = gt || (eq && (eq_wave_off + eq_before) < eq_left);
      const unsigned long long km = __ballot(keep);
      const int k_before = __popcll(km & ((1ull << (t & 63)) - 1ull));
      if ((t & 63) == 0) s_cnt[t >> 6] = __popcll(km);
      __syncthreads();
      int wave_off = 0, chunk = 0;
      for (int q = 0; q < nt / 64; ++q) { if (q < (t >> 6)) wave_off += s_cnt[q]; chunk += s_cnt[q]; }
      const int pos = base + wave_off + k_before;
      if (keep && pos < cap) sel_idx[(long)n * cap + pos] = i;
      base += chunk;
      eq_left -= min(eq_left, eq_chunk);
      __syncthreads();
    }
  }
  if (t == 0) sel_cnt[n] = min(base, cap);
  (void)s_key;
}

struct GatherParams {
  PropLevels lv;
  const int* sel_idx; const int* sel_cnt;    // (N,cap), (N)
  const float* wgt;                           // (N,S) peak weights
  const float* depth_logit;                   // (N, hd, wd, nd) f32
  const float* img2lidar;                     // (N,4,4)
  const void* feat; int feat_dt;              // (N,S,C) token-major (post-MLN) value maps
  float* ref2d;                               // (Mcap,3) normalised reference points
  float* ctx;                                 // (Mcap, C+1) context: feature || log-odds
  float* box2d;                               // (Mcap,4) cx,cy,w,h (pixels)
  float* score;                               // (Mcap)
  int cap, C, hd, wd, nd, ds;
  PropGeom geo; float thr_logodds;
  int N, rows_total;                          // rows_total > 0: fixed-capacity mode (rows past it are dropped, unused ones zero-filled)
  int* m_out; int* overflow_out;              // optional: number of valid rows; 1 if a proposal was (or may have been) dropped
  // multi-depth variant only (prop_gather_kernel<true>): top-`md_k` depth bins per primary, records for far3d_proposal_extra_rows
  int md_k, md_min_bin;
  int* md_flags; int* md_info;                // (rows) valid flag; (rows, 2K): camera, K bins, K-1 ratios (f32 bits)
};

// MD = true: the multi-depth variant (far3d_proposal_gather_md).  The primary rows are the same arithmetic as MD = false -- the
// depth bin is the same first-maximum of the logits, found by PROP_TOPK_BINS' wave arg-max instead of a serial loop -- and every
// primary also leaves a record of its top-K bins for the extra-row launch: md_topk_record ranks the logits of primary `row`'s cell,
// writes the record and returns the top-1 bin.
template <typename P>
__device__ int md_topk_record(const P& g, const float* __restrict__ dl, int lane, int n, int row) {
  float lv[PROP_SLOTS], lk[8];
  int bins[8];
  PROP_TOPK_BINS(dl, 1, g.nd, g.md_k, lane, lv, bins, lk)
  PROP_MD_RECORD(g, lv, bins, lk, lane, n, row, false)
  return bins[0];
}

template <bool MD>
__global__ __launch_bounds__(64) void prop_gather_kernel(GatherParams g) {
  const int n = blockIdx.y, j = blockIdx.x, lane = threadIdx.x;
  if (!MD && n == g.N) {
    // fixed-capacity bookkeeping (one extra row of workgroups): total count, overflow flag, zero-fill of the unused rows so that
    // everything computed from them downstream stays finite (they are masked as attention keys, not removed)
    int M = 0, full = 0;
    for (int k = 0; k < g.N; ++k) { M += g.sel_cnt[k]; full |= g.sel_cnt[k] >= g.cap; }
    const int Mv = min(M, g.rows_total);
    if (j == 0 && lane == 0) {
      if (g.m_out) *g.m_out = Mv;
      if (g.overflow_out) *g.overflow_out = (M > g.rows_total || full) ? 1 : 0;
    }
    for (int row = Mv + j; row < g.rows_total; row += gridDim.x) PROP_ZERO_ROW(g, row, lane)
    return;
  }
  if (j >= g.sel_cnt[n]) return;
  const int s = g.sel_idx[(long)n * g.cap + j];
  int row = j;                                 // output row = exclusive prefix of sel_cnt over the cameras before n, + j
  for (int k = 0; k < n; ++k) row += g.sel_cnt[k];
  if (g.rows_total > 0 && row >= g.rows_total) return;      // over capacity: dropped, flagged through overflow_out
  const PropLevels& lv = g.lv;
  int l = 0;
#pragma unroll
  for (int k = 1; k < PROP_MAX_L; ++k) if (k < lv.L && s >= lv.start[k]) l = k;
  const int W = lv.W[l], r = s - lv.start[l], y = r / W, x = r - y * W;
  const float st = (float)lv.stride[l];
  const float* rp = lv.reg[l] + ((long)n * lv.H[l] * W + r) * lv.nreg;
  const float cx = rp[0] * st + x * st, cy = rp[1] * st + y * st;   // xys = pred * stride + prior
  const float bw = expf(rp[2]) * st, bh = expf(rp[3]) * st;
  const float tlx = cx - bw / 2, tly = cy - bh / 2, brx = cx + bw / 2, bry = cy + bh / 2;
  const float bcx = (tlx + brx) / 2, bcy = (tly + bry) / 2;          // xyxy -> cxcywh exactly as the reference chains them
  const float sc = g.wgt[(long)n * lv.S + s];
  // depth bin at round(centre / ds), clamped (farhead.py:736-747); torch.round = half-to-even = rintf
  int u = (int)rintf(bcx / g.ds), v = (int)rintf(bcy / g.ds);
  u = min(max(u, 0), g.wd - 1); v = min(max(v, 0), g.hd - 1);
  const float* dl = g.depth_logit + (((long)n * g.hd + v) * g.wd + u) * g.nd;
  int best = 0; float bv = dl[0];
  if constexpr (MD) {
    best = md_topk_record(g, dl, lane, n, row);
  } else {
    for (int k = 1; k < g.nd; ++k) if (dl[k] > bv) { bv = dl[k]; best = k; }   // first maximum, like argmax
  }
  float c3[3];
  PROP_BIN_TO_REF(g.geo, g.img2lidar + n * 16, best, bcx, bcy, c3, 0)
  if (lane == 0) {
    g.ref2d[row * 3 + 0] = c3[0]; g.ref2d[row * 3 + 1] = c3[1]; g.ref2d[row * 3 + 2] = c3[2];
    g.box2d[row * 4 + 0] = bcx; g.box2d[row * 4 + 1] = bcy; g.box2d[row * 4 + 2] = brx - tlx; g.box2d[row * 4 + 3] = bry - tly;
    g.score[row] = sc;
    g.ctx[(long)row * (g.C + 1) + g.C] = prop_score_logodds(sc) - g.thr_logodds;
  }
  PROP_CTX_COPY(g.feat, g.feat_dt, ((long)n * lv.S + s) * g.C, g.ctx, (long)row * (g.C + 1), g.C, lane)
}

static int fill_levels(PropLevels& lv, int L, const int32_t* hw, const int32_t* strides, const float* const* cls,
                       const float* const* reg, int ncls, int nreg) {
  lv.L = L; lv.ncls = ncls; lv.nreg = nreg;
  int acc = 0;
  for (int l = 0; l < PROP_MAX_L; ++l) {
    lv.H[l] = l < L ? hw[2 * l] : 1; lv.W[l] = l < L ? hw[2 * l + 1] : 1; lv.stride[l] = l < L ? strides[l] : 1;
    lv.start[l] = acc; lv.cls[l] = l < L ? cls[l] : nullptr; lv.reg[l] = l < L ? reg[l] : nullptr;
    if (l < L) acc += lv.H[l] * lv.W[l];
  }
  lv.S = acc;
  return acc;
}

// cls[l]: (N,h_l,w_l,ncls) f32; reg[l]: (N,h_l,w_l,nreg) f32 with channels (dx,dy,log w,log h,objectness).
// scratch_sw, weights: (N,S) f32.  mode 0 threshold / 1 top-K.  sel_idx (N,cap) i32, sel_cnt (N) i32.
extern "C" int far3d_proposal_select(const float* const* cls, const float* const* reg, int ncls, int nreg, int N, int L,
                                     const int32_t* level_hw, const int32_t* strides, float* scratch_sw, float* weights,
                                     int* sel_idx, int* sel_cnt, int cap, float thr, int mode, void* stream) {
  FAR3D_CHECK_ARG(cls && reg && level_hw && strides && scratch_sw && weights && sel_idx && sel_cnt, "far3d_proposal_select: null argument");
  FAR3D_CHECK_ARG(L >= 1 && L <= PROP_MAX_L && N > 0 && cap > 0 && nreg >= 5 && ncls >= 1, "far3d_proposal_select: bad sizes");
  PropLevels lv;
  const int S = fill_levels(lv, L, level_hw, strides, cls, reg, ncls, nreg);
  FAR3D_CHECK_ARG(mode == 0 || (mode == 1 && cap <= S), "far3d_proposal_select: bad mode / K > S");
  FAR3D_CHECK_ARG(S <= 16 * 1024, "far3d_proposal_select: a camera's S=%d cells are handled as 16 chunks of 1024 (S <= 16384)", S);
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)N * S;
  const unsigned blocks = (unsigned)((total + 255) / 256);
  hipLaunchKernelGGL(prop_score_kernel, dim3(blocks), dim3(256), 0, st, lv, scratch_sw, N);
  hipLaunchKernelGGL(prop_peak_kernel, dim3(blocks), dim3(256), 0, st, lv, scratch_sw, weights, N);
  hipLaunchKernelGGL(prop_select_kernel, dim3(N), dim3(1024), 0, st, weights, sel_idx, sel_cnt, S, cap, thr, mode);
  FAR3D_CHECK_LAUNCH("far3d_proposal_select");
  return FAR3D_OK;
}

// The part of GatherParams far3d_proposal_gather and far3d_proposal_gather_md share: level table, selection, depth map, tokens, outputs,
// depth bins and range, threshold log-odds.  rows: rows_total / primary_rows.  The caller has checked its arguments.
static void gather_fill(GatherParams& g, const float* const* reg, int nreg, int N, int L, const int32_t* level_hw, const int32_t* strides,
                        const int* sel_idx, const int* sel_cnt, int cap, const float* weights, const float* depth_logit, int hd, int wd,
                        int nd, int depth_stride, float depth_min, float depth_max, int depth_bins, const float* img2lidar,
                        const void* feat, int feat_dt, int C, const float* pc_range, float score_thr, float* ref2d, float* ctx,
                        float* box2d, float* score, int rows) {
  memset(&g, 0, sizeof(g));
  const float* none[PROP_MAX_L] = {nullptr, nullptr, nullptr, nullptr};
  fill_levels(g.lv, L, level_hw, strides, none, reg, 1, nreg);
  g.sel_idx = sel_idx; g.sel_cnt = sel_cnt; g.wgt = weights; g.depth_logit = depth_logit;
  g.img2lidar = img2lidar; g.feat = feat; g.feat_dt = feat_dt; g.ref2d = ref2d; g.ctx = ctx; g.box2d = box2d; g.score = score;
  g.cap = cap; g.C = C; g.hd = hd; g.wd = wd; g.nd = nd; g.ds = depth_stride;
  prop_fill_geom(g.geo, depth_min, depth_max, depth_bins, pc_range);
  g.thr_logodds = prop_thr_logodds(score_thr);
  g.N = N; g.rows_total = rows;
}

extern "C" int far3d_proposal_gather(const float* const* reg, int nreg, int N, int L, const int32_t* level_hw,
                                     const int32_t* strides, const int* sel_idx, const int* sel_cnt,
                                     int cap, const float* weights, const float* depth_logit, int hd, int wd, int nd,
                                     int depth_stride, float depth_min, float depth_max, int depth_bins,
                                     const float* img2lidar, const void* feat, int feat_dt, int C, const float* pc_range,
                                     float score_thr, float* ref2d, float* ctx, float* box2d, float* score, int rows_total,
                                     int32_t* m_out, int32_t* overflow_out, void* stream) {
  FAR3D_CHECK_ARG(reg && level_hw && strides && sel_idx && sel_cnt && weights && depth_logit && img2lidar && feat &&
                  pc_range && ref2d && ctx && box2d && score, "far3d_proposal_gather: null argument");
  FAR3D_CHECK_ARG(L >= 1 && L <= PROP_MAX_L && N > 0 && cap > 0 && rows_total >= 0, "far3d_proposal_gather: bad sizes");
  FAR3D_CHECK_ARG(rows_total > 0 || (!m_out && !overflow_out), "far3d_proposal_gather: m_out / overflow_out need rows_total > 0");
  GatherParams g;
  gather_fill(g, reg, nreg, N, L, level_hw, strides, sel_idx, sel_cnt, cap, weights, depth_logit, hd, wd, nd, depth_stride, depth_min,
              depth_max, depth_bins, img2lidar, feat, feat_dt, C, pc_range, score_thr, ref2d, ctx, box2d, score, rows_total);
  g.m_out = m_out; g.overflow_out = overflow_out;
  hipLaunchKernelGGL(prop_gather_kernel<false>, dim3(cap, rows_total > 0 ? N + 1 : N), dim3(64), 0, (hipStream_t)stream, g);
  FAR3D_CHECK_LAUNCH("far3d_proposal_gather");
  return FAR3D_OK;
}

// Multi-depth proposals, part 1 of 2 (per camera block): the primary rows of far3d_proposal_gather (same values, bit for bit) plus a
// record per primary -- valid flag, camera, top-K bins, K-1 probability ratios -- that far3d_proposal_extra_rows turns into the extra
// rows once every camera's primaries exist.  primary_rows > 0: primaries past it are dropped (fixed capacity; the extra-row launch
// flags it); 0: N * cap rows.  No bookkeeping row here: the extra-row launch writes the count, the overflow flag and the hole.
extern "C" int far3d_proposal_gather_md(const float* const* reg, int nreg, int N, int L, const int32_t* level_hw,
                                        const int32_t* strides, const int* sel_idx, const int* sel_cnt,
                                        int cap, const float* weights, const float* depth_logit, int hd, int wd, int nd,
                                        int depth_stride, float depth_min, float depth_max, int depth_bins,
                                        const float* img2lidar, const void* feat, int feat_dt, int C, const float* pc_range,
                                        float score_thr, float* ref2d, float* ctx, float* box2d, float* score, int primary_rows,
                                        int topk, int range_min_bin, int32_t* md_flags, int32_t* md_info, void* stream) {
  FAR3D_CHECK_ARG(reg && level_hw && strides && sel_idx && sel_cnt && weights && depth_logit && img2lidar && feat &&
                  pc_range && ref2d && ctx && box2d && score && md_flags && md_info, "far3d_proposal_gather_md: null argument");
  FAR3D_CHECK_ARG(L >= 1 && L <= PROP_MAX_L && N > 0 && cap > 0 && primary_rows >= 0 && C > 0, "far3d_proposal_gather_md: bad sizes");
  FAR3D_CHECK_ARG(topk >= 2 && topk <= 8 && topk <= nd && nd <= 64 * PROP_SLOTS,
                  "far3d_proposal_gather_md: need 2 <= topk <= 8, topk <= depth bins, depth bins <= %d", 64 * PROP_SLOTS);
  GatherParams g;
  gather_fill(g, reg, nreg, N, L, level_hw, strides, sel_idx, sel_cnt, cap, weights, depth_logit, hd, wd, nd, depth_stride, depth_min,
              depth_max, depth_bins, img2lidar, feat, feat_dt, C, pc_range, score_thr, ref2d, ctx, box2d, score, primary_rows);
  g.md_k = topk; g.md_min_bin = range_min_bin; g.md_flags = md_flags; g.md_info = md_info;
  hipLaunchKernelGGL(prop_gather_kernel<true>, dim3(cap, N), dim3(64), 0, (hipStream_t)stream, g);
  FAR3D_CHECK_LAUNCH("far3d_proposal_gather_md");
  return FAR3D_OK;
}

// Multi-depth proposals, part 2 of 2 (all cameras): rows [0, Mp) hold the primaries (Mp = min(sum sel_cnt, primary_rows)); for
// k = 1 .. K-1 and every valid primary m in row order, extra row Mp + (k-1) * V + rank(m) holds m's box, its context features, its
// log-odds times p_k / p_0 and the reference point of m's k-th depth bin (ref farhead.py:756-805, k-major).  Every workgroup
// counts V and ranks the valid flags itself (ballot + popcount), then writes the extras of the valid primaries whose rank is
// its own modulo the grid, and a share of the hole [M', rows_total).  The grid depends on the capacity only (graph-capturable).
struct ExtraParams {
  const int* sel_cnt; const int* flags; const int* info;
  const float* img2lidar;
  float* ref2d; float* ctx; float* box2d; float* score;
  int N, sel_cap, P, K, C, rows_total, fill_hole;
  PropGeom geo;
  int* m_out; int* overflow_out;
};

#define EXTRA_THREADS 256
__global__ __launch_bounds__(EXTRA_THREADS) void prop_extra_kernel(ExtraParams g) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, G = gridDim.x, w = blockIdx.x;
  __shared__ int s_part[EXTRA_THREADS / 64];
  __shared__ int s_list[EXTRA_THREADS];        // (primary row << 8 | chunk-local slot) of this chunk's valid primaries owned here
  __shared__ int s_rank[EXTRA_THREADS];
  __shared__ int s_n;
  int M = 0, full = 0;
  for (int k = 0; k < g.N; ++k) { M += g.sel_cnt[k]; full |= g.sel_cnt[k] >= g.sel_cap; }
  const int Mp = min(M, g.P);
  // pass 1: V
  int c = 0;
  for (int m0 = 0; m0 < Mp; m0 += EXTRA_THREADS) {
    const int m = m0 + t;
    c += __popcll(__ballot(m < Mp && g.flags[m] != 0));
  }
  if (lane == 0) s_part[wv] = c;
  __syncthreads();
  int V = 0;
#pragma unroll
  for (int q = 0; q < EXTRA_THREADS / 64; ++q) V += s_part[q];
  const long Mfull = (long)Mp + (long)(g.K - 1) * V;           // M' (rows of the reference, after the capacity of the primaries)
  const int Mq = (int)min(Mfull, (long)g.rows_total);
  if (w == 0 && t == 0) {
    if (g.m_out) *g.m_out = Mq;
    if (g.overflow_out) *g.overflow_out = (M > g.P || Mfull > g.rows_total || (g.sel_cap > 0 && full)) ? 1 : 0;
  }
  // pass 2: ranks, chunk by chunk; the valid primaries with rank % G == w are written by this workgroup (one wave per extra row)
  int base = 0;
  for (int m0 = 0; m0 < Mp; m0 += EXTRA_THREADS) {
    const int m = m0 + t;
    const bool vld = m < Mp && g.flags[m] != 0;
    const unsigned long long bm = __ballot(vld);
    const int before = __popcll(bm & ((1ull << lane) - 1ull));
    __syncthreads();                                            // s_part / s_list of the previous chunk are consumed
    if (lane == 0) s_part[wv] = __popcll(bm);
    if (t == 0) s_n = 0;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < EXTRA_THREADS / 64; ++q) { off += q < wv ? s_part[q] : 0; tot += s_part[q]; }
    const int rank = base + off + before;
    if (vld && rank % G == w) {
      const int pos = atomicAdd(&s_n, 1);
      s_list[pos] = m; s_rank[pos] = rank;
    }
    __syncthreads();
    const int nl = s_n, nrow = nl * (g.K - 1);
    for (int e = wv; e < nrow; e += EXTRA_THREADS / 64) {
      const int p = e % nl, k = 1 + e / nl;
      const int src = s_list[p];
      const long dstl = (long)Mp + (long)(k - 1) * V + s_rank[p];
      if (dstl >= g.rows_total) continue;                       // over capacity: dropped in reference order, flagged above
      const int dst = (int)dstl;
      const int* rec = g.info + (long)src * 2 * g.K;
      const int n = rec[0], bin = rec[1 + k];
      const float ratio = __int_as_float(rec[g.K + k]);
      const float* sr = g.ctx + (long)src * (g.C + 1);
      float* dr = g.ctx + (long)dst * (g.C + 1);
      for (int cc = lane; cc < g.C; cc += 64) dr[cc] = sr[cc];  // rows are C + 1 = 257 floats: dword-aligned only
      if (lane == 0) {
        dr[g.C] = sr[g.C] * ratio;
        const float bcx = g.box2d[src * 4 + 0], bcy = g.box2d[src * 4 + 1];
        PROP_BIN_TO_REF(g.geo, g.img2lidar + n * 16, bin, bcx, bcy, g.ref2d, dst * 3)   // what prop_gather_kernel expands
#pragma unroll
        for (int r = 0; r < 4; ++r) g.box2d[dst * 4 + r] = g.box2d[src * 4 + r];
        g.score[dst] = g.score[src];
      }
    }
    base += tot;
  }
  if (!g.fill_hole) return;
  // the hole [M', rows_total): zeros, so that everything computed from it downstream stays finite (masked, not removed)
  for (int row = Mq + w * (EXTRA_THREADS / 64) + wv; row < g.rows_total; row += G * (EXTRA_THREADS / 64)) PROP_ZERO_ROW(g, row, lane)
}

extern "C" int far3d_proposal_extra_rows(const int* sel_cnt, int N, int sel_cap, int primary_rows, int topk, const int32_t* md_flags,
                                         const int32_t* md_info, const float* img2lidar, float depth_min, float depth_max,
                                         int depth_bins, const float* pc_range, int C, float* ref2d, float* ctx, float* box2d,
                                         float* score, int rows_total, int fill_hole, int32_t* m_out, int32_t* overflow_out,
                                         void* stream) {
  FAR3D_CHECK_ARG(sel_cnt && md_flags && md_info && img2lidar && pc_range && ref2d && ctx && box2d && score,
                  "far3d_proposal_extra_rows: null argument");
  FAR3D_CHECK_ARG(N > 0 && primary_rows > 0 && C > 0 && rows_total >= primary_rows && depth_bins > 0,
                  "far3d_proposal_extra_rows: bad sizes");
  FAR3D_CHECK_ARG(topk >= 2 && topk <= 8 && topk <= depth_bins, "far3d_proposal_extra_rows: need 2 <= topk <= 8, topk <= depth bins");
  ExtraParams g;
  memset(&g, 0, sizeof(g));
  g.sel_cnt = sel_cnt; g.flags = md_flags; g.info = md_info; g.img2lidar = img2lidar;
  g.ref2d = ref2d; g.ctx = ctx; g.box2d = box2d; g.score = score;
  g.N = N; g.sel_cap = sel_cap; g.P = primary_rows; g.K = topk; g.C = C; g.rows_total = rows_total; g.fill_hole = fill_hole;
  prop_fill_geom(g.geo, depth_min, depth_max, depth_bins, pc_range);
  g.m_out = m_out; g.overflow_out = overflow_out;
  // a workgroup per 16 primary rows, at most 256: each scans the flags (<= a few thousand) twice and writes 1/G of the extras
  const int G = max(1, min((primary_rows + 15) / 16, 256));
  hipLaunchKernelGGL(prop_extra_kernel, dim3(G), dim3(EXTRA_THREADS), 0, (hipStream_t)stream, g);
  FAR3D_CHECK_LAUNCH("far3d_proposal_extra_rows");
  return FAR3D_OK;
}

// ------------------------------------------------------------------------------------------ block -> compact rows
// Camera-sharded fixed-capacity mode: every rank contributes a block of `rows_per_block` record rows of which the first
// counts[b] are valid (its own cameras' proposals, compacted by far3d_proposal_gather).  After the all-gather the blocks are
// packed into ONE compact run in block (= camera) order: dst rows [0, M) valid, [M, dst_rows) zero, M = min(sum counts, dst_rows).
__global__ __launch_bounds__(64) void compact_rows_kernel(const float* __restrict__ src, const int* __restrict__ counts, int nblocks,
                                                          int rows_per_block, int D, float* __restrict__ dst, int dst_rows,
                                                          int* __restrict__ m_out, int* __restrict__ overflow_out) {
  const int r = blockIdx.x, lane = threadIdx.x;
  int M = 0, b = -1, local = 0;
  for (int k = 0; k < nblocks; ++k) {
    const int c = min(max(counts[k], 0), rows_per_block);
    if (b < 0 && r < M + c) { b = k; local = r - M; }
    M += c;
  }
  if (r == 0 && lane == 0) {
    if (m_out) *m_out = min(M, dst_rows);
    if (overflow_out) *overflow_out = (*overflow_out != 0 || M > dst_rows) ? 1 : 0;
  }
  float* d = dst + (long)r * D;
  if (b >= 0) {
    const float* s = src + ((long)b * rows_per_block + local) * D;
    for (int c = lane; c < D; c += 64) d[c] = s[c];
  } else {
    for (int c = lane; c < D; c += 64) d[c] = 0.f;
  }
}

extern "C" int far3d_compact_rows(const float* src, const int32_t* counts, int nblocks, int rows_per_block, int D, float* dst,
                                  int dst_rows, int32_t* m_out, int32_t* overflow_out, void* stream) {
  FAR3D_CHECK_ARG(src && counts && dst && nblocks > 0 && rows_per_block > 0 && D > 0 && dst_rows > 0, "far3d_compact_rows: bad arguments");
  hipLaunchKernelGGL(compact_rows_kernel, dim3(dst_rows), dim3(64), 0, (hipStream_t)stream, src, (const int*)counts, nblocks, rows_per_block,
                     D, dst, dst_rows, (int*)m_out, (int*)overflow_out);
  FAR3D_CHECK_LAUNCH("far3d_compact_rows");
  return FAR3D_OK;
}
