// Proposals of camera BLOCKS -> the frame's layout (HBM-bound word moves, no arithmetic on the rows):
//   far3d_proposal_merge_blocks  every block (a contiguous run of cameras, processed on its own by far3d_proposal_gather or
//                                far3d_proposal_gather_md) holds its primaries compacted camera-major in rows [0, count_b) of its own
//                                buffers.  The frame's buffers want them back to back in block (= camera) order -- rows [0, Mp) -- with
//                                the multi-depth records beside them (camera field rebased to the frame's camera index), the frame's
//                                sel_cnt, ONE count and ONE overflow flag: exactly what far3d_proposal_gather(_md) on all cameras would
//                                have left, so that far3d_proposal_extra_rows (multi-depth) or the head (single depth) runs unchanged.
// Because a block's rows stay contiguous, every array of a block is ONE run of words that moves to ONE run of the frame's array:
// the kernel is a set of flat copies, 16 bytes per lane wherever source and destination share their alignment modulo 16 bytes
// (always for box2d and the records of an even K; for the 257-word context rows whenever the block's row offset is a multiple of 4).
#include "common.hpp"

#define MERGE_MAX_BLOCKS 16
#define MERGE_THREADS 256
#define MERGE_ARRAYS 6            // ref2d, ctx, box2d, score, md_flags, md_info

struct MergeBlock {
  const uint32_t* src[MERGE_ARRAYS];
  const int* sel_cnt;             // (cams) device
  const int* count;               // device int32 or null
  const int* overflow;            // device int32 or null
  int host_count;                 // used when count is null; < 0: min(sum sel_cnt, rows)
  int first_cam, cams, rows;      // rows: rows of the block's buffers (the count is clamped to it)
};

struct MergeParams {
  MergeBlock b[MERGE_MAX_BLOCKS];
  uint32_t* dst[MERGE_ARRAYS];
  int* sel_cnt; int* m_out; int* overflow_out;
  int nblocks, C, K, P, rows_total, md;
};

// d[i] = s[i] for i in [0, n), shared among all threads of the grid (tid of nth).  REBASE: word i with i % period == 0 gets `add`
// added (the camera field of an md_info row; the run starts at a row boundary).  dwordx4 body when both ends agree modulo 16 bytes.
template <bool REBASE>
__device__ __forceinline__ void copy_words(uint32_t* __restrict__ d, const uint32_t* __restrict__ s, long n, long tid, long nth,
                                           int period, int add) {
  if (n <= 0) return;
  const unsigned ma = (unsigned)(reinterpret_cast<uintptr_t>(d) >> 2) & 3u, mb = (unsigned)(reinterpret_cast<uintptr_t>(s) >> 2) & 3u;
  long head = 0, body = 0;
  if (ma == mb) {                                    // grid-uniform
    head = min((long)((4u - ma) & 3u), n);
    body = (n - head) >> 2;
    for (long i = tid; i < body; i += nth) {
      const long e = head + 4 * i;
      uint4 v = *reinterpret_cast<const uint4*>(s + e);
      if (REBASE) {
        if (e % period == 0) v.x += add;
        if ((e + 1) % period == 0) v.y += add;
        if ((e + 2) % period == 0) v.z += add;
        if ((e + 3) % period == 0) v.w += add;
      }
      *reinterpret_cast<uint4*>(d + e) = v;
    }
  }
  // the words before the first and after the last 16-byte unit (or every word, when the two ends disagree)
  const long tail0 = head + 4 * body;
  for (long i = tid; i < head + (n - tail0); i += nth) {
    const long e = i < head ? i : tail0 + (i - head);
    uint32_t v = s[e];
    if (REBASE && e % period == 0) v += add;
    d[e] = v;
  }
}

__device__ __forceinline__ void zero_words(uint32_t* __restrict__ d, long n, long tid, long nth) {
  if (n <= 0) return;
  const unsigned ma = (unsigned)(reinterpret_cast<uintptr_t>(d) >> 2) & 3u;
  const long head = min((long)((4u - ma) & 3u), n), body = (n - head) >> 2, tail0 = head + 4 * body;
  for (long i = tid; i < body; i += nth) *reinterpret_cast<uint4*>(d + head + 4 * i) = make_uint4(0u, 0u, 0u, 0u);
  for (long i = tid; i < head + (n - tail0); i += nth) d[i < head ? i : tail0 + (i - head)] = 0u;
}

__global__ __launch_bounds__(MERGE_THREADS) void merge_blocks_kernel(MergeParams g) {
  const long tid = (long)blockIdx.x * MERGE_THREADS + threadIdx.x, nth = (long)gridDim.x * MERGE_THREADS;
  const int width[MERGE_ARRAYS] = {3, g.C + 1, 4, 1, 1, 2 * g.K};
  const int narr = g.md ? MERGE_ARRAYS : 4;
  // every workgroup walks the (at most 16) block counts itself: the running sum is the block's first row in the frame
  long sum = 0;
  int flag = 0;
  for (int k = 0; k < g.nblocks; ++k) {
    const MergeBlock& b = g.b[k];
    int c;
    if (b.count) {
      c = *b.count;
    } else if (b.host_count >= 0) {
      c = b.host_count;
    } else {
      c = 0;
      for (int n = 0; n < b.cams; ++n) c += b.sel_cnt[n];
      flag |= c > b.rows;                            // far3d_proposal_gather_md dropped the rest and leaves no flag of its own
    }
    c = min(max(c, 0), b.rows);
    if (b.overflow) flag |= *b.overflow != 0;
    const long take = min((long)c, max((long)g.P - sum, 0l));      // rows of this block that fit below primary_rows
    for (int a = 0; a < narr; ++a) {
      const long w = width[a];
      if (a == 5) copy_words<true>(g.dst[a] + sum * w, b.src[a], take * w, tid, nth, (int)w, b.first_cam);
      else copy_words<false>(g.dst[a] + sum * w, b.src[a], take * w, tid, nth, 1, 0);
    }
    if (blockIdx.x == 0)
      for (int n = threadIdx.x; n < b.cams; n += MERGE_THREADS) g.sel_cnt[b.first_cam + n] = b.sel_cnt[n];
    sum += c;
  }
  const int Mp = (int)min(sum, (long)g.P);
  if (tid == 0) {
    if (g.m_out) *g.m_out = Mp;
    if (g.overflow_out) *g.overflow_out = (flag || sum > g.P) ? 1 : 0;
  }
  if (g.md) return;                                  // rows [Mp, rows_total) belong to far3d_proposal_extra_rows
  for (int a = 0; a < 4; ++a) zero_words(g.dst[a] + (long)Mp * width[a], (long)(g.rows_total - Mp) * width[a], tid, nth);
}

extern "C" int far3d_proposal_merge_blocks(int nblocks, const float* const* ref2d, const float* const* ctx, const float* const* box2d,
                                           const float* const* score, const int32_t* const* md_flags, const int32_t* const* md_info,
                                           const int32_t* const* sel_cnt, const int32_t* const* count_dev, const int32_t* count_host,
                                           const int32_t* const* overflow, const int32_t* first_cam, const int32_t* block_cams,
                                           const int32_t* block_rows, int N, int C, int topk, int primary_rows, int rows_total,
                                           float* o_ref2d, float* o_ctx, float* o_box2d, float* o_score, int32_t* o_md_flags,
                                           int32_t* o_md_info, int32_t* o_sel_cnt, int32_t* m_out, int32_t* overflow_out, void* stream) {
  FAR3D_CHECK_ARG(ref2d && ctx && box2d && score && sel_cnt && first_cam && block_cams && block_rows && o_ref2d && o_ctx && o_box2d &&
                  o_score && o_sel_cnt, "far3d_proposal_merge_blocks: null argument");
  FAR3D_CHECK_ARG(nblocks >= 1 && nblocks <= MERGE_MAX_BLOCKS, "far3d_proposal_merge_blocks: 1 <= nblocks <= %d", MERGE_MAX_BLOCKS);
  FAR3D_CHECK_ARG(N > 0 && C > 0 && primary_rows > 0 && rows_total >= primary_rows, "far3d_proposal_merge_blocks: bad sizes");
  const int md = (md_flags || md_info || o_md_flags || o_md_info) ? 1 : 0;
  FAR3D_CHECK_ARG(!md || (md_flags && md_info && o_md_flags && o_md_info && topk >= 2 && topk <= 8),
                  "far3d_proposal_merge_blocks: the records need md_flags and md_info of every block and of the frame, 2 <= topk <= 8");
  MergeParams g;
  memset(&g, 0, sizeof(g));
  int cam = 0;
  for (int k = 0; k < nblocks; ++k) {
    MergeBlock& b = g.b[k];
    FAR3D_CHECK_ARG(ref2d[k] && ctx[k] && box2d[k] && score[k] && sel_cnt[k] && (!md || (md_flags[k] && md_info[k])),
                    "far3d_proposal_merge_blocks: block %d: null array", k);
    FAR3D_CHECK_ARG(first_cam[k] == cam && block_cams[k] > 0 && block_rows[k] > 0,
                    "far3d_proposal_merge_blocks: block %d: the blocks are contiguous camera runs in ascending order with rows > 0", k);
    cam += block_cams[k];
    b.src[0] = reinterpret_cast<const uint32_t*>(ref2d[k]); b.src[1] = reinterpret_cast<const uint32_t*>(ctx[k]);
    b.src[2] = reinterpret_cast<const uint32_t*>(box2d[k]); b.src[3] = reinterpret_cast<const uint32_t*>(score[k]);
    b.src[4] = md ? reinterpret_cast<const uint32_t*>(md_flags[k]) : nullptr;
    b.src[5] = md ? reinterpret_cast<const uint32_t*>(md_info[k]) : nullptr;
    b.sel_cnt = sel_cnt[k];
    b.count = count_dev ? count_dev[k] : nullptr;
    b.host_count = count_host ? count_host[k] : -1;
    b.overflow = overflow ? overflow[k] : nullptr;
    b.first_cam = first_cam[k]; b.cams = block_cams[k]; b.rows = block_rows[k];
  }
  FAR3D_CHECK_ARG(cam == N, "far3d_proposal_merge_blocks: the blocks hold %d cameras, the frame %d", cam, N);
  g.dst[0] = reinterpret_cast<uint32_t*>(o_ref2d); g.dst[1] = reinterpret_cast<uint32_t*>(o_ctx);
  g.dst[2] = reinterpret_cast<uint32_t*>(o_box2d); g.dst[3] = reinterpret_cast<uint32_t*>(o_score);
  g.dst[4] = reinterpret_cast<uint32_t*>(o_md_flags); g.dst[5] = reinterpret_cast<uint32_t*>(o_md_info);
  g.sel_cnt = o_sel_cnt; g.m_out = m_out; g.overflow_out = overflow_out;
  g.nblocks = nblocks; g.C = C; g.K = md ? topk : 1; g.P = primary_rows; g.rows_total = rows_total; g.md = md;
  // static sizes only: a thread per 16 bytes of the rows the launch can touch, at most 256 workgroups
  const long words = (long)(md ? primary_rows : rows_total) * (C + 9 + (md ? 2 * topk + 1 : 0));
  const int G = (int)max(1l, min((words + 4 * MERGE_THREADS - 1) / (4 * MERGE_THREADS), 256l));
  hipLaunchKernelGGL(merge_blocks_kernel, dim3(G), dim3(MERGE_THREADS), 0, (hipStream_t)stream, g);
  FAR3D_CHECK_LAUNCH("far3d_proposal_merge_blocks");
  return FAR3D_OK;
}
