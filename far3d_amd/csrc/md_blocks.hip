// Proposals of camera BLOCKS -> the frame's layout (HBM-bound word moves, no arithmetic on the rows):
//   far3d_proposal_merge_blocks  every block (a contiguous run of cameras, processed on its own by far3d_proposal_gather or
//                                far3d_proposal_gather_md) holds its primaries compacted camera-major in rows [0, count_b) of its own
//                                buffers.  The frame's buffers want them back to back in block (= camera) order -- rows [0, Mp) -- with
//                                the multi-depth records beside them (camera field rebased to the frame's camera index), the frame's
//                                sel_cnt, ONE count and ONE overflow flag: exactly what far3d_proposal_gather(_md) on all cameras would
//                                have left, so that far3d_proposal_extra_rows (multi-depth) or the head (single depth) runs unchanged.
//   far3d_proposal_pack_block    one multi-depth block -> ONE record of words (header, sel_cnt, img2lidar, the six arrays) for a rank's
//                                exchange; the merge then reads the gathered records in place (end of this file).
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

// far3d_proposal_pack_block: what a camera block's far3d_proposal_gather_md left -> ONE contiguous record of 4-byte words, the unit a
// rank of the camera-sharded runner puts into the frame's exchange (far3d_amd/dist.py).  Sections, each starting on a 16-byte boundary:
//   header (4 words: cameras, effective count, overflow flag, 0) | sel_cnt (per) | img2lidar (per*16) | ref2d (rows*3) |
//   ctx (rows*(C+1)) | box2d (rows*4) | score (rows) | md_flags (rows) | md_info (rows*2K)
// The first `count` rows of every array are copied, every other word of the record is zero-filled (padding camera slots, rows past the
// count, alignment gaps): the record is a function of the valid rows alone, and far3d_proposal_merge_blocks reads its sections in place.
#define PACK_SECTIONS 9

struct PackParams {
  const uint32_t* src[PACK_SECTIONS];                // [0] unused (header), [1] sel_cnt, [2] img2lidar, [3..8] the six row arrays
  long off[PACK_SECTIONS + 1];                       // word offsets of the sections; off[PACK_SECTIONS] = the record's words
  int width[PACK_SECTIONS];                          // words per row (sel_cnt: per camera 1, img2lidar: per camera 16)
  uint32_t* dst;
  const int* sel_cnt;
  const int* overflow_in;                            // device int32 or null
  int cams, rows_src, rows, host_count;              // host_count < 0: min(sum sel_cnt, rows_src)
};

// the section offsets of a record (words); shared by the launcher's check of the caller's record size
static void pack_layout(int per, int rows, int C, int K, long* off, int* width) {
  const int w[PACK_SECTIONS] = {4, 1, 16, 3, C + 1, 4, 1, 1, 2 * K};
  long o = 0;
  for (int s = 0; s < PACK_SECTIONS; ++s) {
    const long n = s == 0 ? 4 : (long)(s <= 2 ? per : rows) * w[s];
    width[s] = w[s];
    off[s] = o;
    o = (o + n + 3) & ~3l;
  }
  off[PACK_SECTIONS] = o;
}

__global__ __launch_bounds__(MERGE_THREADS) void pack_block_kernel(PackParams g) {
  const long tid = (long)blockIdx.x * MERGE_THREADS + threadIdx.x, nth = (long)gridDim.x * MERGE_THREADS;
  // the same count rule as merge_blocks_kernel; every workgroup walks the (few) camera counts itself
  int c, flag = 0;
  if (g.host_count >= 0) {
    c = g.host_count;
  } else {
    c = 0;
    for (int n = 0; n < g.cams; ++n) c += g.sel_cnt[n];
    flag |= c > g.rows_src;
  }
  c = min(max(c, 0), min(g.rows_src, g.rows));
  if (g.overflow_in) flag |= *g.overflow_in != 0;
  if (tid == 0) *reinterpret_cast<uint4*>(g.dst) = make_uint4((unsigned)g.cams, (unsigned)c, (unsigned)flag, 0u);
  for (int s = 1; s < PACK_SECTIONS; ++s) {
    const long valid = (long)(s <= 2 ? g.cams : c) * g.width[s];
    uint32_t* d = g.dst + g.off[s];
    copy_words<false>(d, g.src[s], valid, tid, nth, 1, 0);
    zero_words(d + valid, g.off[s + 1] - g.off[s] - valid, tid, nth);
  }
}

extern "C" int far3d_proposal_pack_block(int cams, int per, int block_rows, int rows, int C, int topk, const int32_t* sel_cnt,
                                         const float* img2lidar, const float* ref2d, const float* ctx, const float* box2d,
                                         const float* score, const int32_t* md_flags, const int32_t* md_info, int count_host,
                                         const int32_t* overflow_in, float* record, long record_words, void* stream) {
  FAR3D_CHECK_ARG(record && per > 0 && rows > 0 && C > 0 && topk >= 2 && topk <= 8, "far3d_proposal_pack_block: bad sizes or null record");
  FAR3D_CHECK_ARG(cams >= 0 && cams <= per && block_rows >= 0 && block_rows <= rows && count_host <= block_rows,
                  "far3d_proposal_pack_block: 0 <= cams <= per, 0 <= block_rows <= rows, count <= block_rows");
  FAR3D_CHECK_ARG(cams == 0 ? (block_rows == 0 && count_host <= 0)
                            : (block_rows > 0 && sel_cnt && img2lidar && ref2d && ctx && box2d && score && md_flags && md_info),
                  "far3d_proposal_pack_block: a block with cameras needs every array; the empty block has no rows");
  FAR3D_CHECK_ARG((reinterpret_cast<uintptr_t>(record) & 15) == 0, "far3d_proposal_pack_block: the record must be 16-byte aligned");
  PackParams g;
  memset(&g, 0, sizeof(g));
  pack_layout(per, rows, C, topk, g.off, g.width);
  FAR3D_CHECK_ARG(record_words == g.off[PACK_SECTIONS], "far3d_proposal_pack_block: the record has %ld words, the layout %ld", record_words,
                  g.off[PACK_SECTIONS]);
  const void* src[PACK_SECTIONS] = {nullptr, sel_cnt, img2lidar, ref2d, ctx, box2d, score, md_flags, md_info};
  for (int s = 0; s < PACK_SECTIONS; ++s) g.src[s] = reinterpret_cast<const uint32_t*>(src[s]);
  g.dst = reinterpret_cast<uint32_t*>(record);
  g.sel_cnt = sel_cnt; g.overflow_in = overflow_in;
  g.cams = cams; g.rows_src = block_rows; g.rows = rows; g.host_count = count_host;
  // static sizes only: a thread per 16 bytes of the record, at most 256 workgroups
  const int G = (int)max(1l, min((g.off[PACK_SECTIONS] + 4 * MERGE_THREADS - 1) / (4 * MERGE_THREADS), 256l));
  hipLaunchKernelGGL(pack_block_kernel, dim3(G), dim3(MERGE_THREADS), 0, (hipStream_t)stream, g);
  FAR3D_CHECK_LAUNCH("far3d_proposal_pack_block");
  return FAR3D_OK;
}
