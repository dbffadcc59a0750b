// Track ids of the detections, carried through the streaming memory (include/far3d_hip.h far3d_track_update; the CPU restatement is
// tests/track_refs.py).  The identity of an object across frames is an index chain through kernels of this library: the memory update
// pushes the top-k ranked queries to the front of the queue, the next frame's propagated queries are the queue's first P slots.
// far3d_track_update follows it on the device, one launch per frame for all scene streams, with no host read (graph-replayable).
//
// One workgroup per stream (blockIdx.x), 1024 threads.  Thread t owns ranked row t (K <= 1024):
//   1. its id: the old queue's slot if the row is a propagated one, else 0;
//   2. births: an id-less row whose score (far3d_head_finalize's plane: PROBABILITIES, -inf in a hole) is finite and >= birth_thr gets
//      next_id + its rank among the frame's births.  The rank is an exclusive prefix count in rank order: ballot + mbcnt inside a wave
//      (wave64: a 64-bit mask), the waves' totals through LDS, every thread sums the totals of the waves in front of its own;
//   3. queue shift, in place: the whole old queue is staged in LDS before the first barrier, every store to it comes after the last;
//   4. detections: the id of each decoded box's query row, found by a scan of the K ranked rows in LDS (they are distinct rows).
// One lane advances the stream's counter with a plain store.
#include "common.hpp"

#define TRACK_THREADS 1024
#define TRACK_MAXK 1024
#define TRACK_MAXL 4096
#define TRACK_MAXDEC 1024

struct TrackParams {
  const long* topk_idx;    // (K) ranked query rows
  const float* score;      // (A) score plane
  const int* query_idx;    // (Kdec) query row of every decoded box (null with Kdec 0)
  long* mem_track;         // (L) queue of ids, updated in place
  long* next_id;           // (1) counter, updated in place
  long* track_ids;         // (Kdec) out
  long s_topk, s_score, s_query, s_mem, s_next, s_ids;      // stream strides, elements
  int A, K, L, Kdec, row0, P;
  double birth_thr;
};

__global__ __launch_bounds__(TRACK_THREADS) void track_update_kernel(TrackParams p) {
  __shared__ long s_old[TRACK_MAXL];                                   // the queue as it stood before this frame
  __shared__ long s_id[TRACK_MAXK];                                    // ids of the ranked rows after the births
  __shared__ __attribute__((aligned(16))) int s_row[TRACK_MAXK];      // the ranked rows (-1: none)
  __shared__ int s_wave[TRACK_THREADS / 64];                           // births per wave
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long sb = blockIdx.x;
  const long* topk = p.topk_idx + sb * p.s_topk;
  const float* score = p.score + sb * p.s_score;
  long* mem = p.mem_track + sb * p.s_mem;
  long* next = p.next_id + sb * p.s_next;
  // every load that depends on nothing is issued here, side by side: the kernel is a chain of memory latencies, not of work
  const long r = t < p.K ? topk[t] : -1;
  const int q = t < p.Kdec ? (p.query_idx + sb * p.s_query)[t] : -1;
  const long base = *next;
  for (int i = t; i < p.L; i += TRACK_THREADS) s_old[i] = mem[i];
  __syncthreads();
  int row = -1;
  long id = 0;
  bool born = false;
  if (t < p.K) {
    if (r >= 0 && r < p.A) {                          // a row outside the plane has no identity and is never born
      row = (int)r;
      if (row >= p.row0 && row < p.row0 + p.P) id = s_old[row - p.row0];
      if (id == 0) {
        const float sc = score[row];
        born = (sc - sc == 0.f) && (double)sc >= p.birth_thr;      // finite (not the hole's -inf, not a NaN) and at the threshold
      }
    }
  }
  const unsigned long long m = __ballot(born);
  const int before = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
  if (lane == 0) s_wave[wv] = __popcll(m);
  __syncthreads();
  int carry = 0, total = 0;
#pragma unroll
  for (int w = 0; w < TRACK_THREADS / 64; ++w) {
    const int c = s_wave[w];
    carry += w < wv ? c : 0;
    total += c;
  }
  if (born) id = base + carry + before;
  s_id[t] = t < p.K ? id : 0;
  s_row[t] = row;
  __syncthreads();
  for (int i = t; i < p.L; i += TRACK_THREADS) mem[i] = i < p.K ? s_id[i] : s_old[i - p.K];
  if (t == 0) *next = base + total;
  if (t < p.Kdec) {
    long out = 0;
    const int k4 = (p.K + 3) >> 2;                    // rows past K are -1: no query row matches them
#pragma unroll 4
    for (int j = 0; j < k4; ++j) {
      const int4 rw = *reinterpret_cast<const int4*>(s_row + 4 * j);
      if (rw.x == q) out = s_id[4 * j];
      if (rw.y == q) out = s_id[4 * j + 1];
      if (rw.z == q) out = s_id[4 * j + 2];
      if (rw.w == q) out = s_id[4 * j + 3];
    }
    (p.track_ids + sb * p.s_ids)[t] = q >= 0 ? out : 0;
  }
}

extern "C" int far3d_track_update(const int64_t* topk_idx, const float* score, const int32_t* query_idx, int64_t* mem_track, int64_t* next_id,
                                  int64_t* track_ids, int B, int A, int K, int L, int Kdec, int row_start, int P, double birth_thr,
                                  const long* batch_strides, void* stream) {
  const char* who = "far3d_track_update";
  FAR3D_CHECK_ARG(topk_idx, "%s: topk_idx is a null pointer", who);
  FAR3D_CHECK_ARG(score, "%s: score is a null pointer", who);
  FAR3D_CHECK_ARG(mem_track, "%s: mem_track is a null pointer", who);
  FAR3D_CHECK_ARG(next_id, "%s: next_id is a null pointer", who);
  FAR3D_CHECK_ARG(batch_strides, "%s: batch_strides is a null pointer", who);
  FAR3D_CHECK_ARG(B >= 1 && B <= 65535, "%s: B=%d outside 1 .. 65535", who, B);
  FAR3D_CHECK_ARG(A > 0 && K > 0 && K <= TRACK_MAXK && K <= A && L > 0 && L <= TRACK_MAXL && K <= L && Kdec >= 0 && Kdec <= TRACK_MAXDEC,
                  "%s: bad sizes A=%d K=%d L=%d Kdec=%d (0 < K <= min(A, L, %d), L <= %d, Kdec <= %d)", who, A, K, L, Kdec, TRACK_MAXK,
                  TRACK_MAXL, TRACK_MAXDEC);
  FAR3D_CHECK_ARG(P >= 0 && P <= L && row_start >= 0 && (long)row_start + P <= A,
                  "%s: the propagated rows [row_start=%d, row_start + P=%d) must lie inside the A=%d rows, P <= L=%d", who, row_start, P, A, L);
  FAR3D_CHECK_ARG(P <= K, "%s: P=%d propagated slots > K=%d ranked rows: a slot that was carried over would be propagated twice", who, P, K);
  FAR3D_CHECK_ARG(Kdec == 0 || (query_idx && track_ids), "%s: Kdec=%d needs query_idx and track_ids", who, Kdec);
  FAR3D_CHECK_ARG(birth_thr == birth_thr, "%s: birth_thr is a NaN", who);
  const long extent[6] = {K, A, Kdec, L, 1, Kdec};
  static const char* const names[6] = {"topk_idx", "score", "query_idx", "mem_track", "next_id", "track_ids"};
  for (int i = 0; i < 6; ++i)
    FAR3D_CHECK_ARG(B == 1 || batch_strides[i] >= extent[i], "%s: batch_strides[%d] (%s) = %ld elements is below one stream's %ld", who, i,
                    names[i], batch_strides[i], extent[i]);
  TrackParams p;
  p.topk_idx = (const long*)topk_idx; p.score = score; p.query_idx = query_idx; p.mem_track = (long*)mem_track; p.next_id = (long*)next_id;
  p.track_ids = (long*)track_ids;
  p.s_topk = batch_strides[0]; p.s_score = batch_strides[1]; p.s_query = batch_strides[2]; p.s_mem = batch_strides[3];
  p.s_next = batch_strides[4]; p.s_ids = batch_strides[5];
  p.A = A; p.K = K; p.L = L; p.Kdec = Kdec; p.row0 = row_start; p.P = P; p.birth_thr = birth_thr;
  hipLaunchKernelGGL(track_update_kernel, dim3(B), dim3(TRACK_THREADS), 0, (hipStream_t)stream, p);
  FAR3D_CHECK_LAUNCH(who);
  return FAR3D_OK;
}

// Track records (include/far3d_hip.h far3d_track_records; the CPU restatement is tests/track_record_refs.py): per frame, behind
// far3d_track_update on the same stream, the age of every id (a counter plane beside the id queue, shifted like it), ONE primary box
// per id and a velocity from the streaming memory's warped previous centre.  One workgroup per stream, 1024 threads.  Thread t owns
// ranked row t (its new hit count) and decoded box t (age, primary, velocity).  LDS: the old hits plane (16 KB, staged before the
// first store to it), the ranked rows and their new hits (8 KB), the boxes' ids with the keep bit folded in (8 KB; 0 = not a
// candidate for primary).  No dynamic LDS, no atomics, no host read.
struct TrackRecParams {
  const long* topk_idx;         // (K) ranked query rows
  const long* mem_track;        // (L) id queue as far3d_track_update left it: [0, K) the ranked rows' ids
  const int* query_idx;         // (Kdec) query row of every decoded box
  const long* track_ids;        // (Kdec) far3d_track_update's ids of the boxes
  const unsigned char* keep;    // (Kdec) the decode's keep flags
  const float* boxes;           // (Kdec, box_stride) decoded boxes, centre in [0, 3)
  const float* m_ref;           // (L, 3) the pre-updated memory's centres, warped into this frame
  const double* m_ts;           // (L) seconds since each centre was written
  int* mem_hits;                // (L) frames each slot's id has been ranked, updated in place
  int* age;                     // (Kdec) out
  unsigned char* primary;       // (Kdec) out
  float* velocity;              // (Kdec, 3) out
  long s_topk, s_mem, s_query, s_ids, s_keep, s_box, s_ref, s_ts, s_hits, s_age, s_prim, s_vel;      // stream strides, elements
  int A, K, L, Kdec, row0, P, box_stride;
};

__global__ __launch_bounds__(TRACK_THREADS) void track_records_kernel(TrackRecParams p) {
  __shared__ int s_old[TRACK_MAXL];                                    // the hits plane as it stood before this frame
  __shared__ __attribute__((aligned(16))) int s_row[TRACK_MAXK];      // the ranked rows (-1: none)
  __shared__ int s_hit[TRACK_MAXK];                                    // their new hit counts
  __shared__ __attribute__((aligned(16))) long s_key[TRACK_MAXDEC];   // id of a kept box, 0 for any other
  const int t = threadIdx.x, wv = t >> 6;
  const long sb = blockIdx.x;
  int* hits = p.mem_hits + sb * p.s_hits;
  // the independent loads side by side, then the two that hang on the box's query row
  const long r = t < p.K ? (p.topk_idx + sb * p.s_topk)[t] : -1;
  const long idk = t < p.K ? (p.mem_track + sb * p.s_mem)[t] : 0;
  int q = -1;
  long tid = 0;
  bool kept = false;
  float bx = 0.f, by = 0.f, bz = 0.f;
  if (t < p.Kdec) {
    q = (p.query_idx + sb * p.s_query)[t];
    tid = (p.track_ids + sb * p.s_ids)[t];
    kept = (p.keep + sb * p.s_keep)[t] != 0;
    const float* b = p.boxes + sb * p.s_box + (long)t * p.box_stride;
    bx = b[0]; by = b[1]; bz = b[2];
  }
  for (int i = t; i < p.L; i += TRACK_THREADS) s_old[i] = hits[i];
  const int slot = (q >= p.row0 && q < p.row0 + p.P) ? q - p.row0 : -1;      // the memory slot a propagated query came from (P <= L)
  float rx = 0.f, ry = 0.f, rz = 0.f;
  double ts = 0.0;
  if (slot >= 0) {
    const float* m = p.m_ref + sb * p.s_ref + 3l * slot;
    rx = m[0]; ry = m[1]; rz = m[2];
    ts = (p.m_ts + sb * p.s_ts)[slot];
  }
  s_key[t] = kept ? tid : 0;
  __syncthreads();
  int row = -1, hn = 0;
  if (t < p.K) {
    if (r >= 0 && r < p.A) row = (int)r;               // a row outside the plane matches no box, as in track_update
    const int ho = (row >= p.row0 && row < p.row0 + p.P) ? s_old[row - p.row0] : 0;
    hn = ho > 0 ? ho + 1 : (idk != 0 ? 1 : 0);        // inherited: one frame older; a birth: 1; no identity: 0
  }
  s_hit[t] = hn;
  s_row[t] = row;
  __syncthreads();
  for (int i = t; i < p.L; i += TRACK_THREADS) hits[i] = i < p.K ? s_hit[i] : s_old[i - p.K];
  if (t < p.Kdec) {
    int rk = -1;
    const int k4 = (p.K + 3) >> 2;                    // rows past K are -1: no query row matches them
#pragma unroll 4
    for (int j = 0; j < k4; ++j) {
      const int4 rw = *reinterpret_cast<const int4*>(s_row + 4 * j);
      if (rw.x == q) rk = 4 * j;
      if (rw.y == q) rk = 4 * j + 1;
      if (rw.z == q) rk = 4 * j + 2;
      if (rw.w == q) rk = 4 * j + 3;
    }
    if (q < 0) rk = -1;
    (p.age + sb * p.s_age)[t] = (tid != 0 && rk >= 0) ? s_hit[rk] - 1 : -1;
    // velocity: only for a box whose query inherited its identity from a slot with a finite, positive age in seconds
    float vx = 0.f, vy = 0.f, vz = 0.f;
    if (rk >= 0 && slot >= 0 && s_old[slot] > 0 && ts > 0.0 && ts - ts == 0.0) {
      const float dt = (float)ts;
      vx = (bx - rx) / dt; vy = (by - ry) / dt; vz = (bz - rz) / dt;
    }
    float* v = p.velocity + sb * p.s_vel + 3l * t;
    v[0] = vx; v[1] = vy; v[2] = vz;
  }
  // primary: the first kept box of its id.  Every wave scans the keys in front of its last lane (wave-uniform bound, broadcast reads)
  const long key = s_key[t];
  bool first = key != 0;
  const int n2 = min(p.Kdec, (wv + 1) * 64) >> 1;     // pairs of keys wholly or partly in front of this wave's lanes
  for (int j = 0; j < n2; ++j) {
    const long2 kk = *reinterpret_cast<const long2*>(s_key + 2 * j);
    if (kk.x == key && 2 * j < t) first = false;
    if (kk.y == key && 2 * j + 1 < t) first = false;
  }
  if (t < p.Kdec) (p.primary + sb * p.s_prim)[t] = first ? 1 : 0;
}

extern "C" int far3d_track_records(const int64_t* topk_idx, const int64_t* mem_track, const int32_t* query_idx, const int64_t* track_ids,
                                   const unsigned char* keep, const float* boxes, const float* m_ref, const double* m_ts,
                                   int32_t* mem_hits, int32_t* track_age, unsigned char* track_primary, float* track_velocity, int B,
                                   int A, int K, int L, int Kdec, int row_start, int P, int box_stride, const long* batch_strides,
                                   void* stream) {
  const char* who = "far3d_track_records";
  FAR3D_CHECK_ARG(topk_idx, "%s: topk_idx is a null pointer", who);
  FAR3D_CHECK_ARG(mem_track, "%s: mem_track is a null pointer", who);
  FAR3D_CHECK_ARG(m_ref, "%s: m_ref is a null pointer", who);
  FAR3D_CHECK_ARG(m_ts, "%s: m_ts is a null pointer", who);
  FAR3D_CHECK_ARG(mem_hits, "%s: mem_hits is a null pointer", who);
  FAR3D_CHECK_ARG(batch_strides, "%s: batch_strides is a null pointer", who);
  FAR3D_CHECK_ARG(B >= 1 && B <= 65535, "%s: B=%d outside 1 .. 65535", who, B);
  FAR3D_CHECK_ARG(A > 0 && K > 0 && K <= TRACK_MAXK && K <= A && L > 0 && L <= TRACK_MAXL && K <= L && Kdec >= 0 && Kdec <= TRACK_MAXDEC,
                  "%s: bad sizes A=%d K=%d L=%d Kdec=%d (0 < K <= min(A, L, %d), L <= %d, Kdec <= %d)", who, A, K, L, Kdec, TRACK_MAXK,
                  TRACK_MAXL, TRACK_MAXDEC);
  FAR3D_CHECK_ARG(P >= 0 && P <= L && row_start >= 0 && (long)row_start + P <= A,
                  "%s: the propagated rows [row_start=%d, row_start + P=%d) must lie inside the A=%d rows, P <= L=%d", who, row_start, P, A, L);
  FAR3D_CHECK_ARG(P <= K, "%s: P=%d propagated slots > K=%d ranked rows: a slot that was carried over would be propagated twice", who, P, K);
  FAR3D_CHECK_ARG(box_stride >= 3, "%s: box_stride=%d is below the 3 floats of a centre", who, box_stride);
  if (Kdec > 0) {
    FAR3D_CHECK_ARG(query_idx, "%s: query_idx is a null pointer (Kdec=%d)", who, Kdec);
    FAR3D_CHECK_ARG(track_ids, "%s: track_ids is a null pointer (Kdec=%d)", who, Kdec);
    FAR3D_CHECK_ARG(keep, "%s: keep is a null pointer (Kdec=%d)", who, Kdec);
    FAR3D_CHECK_ARG(boxes, "%s: boxes is a null pointer (Kdec=%d)", who, Kdec);
    FAR3D_CHECK_ARG(track_age, "%s: track_age is a null pointer (Kdec=%d)", who, Kdec);
    FAR3D_CHECK_ARG(track_primary, "%s: track_primary is a null pointer (Kdec=%d)", who, Kdec);
    FAR3D_CHECK_ARG(track_velocity, "%s: track_velocity is a null pointer (Kdec=%d)", who, Kdec);
  }
  const long extent[12] = {K, L, Kdec, Kdec, Kdec, (long)Kdec * box_stride, 3l * L, L, L, Kdec, Kdec, 3l * Kdec};
  static const char* const names[12] = {"topk_idx", "mem_track", "query_idx", "track_ids", "keep", "boxes", "m_ref", "m_ts", "mem_hits",
                                        "track_age", "track_primary", "track_velocity"};
  for (int i = 0; i < 12; ++i)
    FAR3D_CHECK_ARG(B == 1 || batch_strides[i] >= extent[i], "%s: batch_strides[%d] (%s) = %ld elements is below one stream's %ld", who, i,
                    names[i], batch_strides[i], extent[i]);
  TrackRecParams p;
  p.topk_idx = (const long*)topk_idx; p.mem_track = (const long*)mem_track; p.query_idx = query_idx; p.track_ids = (const long*)track_ids;
  p.keep = keep; p.boxes = boxes; p.m_ref = m_ref; p.m_ts = m_ts; p.mem_hits = mem_hits; p.age = track_age; p.primary = track_primary;
  p.velocity = track_velocity;
  p.s_topk = batch_strides[0]; p.s_mem = batch_strides[1]; p.s_query = batch_strides[2]; p.s_ids = batch_strides[3];
  p.s_keep = batch_strides[4]; p.s_box = batch_strides[5]; p.s_ref = batch_strides[6]; p.s_ts = batch_strides[7];
  p.s_hits = batch_strides[8]; p.s_age = batch_strides[9]; p.s_prim = batch_strides[10]; p.s_vel = batch_strides[11];
  p.A = A; p.K = K; p.L = L; p.Kdec = Kdec; p.row0 = row_start; p.P = P; p.box_stride = box_stride;
  hipLaunchKernelGGL(track_records_kernel, dim3(B), dim3(TRACK_THREADS), 0, (hipStream_t)stream, p);
  FAR3D_CHECK_LAUNCH(who);
  return FAR3D_OK;
}
