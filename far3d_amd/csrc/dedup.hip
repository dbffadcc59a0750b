// Duplicate suppression of the decoded boxes on the device (include/far3d_hip.h far3d_box_dedup; the contract, executable, is
// tests/dedup_refs.py): a greedy pass in the decode's order over the rotated bird's-eye-view footprints -- box i is dropped iff a
// surviving box j < i overlaps it (IoU above thr, or centres closer than thr).  One launch per frame for all scene streams, no host
// read, no atomics (graph-replayable).
//
// One workgroup per stream (blockIdx.x), 1024 threads = 16 waves, Kdec <= 1024.  Four phases, a barrier between each two:
//   1. records: thread t stages box t in LDS (centre, half extents, cos / sin of the yaw, circumradius, label) and a flag: the box can
//      take part in a pair (a judgeable candidate).
//   2. pairs: a wave owns units (suppressor j, 64-wide chunk c of the boxes i): the suppressor is wave-uniform (broadcast LDS reads),
//      lane l judges box i = 64 c + l, and __ballot gives word M[c][j] of the hit matrix.  Only j < i can hit, so chunk c has rows
//      j < 64 (c + 1): the matrix is a triangle of 64 * (1 + ... + 16) = 8704 words, 68 KB -- IN LDS, beside 36 KB of records (no
//      workspace).  The waves take the rows of a chunk round robin.
//   3. greedy: wave 0 walks the chunks.  Word c of the suppressed mask is the OR of the rows of the survivors in front of the chunk
//      (lane l ORs rows 64 jb + l, one butterfly per chunk), then the diagonal 64 x 64 block is resolved in registers: 64 unrolled
//      steps, row k read with readlane, ORed in iff box k still stands.
//   4. outputs: thread t writes dup_keep[t]; a suppressed box scans the rows in front of it for the first survivor that hit it (its
//      wave reads one matrix word per row, a broadcast) and stops when every lane of the wave has found its own.
//
// The overlap of two rectangles, in the suppressor's frame (translate by c_i - c_j, rotate by -yaw_j: the suppressor is the axis-aligned
// Q = [-a, a] x [-b, b], coordinates stay small at any range): the boundary of P n Q is made of the parts of P's edges inside Q and the
// parts of Q's edges inside P, so the area is half the sum of cross(start, end) over those parts (Green) -- eight segment clips, every
// index a compile-time constant, no polygon of variable length.  P's edges are clipped to the CLOSED Q, Q's edges to the OPEN P, both
// from the same four corner points of P, so that a shared piece of boundary is counted once: an edge of P that lies on an edge of Q
// counts iff the two run the same way (identical boxes: the whole of P; boxes that touch from outside: nothing).  The sum is taken
// about the centre of the smaller rectangle.
#include "common.hpp"

#define DEDUP_THREADS 1024
#define DEDUP_MAXK 1024
#define DEDUP_WAVES (DEDUP_THREADS / 64)
#define DEDUP_WORDS (64 * (DEDUP_WAVES * (DEDUP_WAVES + 1) / 2))

struct DedupParams {
  const float* boxes;            // (Kdec, box_stride)
  const float* scores;           // (Kdec)
  const long* labels;            // (Kdec)
  const unsigned char* keep;     // (Kdec)
  unsigned char* dup_keep;       // (Kdec) out
  int* dup_of;                   // (Kdec) out
  float* overlap;                // (Kdec, Kdec) out, or null
  long s_box, s_score, s_label, s_keep, s_dk, s_of, s_ov;      // stream strides, elements
  int Kdec, box_stride, mode, class_aware;
  float thr;                     // IoU: the threshold; centre: its square
  double score_thr;
};

__device__ __forceinline__ bool dd_finite(float v) { return v - v == 0.f; }

// one half-plane against the segment's parameter range: g0, g1 the signed distances of its ends (inside: >= 0).  An edge ON the line
// stays iff `same` (it runs the way the rectangle's own edge does)
__device__ __forceinline__ void dd_clip_closed(float g0, float g1, bool same, float& t0, float& t1, bool& ok) {
  if (g0 < 0.f && g1 < 0.f) ok = false;
  else if (g0 == 0.f && g1 == 0.f) ok = ok && same;
  else if (g0 < 0.f) t0 = fmaxf(t0, g0 / (g0 - g1));
  else if (g1 < 0.f) t1 = fminf(t1, g0 / (g0 - g1));
}

// the same against an open half-plane (inside: > 0)
__device__ __forceinline__ void dd_clip_open(float f0, float f1, float& t0, float& t1, bool& ok) {
  if (f0 <= 0.f && f1 <= 0.f) ok = false;
  else if (f0 <= 0.f) t0 = fmaxf(t0, f0 / (f0 - f1));
  else if (f1 <= 0.f) t1 = fminf(t1, f0 / (f0 - f1));
}

// IoU of Q (centre 0, half extents a, b, axis-aligned) and P (centre (lx, ly), half extents hx, hy, turned by (cr, sr)), both of
// judgeable boxes
__device__ __forceinline__ float dd_iou_local(float a, float b, float lx, float ly, float cr, float sr, float hx, float hy) {
  const float ux = hx * cr, uy = hx * sr, vx = -hy * sr, vy = hy * cr;
  const float px[4] = {lx + ux + vx, lx - ux + vx, lx - ux - vx, lx + ux - vx};      // counter-clockwise
  const float py[4] = {ly + uy + vy, ly - uy + vy, ly - uy - vy, ly + uy - vy};
  const float qx[4] = {a, a, -a, -a}, qy[4] = {-b, b, b, -b};                        // counter-clockwise
  const float areaQ = 4.f * a * b, areaP = 4.f * hx * hy;
  const float ox = areaP < areaQ ? lx : 0.f, oy = areaP < areaQ ? ly : 0.f;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {             // P's edges inside the closed Q
    const float x0 = px[k], y0 = py[k], x1 = px[(k + 1) & 3], y1 = py[(k + 1) & 3];
    float t0 = 0.f, t1 = 1.f;
    bool ok = true;
    dd_clip_closed(a - x0, a - x1, y1 > y0, t0, t1, ok);
    dd_clip_closed(b - y0, b - y1, x1 < x0, t0, t1, ok);
    dd_clip_closed(x0 + a, x1 + a, y1 < y0, t0, t1, ok);
    dd_clip_closed(y0 + b, y1 + b, x1 > x0, t0, t1, ok);
    if (ok && t1 > t0) {
      const float ex = x1 - x0, ey = y1 - y0;
      const float sx = x0 + t0 * ex - ox, sy = y0 + t0 * ey - oy, fx = x0 + t1 * ex - ox, fy = y0 + t1 * ey - oy;
      acc += sx * fy - sy * fx;
    }
  }
  float f[4][4];                            // f[k][m]: corner m of Q against edge k of P (inside: > 0)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float ex = px[(k + 1) & 3] - px[k], ey = py[(k + 1) & 3] - py[k];
#pragma unroll
    for (int m = 0; m < 4; ++m) f[k][m] = ex * (qy[m] - py[k]) - ey * (qx[m] - px[k]);
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {             // Q's edges inside the open P
    float t0 = 0.f, t1 = 1.f;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) dd_clip_open(f[k][m], f[k][(m + 1) & 3], t0, t1, ok);
    if (ok && t1 > t0) {
      const float x0 = qx[m], y0 = qy[m], ex = qx[(m + 1) & 3] - x0, ey = qy[(m + 1) & 3] - y0;
      const float sx = x0 + t0 * ex - ox, sy = y0 + t0 * ey - oy, fx = x0 + t1 * ex - ox, fy = y0 + t1 * ey - oy;
      acc += sx * fy - sy * fx;
    }
  }
  const float inter = fminf(fmaxf(0.5f * acc, 0.f), fminf(areaP, areaQ));
  return inter / (areaP + areaQ - inter);
}

__device__ __forceinline__ int dd_row0(int c) { return 32 * c * (c + 1); }      // first matrix word of chunk c: 64 * (1 + ... + c)

__global__ __launch_bounds__(DEDUP_THREADS) void box_dedup_kernel(DedupParams p) {
  __shared__ unsigned long long s_m[DEDUP_WORDS];      // s_m[dd_row0(c) + j]: bit l = box j hits box 64 c + l
  __shared__ float s_cx[DEDUP_MAXK], s_cy[DEDUP_MAXK], s_hx[DEDUP_MAXK], s_hy[DEDUP_MAXK], s_cos[DEDUP_MAXK], s_sin[DEDUP_MAXK], s_rad[DEDUP_MAXK];
  __shared__ long s_lab[DEDUP_MAXK];
  __shared__ unsigned char s_act[DEDUP_MAXK];          // 1: a judgeable candidate
  __shared__ unsigned long long s_sup[DEDUP_WAVES];    // the suppressed boxes, one word per chunk
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long sb = blockIdx.x;
  const int K = p.Kdec, nch = (K + 63) >> 6;
  // ---- 1. records
  bool cand = false;
  {
    bool act = false;
    float cx = 0.f, cy = 0.f, hx = 0.f, hy = 0.f, cs = 1.f, sn = 0.f;
    long lab = 0;
    if (t < K) {
      const float* b = p.boxes + sb * p.s_box + (long)t * p.box_stride;
      const float sc = (p.scores + sb * p.s_score)[t];
      const float x = b[0], y = b[1], d3 = b[3], d4 = b[4], yaw = b[6];
      lab = (p.labels + sb * p.s_label)[t];
      cand = (p.keep + sb * p.s_keep)[t] != 0 && dd_finite(sc) && (double)sc >= p.score_thr;
      if (cand && dd_finite(x) && dd_finite(y) && dd_finite(d3) && dd_finite(d4) && dd_finite(yaw) && d3 > 0.f && d4 > 0.f) {
        act = true;
        cx = x; cy = y; hx = 0.5f * d3; hy = 0.5f * d4; cs = cosf(yaw); sn = sinf(yaw);
      }
    }
    s_cx[t] = cx; s_cy[t] = cy; s_hx[t] = hx; s_hy[t] = hy; s_cos[t] = cs; s_sin[t] = sn; s_rad[t] = sqrtf(hx * hx + hy * hy);
    s_lab[t] = lab;
    s_act[t] = act ? 1 : 0;
  }
  __syncthreads();
  // ---- 2. pairs
  float* ov = p.overlap ? p.overlap + sb * p.s_ov : nullptr;
  if (ov) {               // the entries no unit below reaches: row i, columns from the end of its own chunk
    const long n = (long)K * K;
    for (long e = t; e < n; e += DEDUP_THREADS) {
      const int i = (int)(e / K), j = (int)(e - (long)i * K);
      if (j >= 64 * ((i >> 6) + 1)) ov[e] = 0.f;
    }
  }
  for (int c = 0; c < nch; ++c) {
    const int i = 64 * c + lane, nj = min(K, 64 * (c + 1));
    const float cxi = s_cx[i], cyi = s_cy[i], hxi = s_hx[i], hyi = s_hy[i], ci = s_cos[i], si = s_sin[i], ri = s_rad[i];
    const long labi = s_lab[i];
    const bool acti = s_act[i] != 0;
    for (int j = wv; j < nj; j += DEDUP_WAVES) {
      bool hit = false;
      float o = 0.f;
      if (s_act[j] && acti && j < i && (!p.class_aware || s_lab[j] == labi)) {
        const float dx = cxi - s_cx[j], dy = cyi - s_cy[j];
        const float d2 = dx * dx + dy * dy;
        if (p.mode == 1) {
          o = d2;
          hit = o < p.thr;
        } else {
          const float rs = ri + s_rad[j];
          if (d2 <= rs * rs) {
            const float cj = s_cos[j], sj = s_sin[j];
            o = dd_iou_local(s_hx[j], s_hy[j], cj * dx + sj * dy, cj * dy - sj * dx, ci * cj + si * sj, si * cj - ci * sj, hxi, hyi);
            hit = o > p.thr;
          }
        }
      }
      const unsigned long long m = __ballot(hit);
      if (lane == 0) s_m[dd_row0(c) + j] = m;
      if (ov && i < K) ov[(long)i * K + j] = o;
    }
  }
  __syncthreads();
  // ---- 3. greedy, wave 0
  if (wv == 0) {
    for (int c = 0; c < nch; ++c) {
      const unsigned long long* row = s_m + dd_row0(c);
      unsigned long long acc = 0ull;
      for (int jb = 0; jb < c; ++jb) {
        const unsigned long long v = row[64 * jb + lane];
        acc |= ((s_sup[jb] >> lane) & 1ull) ? 0ull : v;
      }
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) acc |= __shfl_xor(acc, s);
      unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)acc), hi = __builtin_amdgcn_readfirstlane((unsigned)(acc >> 32));
      const int j = 64 * c + lane;
      const unsigned long long d = j < K ? row[j] : 0ull;
      const unsigned dlo = (unsigned)d, dhi = (unsigned)(d >> 32);
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        const unsigned rl = __builtin_amdgcn_readlane(dlo, k), rh = __builtin_amdgcn_readlane(dhi, k);
        if (!((lo >> k) & 1u)) { lo |= rl; hi |= rh; }
      }
#pragma unroll
      for (int k = 32; k < 64; ++k) {       // a row reaches only boxes behind it: the low word is final
        const unsigned rh = __builtin_amdgcn_readlane(dhi, k);
        if (!((hi >> (k - 32)) & 1u)) hi |= rh;
      }
      s_sup[c] = ((unsigned long long)hi << 32) | lo;      // every lane stores the same word and reads back its own store
    }
  }
  __syncthreads();
  // ---- 4. outputs
  if (wv < nch) {
    const bool sup = (s_sup[wv] >> lane) & 1ull;
    bool pending = sup;
    int of = -1;
    const unsigned long long* row = s_m + dd_row0(wv);
    const int nj = min(K, 64 * (wv + 1));
    for (int j = 0; j < nj; ++j) {
      if (__ballot(pending) == 0ull) break;
      const bool alive = !((s_sup[j >> 6] >> (j & 63)) & 1ull);
      if (pending && alive && ((row[j] >> lane) & 1ull)) {
        of = j;
        pending = false;
      }
    }
    if (t < K) {
      (p.dup_keep + sb * p.s_dk)[t] = (cand && !sup) ? 1 : 0;
      (p.dup_of + sb * p.s_of)[t] = of;
    }
  }
}

extern "C" int far3d_box_dedup(const float* boxes, const float* scores, const int64_t* labels, const unsigned char* keep,
                               unsigned char* dup_keep, int32_t* dup_of, float* overlap_out, int B, int Kdec, int box_stride, int mode,
                               int class_aware, double thr, double score_thr, const long* batch_strides, void* stream) {
  const char* who = "far3d_box_dedup";
  FAR3D_CHECK_ARG(batch_strides, "%s: batch_strides is a null pointer", who);
  FAR3D_CHECK_ARG(B >= 1 && B <= 65535, "%s: B=%d outside 1 .. 65535", who, B);
  FAR3D_CHECK_ARG(Kdec >= 0 && Kdec <= DEDUP_MAXK, "%s: Kdec=%d outside 0 .. %d", who, Kdec, DEDUP_MAXK);
  if (Kdec > 0) {
    FAR3D_CHECK_ARG(boxes, "%s: boxes is a null pointer (Kdec=%d)", who, Kdec);
    FAR3D_CHECK_ARG(scores, "%s: scores is a null pointer (Kdec=%d)", who, Kdec);
    FAR3D_CHECK_ARG(labels, "%s: labels is a null pointer (Kdec=%d)", who, Kdec);
    FAR3D_CHECK_ARG(keep, "%s: keep is a null pointer (Kdec=%d)", who, Kdec);
    FAR3D_CHECK_ARG(dup_keep, "%s: dup_keep is a null pointer (Kdec=%d)", who, Kdec);
    FAR3D_CHECK_ARG(dup_of, "%s: dup_of is a null pointer (Kdec=%d)", who, Kdec);
  }
  FAR3D_CHECK_ARG(box_stride >= 7, "%s: box_stride=%d is below the 7 floats (x, y, z, d3, d4, h, yaw) of a box", who, box_stride);
  FAR3D_CHECK_ARG(mode == 0 || mode == 1, "%s: mode=%d is neither 0 (iou_bev) nor 1 (centre)", who, mode);
  FAR3D_CHECK_ARG(thr == thr, "%s: thr is a NaN", who);
  if (mode == 0)
    FAR3D_CHECK_ARG(thr >= 0.0 && thr < 1.0, "%s: thr=%g outside [0, 1) of an IoU (mode 0)", who, thr);
  else
    FAR3D_CHECK_ARG(thr > 0.0 && thr - thr == 0.0, "%s: thr=%g is not a finite distance > 0 in metres (mode 1)", who, thr);
  FAR3D_CHECK_ARG(score_thr >= 0.0 && score_thr <= 1.0, "%s: score_thr=%g outside [0, 1]", who, score_thr);
  const long extent[7] = {(long)Kdec * box_stride, Kdec, Kdec, Kdec, Kdec, Kdec, (long)Kdec * Kdec};
  static const char* const names[7] = {"boxes", "scores", "labels", "keep", "dup_keep", "dup_of", "overlap_out"};
  for (int i = 0; i < 7; ++i)
    FAR3D_CHECK_ARG(B == 1 || (i == 6 && !overlap_out) || batch_strides[i] >= extent[i],
                    "%s: batch_strides[%d] (%s) = %ld elements is below one stream's %ld", who, i, names[i], batch_strides[i], extent[i]);
  if (Kdec == 0) return FAR3D_OK;
  DedupParams p;
  p.boxes = boxes; p.scores = scores; p.labels = (const long*)labels; p.keep = keep; p.dup_keep = dup_keep; p.dup_of = dup_of;
  p.overlap = overlap_out;
  p.s_box = batch_strides[0]; p.s_score = batch_strides[1]; p.s_label = batch_strides[2]; p.s_keep = batch_strides[3];
  p.s_dk = batch_strides[4]; p.s_of = batch_strides[5]; p.s_ov = batch_strides[6];
  p.Kdec = Kdec; p.box_stride = box_stride; p.mode = mode; p.class_aware = class_aware ? 1 : 0;
  p.thr = mode == 1 ? (float)(thr * thr) : (float)thr;
  p.score_thr = score_thr;
  hipLaunchKernelGGL(box_dedup_kernel, dim3(B), dim3(DEDUP_THREADS), 0, (hipStream_t)stream, p);
  FAR3D_CHECK_LAUNCH(who);
  return FAR3D_OK;
}
