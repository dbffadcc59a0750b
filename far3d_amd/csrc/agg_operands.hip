// far3d_agg_operands / far3d_camera_sum -- the aggregation through the reference's own MSDA operands (gfx950).
//
// DeformableFeatureAggregationCuda (reference models/utils/detr3d_transformer.py:522-569) builds two tensors and hands them to the MSDA
// operator: the projected key points `points_2d` (:547-555) and the softmax weights (:535-542).  The fused kernel of sampling.hip never
// materialises them and is built for one shape family.  This file is the second, general statement of the same arithmetic:
//   far3d_agg_operands  ->  far3d_msda_forward (bs = B*N, any H / Dh / L / P)  ->  far3d_camera_sum
// for every shape and batch size the reference class accepts, with the two operands as a public output in the reference's layout.
// It is a fallback and an inspection path (about 3 * B*N*A*L*P*G floats of operands go through HBM), never the default for the family
// the fused kernel covers.  Nothing here touches sampling.hip.
#include "common.hpp"
#include <math.h>

#define AGGOP_THREADS 256
#define AGGOP_MAX_N 32
#define AGGOP_MAX_L 8
#define AGGOP_MAX_P 64
#define AGGOP_MAX_G 64
#define AGGOP_MAX_NLP 8192
#define AGGOP_STAGE_J 16384     // up to this many weights per camera the run is transposed in LDS and leaves as one contiguous store
// aggop_group_reduce combines AGGOP_THREADS / 64 wave results (or up to AGGOP_THREADS partials) through AGGOP_THREADS floats of LDS, and for a
// power-of-two G <= 64 relies on AGGOP_THREADS % G == 0 so that every lane of every wave takes part in the shuffles
static_assert(AGGOP_THREADS == 256 && AGGOP_THREADS % 64 == 0 && AGGOP_MAX_G <= 64, "aggop_group_reduce is written for four wave64s and G <= 64");
// Dynamic LDS in floats: the U row [J] + the transposed run [J, staged only] + (u, v) [N*P*2] + the reduction scratch.  The largest request
// any accepted shape can make; the per-kernel limit is raised to THIS value (not to a call's own size, which grows between calls).
constexpr int aggop_max(int a, int b) { return a > b ? a : b; }
constexpr int AGGOP_MAX_LDS_FLOATS = aggop_max(2 * AGGOP_STAGE_J, AGGOP_MAX_L * AGGOP_MAX_P * AGGOP_MAX_G) + 2 * AGGOP_MAX_N * AGGOP_MAX_P + AGGOP_THREADS;
constexpr int AGGOP_MAX_LDS = AGGOP_MAX_LDS_FLOATS * (int)sizeof(float);
static_assert(AGGOP_MAX_LDS <= 160 * 1024, "far3d_agg_operands: the accepted sizes must fit the 160 KiB of LDS of a gfx950 CU");

struct AggOpParams {
  int A, N, G, P, L;
  int J, LP;                // J = L*P*G logits per camera, LP = L*P
  int ldU, ldO;             // row strides (floats) of U and of the key-point offsets
  int expand;               // 1: loc (B*N,A,G,L,P,2); 0: loc (B*N,A,P,2)
  int vecU, vecW, vecL;     // 16-byte accesses are possible for the U rows / the weight runs / the location runs
  int staged;               // weight runs go through the LDS transpose
  int pow2;                 // G is a power of two: the group reductions start with wave shuffles
  int R;                    // rows of the thread grid: thread t works on group t % G, row t / G (R = 256 / G)
  float pc_lo[3], pc_span[3];
  float pad_w, pad_h;
};

// Max or sum of one value per thread over the threads of the same group g = t % G.  pow2: 64 % G == 0, so a wave's lanes of one group are
// a xor-orbit (offsets 32 .. G) and the 4 waves' results are combined in wave order; else the R*G partials go through LDS and are combined in
// row order.  Every thread returns the same bits for its group, whatever B or the launch: the order is a function of (G, t) alone.
template <bool IS_MAX>
__device__ __forceinline__ float aggop_group_reduce(float v, int t, int g, const AggOpParams& prm, float* red) {
  int rows;
  if (prm.pow2) {
    for (int off = 32; off >= prm.G; off >>= 1) {
      const float o = __shfl_xor(v, off, 64);
      v = IS_MAX ? fmaxf(v, o) : v + o;
    }
    if ((t & 63) < prm.G) red[(t >> 6) * prm.G + (t & 63)] = v;
    rows = AGGOP_THREADS / 64;
  } else {
    if (t < prm.R * prm.G) red[t] = v;
    rows = prm.R;
  }
  __syncthreads();
  float r = red[g];
  for (int i = 1; i < rows; ++i) {
    const float o = red[i * prm.G + g];
    r = IS_MAX ? fmaxf(r, o) : r + o;
  }
  __syncthreads();      // red is written again by the next reduction
  return r;
}

// One workgroup per (b, a).  LDS: U row [J] | weight run of one camera, transposed [J, staged only] | (u, v) of every (camera, point)
// [N*P*2] | reduction scratch [AGGOP_THREADS].
__global__ __launch_bounds__(AGGOP_THREADS) void agg_operands_kernel(const float* __restrict__ ref, const float* __restrict__ offsets,
                                                                     const float* __restrict__ l2i, const float* __restrict__ U,
                                                                     const float* __restrict__ Vc, float* __restrict__ loc,
                                                                     float* __restrict__ weights, float* __restrict__ key_points,
                                                                     const AggOpParams prm) {
  extern __shared__ __attribute__((aligned(16))) float aggop_lds[];
  const int t = threadIdx.x;
  const int N = prm.N, G = prm.G, P = prm.P, J = prm.J, LP = prm.LP, R = prm.R;
  const long row = blockIdx.x;                 // b * A + a
  const int b = (int)(row / prm.A), a = (int)(row - (long)b * prm.A);
  float* Us = aggop_lds;
  float* Ts = Us + J;
  float* uv = Ts + (prm.staged ? J : 0);
  float* red = uv + N * P * 2;

  // ---- the U row, once
  const float* Urow = U + row * prm.ldU;
  if (prm.vecU) {
    for (int i = t; i < J / 4; i += AGGOP_THREADS) reinterpret_cast<float4*>(Us)[i] = reinterpret_cast<const float4*>(Urow)[i];
  } else {
    for (int i = t; i < J; i += AGGOP_THREADS) Us[i] = Urow[i];
  }

  // ---- key points and their projection into every camera (reference :524-525, :547-552); fp32, true divisions
  for (int i = t; i < N * P; i += AGGOP_THREADS) {
    const int n = i / P, p = i - n * P;
    const float* o = offsets + row * prm.ldO + p * 3;
    const float* r3 = ref + row * 3;
    const float kx = (r3[0] * prm.pc_span[0] + prm.pc_lo[0]) + o[0];
    const float ky = (r3[1] * prm.pc_span[1] + prm.pc_lo[1]) + o[1];
    const float kz = (r3[2] * prm.pc_span[2] + prm.pc_lo[2]) + o[2];
    if (n == 0 && key_points) {
      float* kp = key_points + (row * P + p) * 3;
      kp[0] = kx; kp[1] = ky; kp[2] = kz;
    }
    const float* m = l2i + ((long)b * N + n) * 16;
    const float x = m[0] * kx + m[1] * ky + m[2] * kz + m[3];
    const float y = m[4] * kx + m[5] * ky + m[6] * kz + m[7];
    const float z = m[8] * kx + m[9] * ky + m[10] * kz + m[11];
    const float zc = fmaxf(z, 1e-5f);
    uv[2 * i] = (x / zc) / prm.pad_w;
    uv[2 * i + 1] = (y / zc) / prm.pad_h;
  }
  __syncthreads();

  // ---- locations: per camera one contiguous run, the P points repeated for every (group, level) (reference :555)
  {
    const int run = prm.expand ? 2 * J : 2 * P, P2 = 2 * P;
    for (int n = 0; n < N; ++n) {
      float* dst = loc + (((long)b * N + n) * prm.A + a) * run;
      const float* src = uv + n * P2;
      if (prm.vecL) {
        for (int i = t * 4; i < run; i += AGGOP_THREADS * 4) {
          int e = i % P2;
          float4 v;
          v.x = src[e]; e = e + 1 == P2 ? 0 : e + 1;
          v.y = src[e]; e = e + 1 == P2 ? 0 : e + 1;
          v.z = src[e]; e = e + 1 == P2 ? 0 : e + 1;
          v.w = src[e];
          *reinterpret_cast<float4*>(dst + i) = v;
        }
      } else {
        for (int i = t; i < run; i += AGGOP_THREADS) dst[i] = src[i % P2];
      }
    }
  }

  // ---- softmax over the N*L*P logits U[a][j] + Vc[n][j] of every group (reference :539-540): max, sum of expf in a fixed order, division
  const int g = t % G, r0 = t / G;
  const bool active = t < R * G;
  const float* Vb = Vc + (long)b * N * J;
  float mx = -INFINITY;
  if (active)
    for (int lp = r0; lp < LP; lp += R) {
      const int j = lp * G + g;
      const float u = Us[j];
      for (int n = 0; n < N; ++n) mx = fmaxf(mx, u + Vb[(long)n * J + j]);
    }
  mx = aggop_group_reduce<true>(mx, t, g, prm, red);
  float sum = 0.f;
  if (active)
    for (int lp = r0; lp < LP; lp += R) {
      const int j = lp * G + g;
      const float u = Us[j];
      for (int n = 0; n < N; ++n) sum += expf((u + Vb[(long)n * J + j]) - mx);
    }
  sum = aggop_group_reduce<false>(sum, t, g, prm, red);

  // ---- weights (B*N, A, G, L*P): the camera's run is transposed from (l*P+p, g) to (g, l*P+p) in LDS and stored contiguously
  for (int n = 0; n < N; ++n) {
    float* dst = weights + (((long)b * N + n) * prm.A + a) * J;
    float* wout = prm.staged ? Ts : dst;
    if (active)
      for (int lp = r0; lp < LP; lp += R) {
        const int j = lp * G + g;
        wout[g * LP + lp] = expf((Us[j] + Vb[(long)n * J + j]) - mx) / sum;
      }
    if (prm.staged) {
      __syncthreads();
      if (prm.vecW) {
        for (int i = t; i < J / 4; i += AGGOP_THREADS) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(Ts)[i];
      } else {
        for (int i = t; i < J; i += AGGOP_THREADS) dst[i] = Ts[i];
      }
      __syncthreads();
    }
  }
}

extern "C" int far3d_agg_operands(const float* ref, const float* offsets, const float* lidar2img, const float* U, const float* Vc,
                                  float* loc, float* weights, float* key_points, int B, int A, int N, int G, int P, int L,
                                  const float* pc_range, float pad_h, float pad_w, int ldU, int ldOffs, int expand, void* stream) {
  FAR3D_CHECK_ARG(B >= 0 && A >= 0 && N >= 1 && N <= AGGOP_MAX_N && L >= 1 && L <= AGGOP_MAX_L && P >= 1 && P <= AGGOP_MAX_P && G >= 1 &&
                  G <= AGGOP_MAX_G && (long)N * L * P <= AGGOP_MAX_NLP,
                  "far3d_agg_operands: sizes out of range: B=%d A=%d N=%d (1..%d) L=%d (1..%d) P=%d (1..%d) G=%d (1..%d) N*L*P=%ld (<= %d)",
                  B, A, N, AGGOP_MAX_N, L, AGGOP_MAX_L, P, AGGOP_MAX_P, G, AGGOP_MAX_G, (long)N * L * P, AGGOP_MAX_NLP);
  FAR3D_CHECK_ARG(pc_range, "far3d_agg_operands: null pc_range");
  AggOpParams prm;
  prm.A = A; prm.N = N; prm.G = G; prm.P = P; prm.L = L;
  prm.LP = L * P; prm.J = L * P * G;
  prm.ldU = ldU > 0 ? ldU : prm.J;
  prm.ldO = ldOffs > 0 ? ldOffs : P * 3;
  FAR3D_CHECK_ARG(prm.ldU >= prm.J && prm.ldO >= P * 3 && (long)B * A < (1L << 31),
                  "far3d_agg_operands: row strides ldU=%d (>= %d) / ldOffs=%d (>= %d) or B*A=%ld (< 2^31) out of range", prm.ldU, prm.J, prm.ldO,
                  P * 3, (long)B * A);
  if ((long)B * A == 0) return FAR3D_OK;
  FAR3D_CHECK_ARG(ref && offsets && lidar2img && U && Vc && loc && weights, "far3d_agg_operands: null pointer argument");
  prm.expand = expand ? 1 : 0;
  auto al = [](const void* p) { return ((uintptr_t)p % 16) == 0; };
  prm.vecU = prm.J % 4 == 0 && prm.ldU % 4 == 0 && al(U);
  prm.vecW = prm.J % 4 == 0 && al(weights);
  prm.vecL = (prm.expand ? 2 * prm.J : 2 * P) % 4 == 0 && al(loc);
  prm.staged = prm.J <= AGGOP_STAGE_J;
  prm.pow2 = (G & (G - 1)) == 0;
  prm.R = AGGOP_THREADS / G;
  for (int d = 0; d < 3; ++d) { prm.pc_lo[d] = pc_range[d]; prm.pc_span[d] = pc_range[3 + d] - pc_range[d]; }
  prm.pad_w = pad_w; prm.pad_h = pad_h;
  const int lds = (int)sizeof(float) * (prm.J * (prm.staged ? 2 : 1) + N * P * 2 + AGGOP_THREADS);
  FAR3D_CHECK_ARG(lds <= AGGOP_MAX_LDS, "far3d_agg_operands: %d bytes of LDS for N=%d L=%d P=%d G=%d exceed the kernel's %d", lds, N, L, P, G,
                  AGGOP_MAX_LDS);
  if (lds > 64 * 1024) {      // allowed once per device, for the largest request of any accepted shape
    static std::atomic<unsigned long long> lds_ok{0};
    const int e = far3d_allow_lds((const void*)agg_operands_kernel, AGGOP_MAX_LDS, lds_ok, "far3d_agg_operands");
    if (e != FAR3D_OK) return e;
  }
  hipLaunchKernelGGL(agg_operands_kernel, dim3((unsigned)((long)B * A)), dim3(AGGOP_THREADS), lds, (hipStream_t)stream, ref, offsets, lidar2img,
                     U, Vc, loc, weights, key_points, prm);
  FAR3D_CHECK_LAUNCH("far3d_agg_operands");
  return FAR3D_OK;
}

// x (B*N, A, C) -> out (B, A, C): cameras added in ascending order, ((x0 + x1) + x2) + ...  One streaming pass, 16 bytes per lane.
template <typename V>
__global__ __launch_bounds__(256) void camera_sum_kernel(const V* __restrict__ x, V* __restrict__ out, int N, long per, long total) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / per, e = i - b * per;
    const V* p = x + b * N * per + e;
    V acc = p[0];
    for (int n = 1; n < N; ++n) {
      const V v = p[(long)n * per];
      if constexpr (sizeof(V) == 16) { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
      else acc += v;
    }
    out[i] = acc;
  }
}

extern "C" int far3d_camera_sum(const float* x, float* out, int B, int N, int A, int C, void* stream) {
  FAR3D_CHECK_ARG(B >= 0 && N >= 1 && A >= 0 && C >= 1, "far3d_camera_sum: bad sizes B=%d N=%d A=%d C=%d", B, N, A, C);
  const long per = (long)A * C;
  if ((long)B * per == 0) return FAR3D_OK;
  FAR3D_CHECK_ARG(x && out, "far3d_camera_sum: null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = per % 4 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0;
  const long unit = vec ? per / 4 : per, total = (long)B * unit;
  long blocks = (total + 255) / 256;
  if (blocks > 256L * 16) blocks = 256L * 16;
  if (vec)
    hipLaunchKernelGGL(camera_sum_kernel<float4>, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<const float4*>(x),
                       reinterpret_cast<float4*>(out), N, unit, total);
  else
    hipLaunchKernelGGL(camera_sum_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, x, out, N, unit, total);
  FAR3D_CHECK_LAUNCH("far3d_camera_sum");
  return FAR3D_OK;
}
