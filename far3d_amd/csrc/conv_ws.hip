// Instantiations of the persistent wave-specialised kernels (conv_ws.hpp): the FAR3D_TILES_WS_CONV3 rows (3x3, ids 400-459, and their grouped
// launches 5xx = 4xx + 100) and the FAR3D_TILES_WS_GEMM rows (1x1 GEMM on pair-stored maps, 460-476) of conv_tiles.hpp.
// Epilogue: bias + activation + pair / bf16 store only (no residual, no second output; 3x3: no channel sums): far3d_conv2d_nhwc refuses
// the tile for a layer that needs more.  A grouped launch adds the fp32 second output (camera-aware MLN) per problem.
#include "conv_ws.hpp"
#include "far3d_hip.h"

#ifdef FAR3D_PROFILING
std::atomic<int> g_ws_ablate{0};
extern "C" int far3d_conv_ws_set_ablate(int mask) { g_ws_ablate.store(mask); return 0; }     // probes only (see conv_ws.hpp)
#endif

// The mark of a FAR3D_TILES_WS_CONV3 row decides what `case id + 100` is: in the caps ...
#define WS_CAPS_SINGLE(id, ...) case id: return Conv3x3WsShape<__VA_ARGS__>::caps;
#define WS_CAPS_GROUPED(id, ...)                                                   \
  case id: return Conv3x3WsShape<__VA_ARGS__>::caps | FAR3D_TILE_HAS_GROUP;        \
  case id + 100: return Conv3x3WsShape<__VA_ARGS__>::caps | FAR3D_TILE_GROUPED;
#define WS_CAPS_GROUPED_PLAIN(id, ...) WS_CAPS_GROUPED(id, __VA_ARGS__)
#define WS_CAPS(a, id, mark, ...) WS_CAPS_##mark(id, __VA_ARGS__)
// ... and in the grouped dispatcher (the bool: may the grouped kernel defer its epilogue where the row does)
#define WS_GROUP_SINGLE(id, ...)
#define WS_GROUP_GROUPED(id, ...) case id + 100: return launch_conv3x3_ws_grouped<true, __VA_ARGS__>(P, G, st);
#define WS_GROUP_GROUPED_PLAIN(id, ...) case id + 100: return launch_conv3x3_ws_grouped<false, __VA_ARGS__>(P, G, st);
#define WS_GROUP(a, id, mark, ...) WS_GROUP_##mark(id, __VA_ARGS__)
#define WS_LAUNCH(a, id, mark, ...) case id: return launch_conv3x3_ws<__VA_ARGS__>(P, st);

int far3d_ws_tile_caps(int tile) {
  switch (tile) {
    FAR3D_TILES_WS_CONV3(WS_CAPS, )
    FAR3D_TILES_WS_GEMM(TILE_CAPS, Gemm1x1WsShape)
    default: return -1;
  }
}

int far3d_conv_ws_launch(const IgemmParams& P, int tile, hipStream_t st) {
  switch (tile) {
    FAR3D_TILES_WS_CONV3(WS_LAUNCH, )
    default: break;
  }
  far3d_set_error("far3d_conv2d_nhwc: unknown wave-specialised tile %d", tile);
  return FAR3D_ERR_ARG;
}

// The item dealing of a single-problem launch, for tests (include/far3d_hip.h): the inline function the kernel evaluates.
extern "C" int far3d_ws_deal(int n_full, int n_light, int grid, int wg, int k) {
  if (n_full < 0 || n_light < 0 || grid < 1 || wg < 0 || wg >= grid) return -1;
  return ws_deal_item(n_full, n_light, grid, wg, k);
}

int far3d_gemm_ws_launch(const IgemmParams& P, int tile, hipStream_t st) {
  switch (tile) {
    FAR3D_TILES_WS_GEMM(TILE_LAUNCH, launch_gemm1x1_ws)
    default: break;
  }
  far3d_set_error("far3d_conv2d_nhwc: unknown wave-specialised GEMM tile %d", tile);
  return FAR3D_ERR_ARG;
}

// Grouped launches: the marked rows, ids + 100
static int far3d_conv_ws_grouped_launch(const IgemmParams& P, const WsGroup& G, int tile, hipStream_t st) {
  switch (tile) {
    FAR3D_TILES_WS_CONV3(WS_GROUP, )
    default: break;
  }
  far3d_set_error("far3d_conv2d_nhwc_grouped: unknown grouped tile %d", tile);
  return FAR3D_ERR_ARG;
}

// See include/far3d_hip.h for the argument contract.  Every refusal is an error of the call: nothing is launched, nothing falls back.
extern "C" int far3d_conv2d_nhwc_grouped(const far3d_conv_problem* probs, int n, int tile, void* stream) {
  FAR3D_CHECK_ARG(probs && n >= 1 && n <= FAR3D_WS_GROUP_MAX, "far3d_conv2d_nhwc_grouped: %d problems (1..%d)", n, FAR3D_WS_GROUP_MAX);
  const int caps = far3d_ws_tile_caps(tile);
  FAR3D_CHECK_ARG(caps >= 0 && (caps & FAR3D_TILE_GROUPED), "far3d_conv2d_nhwc_grouped: tile %d is not a grouped tile (conv_tiles.hpp: 100 + a marked 4xx id)", tile);
  auto aligned = [](const void* p, long a) { return ((uintptr_t)p % a) == 0; };
  WsGroup G;
  memset(&G, 0, sizeof(G));
  G.n = n;
  const int Cin = probs[0].Cin;
  for (int i = 0; i < n; ++i) {
    const far3d_conv_problem& c = probs[i];
    FAR3D_CHECK_ARG(c.Cin == Cin, "far3d_conv2d_nhwc_grouped: problem %d has Cin %d, problem 0 has %d (one Cin per launch)", i, c.Cin, Cin);
    FAR3D_CHECK_ARG(c.x && c.w && c.y && c.N > 0 && c.H > 0 && c.W > 0 && c.Cout > 0 && Cin > 0 && Cin % 32 == 0 && c.Cout % 32 == 0 &&
                    c.act >= 0 && c.act <= 2 && c.ldx >= 2 * Cin && c.ldy >= 2 * c.Cout &&
                    aligned(c.x, 16) && aligned(c.y, 16) && c.ldx % 8 == 0 && c.ldy % 8 == 0 && c.x_img_stride % 8 == 0 && c.y_img_stride % 8 == 0 &&
                    (long)c.N * c.H * c.W < (1L << 31) - 4096 && (long)c.H * c.W * c.ldx * 2 < 0x7fffffffL,
                    "far3d_conv2d_nhwc_grouped: problem %d: needs pair-stored maps in and out, Cin and Cout multiples of 32, 16-byte aligned rows "
                    "(N=%d H=%d W=%d Cin=%d Cout=%d ldx=%d ldy=%d act=%d)", i, c.N, c.H, c.W, c.Cin, c.Cout, c.ldx, c.ldy, c.act);
    FAR3D_CHECK_ARG(!c.y2 || (c.y2_scale && c.y2_shift && aligned(c.y2, 16) && aligned(c.y2_scale, 16) && aligned(c.y2_shift, 16) &&
                              c.ldy2 >= c.Cout && c.ldy2 % 4 == 0 && c.y2_img_stride % 4 == 0),
                    "far3d_conv2d_nhwc_grouped: problem %d: the second output is fp32 with 16-byte aligned rows, scale and shift", i);
    WsProblem& q = G.p[i];
    q.x = c.x; q.w = c.w; q.bias = c.bias; q.y = c.y;
    q.y2 = c.y2; q.y2_scale = c.y2_scale; q.y2_shift = c.y2_shift;
    q.x_img_stride = c.x_img_stride; q.y_img_stride = c.y_img_stride; q.y2_img_stride = c.y2_img_stride;
    q.N = c.N; q.H = c.H; q.W = c.W; q.ldx = c.ldx; q.ldy = c.ldy; q.ldy2 = c.ldy2; q.Cout = c.Cout; q.act = c.act;
  }
  IgemmParams P;
  memset(&P, 0, sizeof(P));
  const far3d_conv_problem& c0 = probs[0];
  P.x = c0.x; P.w = c0.w; P.bias = c0.bias; P.y = c0.y;
  P.x_img_stride = c0.x_img_stride; P.y_img_stride = c0.y_img_stride;
  P.N = c0.N; P.H = c0.H; P.W = c0.W; P.Cin = Cin; P.ldx = c0.ldx; P.Ho = c0.H; P.Wo = c0.W; P.Cout = c0.Cout; P.ldy = c0.ldy;
  P.KH = 3; P.KW = 3; P.stride = 1; P.pad = 1;
  P.cin_pad = Cin; P.nsteps = 9 * Cin / 32;
  P.act = c0.act; P.y_dt = FAR3D_DT_BF16_PAIR;
  const int rc = far3d_conv_ws_grouped_launch(P, G, tile, (hipStream_t)stream);
  if (rc != FAR3D_OK) return rc;
  FAR3D_CHECK_LAUNCH("far3d_conv2d_nhwc_grouped");
  return FAR3D_OK;
}
