// far3d_conv2d_nhwc: argument checks and tile dispatch; the kernels live in igemm_kernels.hpp (shared with igemm_pair.hip,
// which holds the instantiations for pair-stored activations so that the two halves compile in parallel).
#include "igemm_kernels.hpp"

int far3d_conv_pair_launch(const IgemmParams& P, int tile, hipStream_t st);   // igemm_pair.hip
int far3d_conv_f32_launch(const IgemmParams& P, int tile, hipStream_t st);    // igemm_pair.hip (fp32 rows on the pipelined GEMM kernel, tiles 479-494)
int far3d_pair_tile_caps(int tile);                                           // igemm_pair.hip (its rows of conv_tiles.hpp)
int far3d_gemm_ws_launch(const IgemmParams& P, int tile, hipStream_t st);     // conv_ws.hip (persistent wave-specialised 1x1 GEMM, tiles 460-476)
int far3d_conv_ws_launch(const IgemmParams& P, int tile, hipStream_t st);     // conv_ws.hip (persistent wave-specialised 3x3, tiles 400-459)
int far3d_ws_tile_caps(int tile);                                             // conv_ws.hip (its rows of conv_tiles.hpp)

// The plain-bf16 LDS-DMA rows of conv_tiles.hpp: -1 = no such tile
static int bf16_tile_caps(int tile) {
  switch (tile) {
    FAR3D_TILES_DMA(TILE_CAPS, IgemmDmaShape)
    FAR3D_TILES_GEMM(TILE_CAPS, Gemm1x1PipeShape)
    FAR3D_TILES_GEMM_WIDE(TILE_CAPS, Gemm1x1WideShape)
    FAR3D_TILES_GEMM_SPLIT(TILE_CAPS, Gemm1x1SplitShape)
    FAR3D_TILES_CONV3(TILE_CAPS, Conv3x3PipeShape)
    default: return -1;
  }
}

static int bf16_tile_launch(const IgemmParams& P, int tile, hipStream_t st) {
  switch (tile) {
    FAR3D_TILES_DMA(TILE_LAUNCH, launch_igemm_dma)
    FAR3D_TILES_GEMM(TILE_LAUNCH, launch_gemm1x1_pipe)
    FAR3D_TILES_GEMM_WIDE(TILE_LAUNCH, launch_gemm1x1_wide)
    FAR3D_TILES_GEMM_SPLIT(TILE_LAUNCH, launch_gemm1x1_split)
    FAR3D_TILES_CONV3(TILE_LAUNCH, launch_conv3x3_pipe)
    default: return FAR3D_ERR_ARG;      // not reached: the caller asked bf16_tile_caps first
  }
}

// Every id above 5 belongs to one family, so to one storage.
static int tile_row_caps(int tile) {
  int c = bf16_tile_caps(tile);
  if (c < 0) c = far3d_pair_tile_caps(tile);
  if (c < 0) c = far3d_ws_tile_caps(tile);
  return c;
}

// See include/far3d_hip.h.
extern "C" int far3d_conv_tile_caps(int tile, int x_dt, int w_dt) {
  const int store = x_dt == FAR3D_DT_BF16_PAIR ? (w_dt == FAR3D_DT_F32_BF16X3 ? FAR3D_TILE_PAIR : -1)
                    : x_dt == FAR3D_DT_BF16 ? (w_dt == FAR3D_DT_BF16 ? FAR3D_TILE_BF16 : -1)
                    : x_dt != FAR3D_DT_F32 ? -1
                    : w_dt == FAR3D_DT_F32 ? FAR3D_TILE_F32 : w_dt == FAR3D_DT_F32_BF16X3 ? FAR3D_TILE_F32_SPLIT : w_dt == FAR3D_DT_BF16 ? FAR3D_TILE_F32_BF16 : -1;
  if (store < 0) return -1;
  const int c = tile_row_caps(tile);
  if (c >= 0 && FAR3D_TILE_STORE(c) == store) return c;
  switch (tile) {      // the register-staged kernel takes every storage
#define TILE_CAPS_IGEMM(a, id, ...) case id: return IgemmShape<__VA_ARGS__>::caps | store << 2;
    FAR3D_TILES_IGEMM(TILE_CAPS_IGEMM, )
    default: return -1;
  }
}

// the end of every path of far3d_conv2d_nhwc: rc of the launcher, then the runtime's word on the launch
static int launched(int rc) {
  if (rc != FAR3D_OK) return rc;
  FAR3D_CHECK_LAUNCH("far3d_conv2d_nhwc");
  return FAR3D_OK;
}

#ifdef FAR3D_PROFILING
// tools/conv_phase_times.py: where the per-workgroup stamps of the pipelined conv / GEMM kernels go (8 x uint64 per workgroup)
static unsigned long long* g_conv_ts = nullptr;
extern "C" int far3d_prof_set_conv_timestamps(void* buf) { g_conv_ts = (unsigned long long*)buf; return 0; }
#endif

// See include/far3d_hip.h for the argument contract.
extern "C" int far3d_conv2d_nhwc(const void* x, int x_dt, const void* w, int w_dt, const float* bias, void* y,
                                 int y_dt, int N, int H, int W, int Cin, int ldx, long x_img_stride, int Ho,
                                 int Wo, int Cout, int ldy, long y_img_stride, int KH, int KW, int stride,
                                 int pad, int act, const void* res, int res_dt, int ldr, long res_img_stride,
                                 int Hr, int Wr, void* y2, int y2_dt, int ldy2, long y2_img_stride,
                                 const float* y2_scale, const float* y2_shift, long long* chan_sums, int tile, void* stream) {
  FAR3D_CHECK_ARG(x && w && y, "far3d_conv2d_nhwc: null x/w/y");
  FAR3D_CHECK_ARG(N > 0 && H > 0 && W > 0 && Cin > 0 && Ho > 0 && Wo > 0 && Cout > 0,
                  "far3d_conv2d_nhwc: bad sizes N=%d H=%d W=%d Cin=%d Ho=%d Wo=%d Cout=%d", N, H, W, Cin, Ho, Wo, Cout);
  FAR3D_CHECK_ARG(KH >= 1 && KW >= 1 && stride >= 1 && pad >= 0, "far3d_conv2d_nhwc: bad kernel geometry");
  FAR3D_CHECK_ARG((Ho - 1) * stride - pad + KH - 1 < H + pad + stride && (Wo - 1) * stride - pad + KW - 1 < W + pad + stride,
                  "far3d_conv2d_nhwc: output size %dx%d inconsistent with input %dx%d k=%d s=%d p=%d", Ho, Wo, H, W, KH, stride, pad);
  const bool pair_in = x_dt == FAR3D_DT_BF16_PAIR, pair_out = y_dt == FAR3D_DT_BF16_PAIR;
  FAR3D_CHECK_ARG(ldx >= Cin * (pair_in ? 2 : 1) && ldy >= Cout * (pair_out ? 2 : 1), "far3d_conv2d_nhwc: pixel strides smaller than channel counts");
  FAR3D_CHECK_ARG((x_dt == FAR3D_DT_F32 || x_dt == FAR3D_DT_BF16 || pair_in) &&
                  (w_dt == FAR3D_DT_F32 || w_dt == FAR3D_DT_BF16 || w_dt == FAR3D_DT_F32_BF16X3) &&
                  (y_dt == FAR3D_DT_F32 || y_dt == FAR3D_DT_BF16 || pair_out), "far3d_conv2d_nhwc: unsupported dtype");
  FAR3D_CHECK_ARG(pair_in ? (w_dt == FAR3D_DT_F32_BF16X3 && y_dt != FAR3D_DT_BF16 && Cin % 32 == 0) : !pair_out,
                  "far3d_conv2d_nhwc: pair-stored activations need split weights (w_dt 2), Cin %% 32 == 0 and a pair or f32 output; "
                  "pair outputs come from pair inputs");
  FAR3D_CHECK_ARG(!pair_out || Cout % 32 == 0, "far3d_conv2d_nhwc: pair-stored output needs Cout %% 32 == 0 (got %d)", Cout);
  FAR3D_CHECK_ARG(!(res && res_dt == FAR3D_DT_BF16_PAIR) || Cout % 32 == 0, "far3d_conv2d_nhwc: pair-stored residual needs Cout %% 32 == 0");
  FAR3D_CHECK_ARG(!(y2 && y2_dt == FAR3D_DT_BF16_PAIR), "far3d_conv2d_nhwc: the second output is f32 or bf16");
  FAR3D_CHECK_ARG(!(x_dt == FAR3D_DT_BF16 && w_dt != FAR3D_DT_BF16),
                  "far3d_conv2d_nhwc: bf16 activations with fp32 weights is not a supported combination");
  FAR3D_CHECK_ARG(act >= 0 && act <= 2, "far3d_conv2d_nhwc: unknown activation %d", act);
  FAR3D_CHECK_ARG(!y2 || (y2_scale && y2_shift), "far3d_conv2d_nhwc: y2 needs scale and shift");
  IgemmParams P;
  memset(&P, 0, sizeof(P));
  P.x = x; P.w = w; P.bias = bias; P.y = y; P.y2 = y2; P.y2_scale = y2_scale; P.y2_shift = y2_shift; P.res = res;
  P.x_img_stride = x_img_stride; P.y_img_stride = y_img_stride; P.y2_img_stride = y2_img_stride;
  P.res_img_stride = res_img_stride;
  P.N = N; P.H = H; P.W = W; P.Cin = Cin; P.ldx = ldx; P.Ho = Ho; P.Wo = Wo; P.Cout = Cout; P.ldy = ldy;
  P.KH = KH; P.KW = KW; P.stride = stride; P.pad = pad;
  P.cin_pad = (Cin + 31) / 32 * 32;
  P.nsteps = KH * KW * P.cin_pad / 32;
  P.act = act; P.y_dt = y_dt; P.y2_dt = y2_dt; P.ldy2 = ldy2;
  P.res_dt = res_dt; P.ldr = ldr; P.Hr = res ? Hr : Ho; P.Wr = res ? Wr : Wo;
  const int xe = x_dt == FAR3D_DT_F32 ? 4 : 2;
  const int ve = w_dt == FAR3D_DT_BF16 ? 8 : 4;  // elements per staged 16-byte chunk of the compute type
  auto aligned = [](const void* p, long a) { return ((uintptr_t)p % a) == 0; };
  P.x_vec = aligned(x, 16) && (ldx % ve == 0) && (x_img_stride % ve == 0) && (long)ve * xe % 16 == 0;
  P.y_vec = aligned(y, 16) && (ldy % 4 == 0) && (y_img_stride % 4 == 0);
  P.y2_vec = y2 && aligned(y2, 16) && (ldy2 % 4 == 0) && (y2_img_stride % 4 == 0);
  P.chan_sums = chan_sums; P.sums_hw = Ho * Wo;
#ifdef FAR3D_PROFILING
  P.prof = g_conv_ts;
#endif
  P.y_rows16 = (y_dt == FAR3D_DT_BF16 || pair_out) && !res && !y2 && aligned(y, 16) && (ldy % 8 == 0) && (y_img_stride % 8 == 0) && (Cout % 8 == 0);
  hipStream_t st = (hipStream_t)stream;
  const int caps = tile_row_caps(tile);       // -1: auto, ids 1-5, or no such tile
  const int store = caps < 0 ? -1 : FAR3D_TILE_STORE(caps);
  if (chan_sums) {       // only tiles with FAR3D_TILE_SUMS accumulate them (auto on a pair map is one: 179); anything else is an error, not a silent fallback
    const bool sums_tile = (pair_in && tile == 0) || (caps >= 0 && (caps & FAR3D_TILE_SUMS) && store == (pair_in ? FAR3D_TILE_PAIR : FAR3D_TILE_BF16));
    FAR3D_CHECK_ARG(KH == 1 && KW == 1 && stride == 1 && pad == 0 && sums_tile && (pair_in || (x_dt == FAR3D_DT_BF16 && Cin % 32 == 0 && P.x_vec)),
                    "far3d_conv2d_nhwc: channel sums need a 1x1 / stride 1 layer on a bf16 or pair-stored map and a tile that takes them "
                    "(far3d_conv_tile_caps: FAR3D_TILE_SUMS); got k=%d tile=%d", KH, tile);
  }
  if (caps >= 0 && (caps & FAR3D_TILE_PERSISTENT) && (caps & FAR3D_TILE_GEOM) == FAR3D_TILE_3X3 && !(caps & FAR3D_TILE_GROUPED)) {
    // persistent wave-specialised 3x3 kernel: a refusal is an error of the call, never a silent fallback
    const bool pair_tile = store == FAR3D_TILE_PAIR;
    FAR3D_CHECK_ARG(tile_geom_fits(caps, P) && !res && !y2 && !chan_sums && Cin % 32 == 0 && Cout % 32 == 0 &&
                    pair_tile == pair_in && (pair_in ? pair_out : (x_dt == FAR3D_DT_BF16 && w_dt == FAR3D_DT_BF16 && y_dt == FAR3D_DT_BF16)) &&
                    aligned(x, 16) && aligned(y, 16) && ldx % 8 == 0 && ldy % 8 == 0 && x_img_stride % 8 == 0 && y_img_stride % 8 == 0 &&
                    (long)N * H * W < (1L << 31) - 4096,
                    "far3d_conv2d_nhwc: tile %d (wave-specialised 3x3) needs a 3x3 / stride 1 / pad 1 layer, Cin and Cout multiples of 32, %s in and out, "
                    "16-byte aligned rows and no residual / second output / channel sums", tile, pair_tile ? "pair-stored" : "bf16");
    return launched(far3d_conv_ws_launch(P, tile, st));
  }
  if (caps >= 0 && (caps & FAR3D_TILE_PERSISTENT) && (caps & FAR3D_TILE_GEOM) == FAR3D_TILE_1X1) {
    // persistent wave-specialised 1x1 GEMM on pair-stored maps: a refusal is an error of the call
    FAR3D_CHECK_ARG(tile_geom_fits(caps, P) && !res && !y2 && Cin % 32 == 0 && Cout % 32 == 0 && pair_in && pair_out &&
                    aligned(x, 16) && aligned(y, 16) && ldx % 8 == 0 && ldy % 8 == 0 && x_img_stride % 8 == 0 && y_img_stride % 8 == 0 &&
                    (long)N * H * W < (1L << 31) - 4096 && ((long)(N - 1) * x_img_stride + (long)H * W * ldx) * 2 < 0x7fffffffL,
                    "far3d_conv2d_nhwc: tile %d (wave-specialised GEMM) needs a 1x1 / stride 1 layer on pair-stored maps, Cin and Cout multiples of 32, "
                    "16-byte aligned rows, an input map below 2 GB and no residual / second output", tile);
    return launched(far3d_gemm_ws_launch(P, tile, st));
  }
  if (pair_in) {
    FAR3D_CHECK_ARG(aligned(x, 16) && ldx % 8 == 0 && x_img_stride % 8 == 0 && (!pair_out || (aligned(y, 8) && ldy % 4 == 0 && y_img_stride % 4 == 0)),
                    "far3d_conv2d_nhwc: pair-stored tensors must be 16-byte aligned with pixel strides that are multiples of 8 elements");
    return launched(far3d_conv_pair_launch(P, tile, st));
  }
  const long Npix = (long)N * Ho * Wo;
  FAR3D_CHECK_ARG(Npix < (1L << 31) - 4096 && (long)N * H * W < (1L << 31) - 4096, "far3d_conv2d_nhwc: %ld pixels: the kernels index pixels with 32 bits", Npix);
  // fp32 activation rows on the pipelined GEMM kernel (1x1 only).  32 floats = the 128 bytes of a pair-stored 32-channel block: the rows
  // go in as pair rows of twice the stride.
  const bool f32_rows = x_dt == FAR3D_DT_F32 && KH == 1 && KW == 1 && stride == 1 && pad == 0 && Cin % 32 == 0 && !chan_sums &&
                        aligned(x, 16) && ldx % 4 == 0 && x_img_stride % 4 == 0 && ((long)(N - 1) * x_img_stride + (long)Ho * Wo * ldx) * 4 < 0x7fffffffL;
  IgemmParams Q = P;
  Q.ldx = 2 * ldx; Q.x_img_stride = 2 * x_img_stride;
  // x pre-split weights, in-register hi / lo split of the rows (tiles 479-481; auto); a layer that does not qualify takes the kernels below
  if (f32_rows && w_dt == FAR3D_DT_F32_BF16X3 && (tile == 0 || store == FAR3D_TILE_F32_SPLIT)) {
    // auto: the 64 x 64 tile (measured 7.3-10 us on the decoder's GEMMs against 11-18 for the 128 x 128 ones and 12-19 for the staged
    // exact-fp32 kernel, profiles/r5/fp32_rows_gemm.txt); the 8-wave 128 x 128 tile only when even that one fills the chip 8 times over
    const int t = tile ? tile : ((((Npix + 127) / 128) * ((Cout + 127) / 128) >= 2048) ? 479 : 480);
    return launched(far3d_conv_f32_launch(Q, t, st));
  }
  // x fp32 weights, explicit tiles 482-494: EXACT fp32 MFMA (far3d_amd.ops.linear picks them for the decoder-sized GEMMs; tile 0 keeps
  // the register-staged kernel, which takes every shape)
  if (store == FAR3D_TILE_F32) {
    FAR3D_CHECK_ARG(f32_rows && w_dt == FAR3D_DT_F32,
                    "far3d_conv2d_nhwc: tile %d (exact fp32 on the pipelined kernel) needs fp32 rows and fp32 weights, a 1x1 / stride 1 layer, Cin %% 32 == 0 "
                    "and 16-byte aligned rows", tile);
    return launched(far3d_conv_f32_launch(Q, tile, st));
  }
  if (tile == 0) tile = igemm_auto_tile(Npix, Cout);
  // plain bf16 with aligned rows: the LDS-DMA kernels, where the tile takes the layer's geometry
  if (x_dt == FAR3D_DT_BF16 && w_dt == FAR3D_DT_BF16 && (Cin % 32) == 0 && P.x_vec) {
    const int c = bf16_tile_caps(tile);
    if (c >= 0 && tile_geom_fits(c, P)) return launched(bf16_tile_launch(P, tile, st));
  }
  if (tile > 5) { far3d_set_error("far3d_conv2d_nhwc: tile %d needs the bf16 LDS-DMA path (Cin %% 32 == 0, aligned) and a layer of the tile's geometry", tile); return FAR3D_ERR_ARG; }
  // the register-staged kernel: 1 = 128x128, 2 = 64x128, 3 = 64x64, 4 = 128x64, 5 = 64x256 (channels x pixels)
  if (x_dt == FAR3D_DT_F32 && w_dt == FAR3D_DT_F32) return launched(launch_igemm_tile<float, float>(P, tile, st));
  if (x_dt == FAR3D_DT_F32 && w_dt == FAR3D_DT_F32_BF16X3) return launched(launch_igemm_tile<float, split_t>(P, tile, st));
  if (x_dt == FAR3D_DT_F32 && w_dt == FAR3D_DT_BF16) return launched(launch_igemm_tile<float, bf16_t>(P, tile, st));
  return launched(launch_igemm_tile<bf16_t, bf16_t>(P, tile, st));
}
