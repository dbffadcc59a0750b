// Instantiations of the conv / GEMM kernels for pair-stored activations (FAR3D_DT_BF16_PAIR, common.hpp): the fast path of the
// "bf16x3" precision mode -- and of the same GEMM kernel on fp32 activation rows.  Separate translation unit so that it compiles in
// parallel with igemm.hip.  The tiles are the FAR3D_TILES_IGEMM (with pair types), _PAIR_* and _F32_GEMM lists of conv_tiles.hpp.
#include "igemm_kernels.hpp"

int far3d_pair_tile_caps(int tile) {
  switch (tile) {
    FAR3D_TILES_PAIR_GEMM(TILE_CAPS, Gemm1x1PipeShape)
    FAR3D_TILES_PAIR_CONV3(TILE_CAPS, Conv3x3PipeShape)
    FAR3D_TILES_F32_GEMM(TILE_CAPS, Gemm1x1PipeShape)
    default: return -1;
  }
}

int far3d_conv_pair_launch(const IgemmParams& P, int tile, hipStream_t st) {
  if (tile == 0) {    // 3x3 / 1x1 stride 1: the library defaults; strided / odd kernels: the heuristic of the register-staged kernel
    tile = tile_geom_fits(FAR3D_TILE_3X3, P) ? 160 : tile_geom_fits(FAR3D_TILE_1X1, P) ? 179 : igemm_auto_tile((long)P.N * P.Ho * P.Wo, P.Cout);
  }
  if (tile <= 5) return launch_igemm_tile<pair_t, split_t>(P, tile, st);
  const int caps = far3d_pair_tile_caps(tile);
  if (caps >= 0 && FAR3D_TILE_STORE(caps) == FAR3D_TILE_PAIR && tile_geom_fits(caps, P)) {
    switch (tile) {
      FAR3D_TILES_PAIR_GEMM(TILE_LAUNCH, launch_gemm1x1_pipe)
      FAR3D_TILES_PAIR_CONV3(TILE_LAUNCH, launch_conv3x3_pipe)
      default: break;
    }
  }
  far3d_set_error("far3d_conv2d_nhwc: tile %d is not available for pair-stored activations with k=%d stride=%d", tile, P.KH, P.stride);
  return FAR3D_ERR_ARG;
}

// fp32 activation rows on the pipelined GEMM kernel (the caller has doubled P.ldx and P.x_img_stride and checked the storage of the tile)
int far3d_conv_f32_launch(const IgemmParams& P, int tile, hipStream_t st) {
  switch (tile) {
    FAR3D_TILES_F32_GEMM(TILE_LAUNCH, launch_gemm1x1_pipe)
    default: break;
  }
  far3d_set_error("far3d_conv2d_nhwc: tile %d is not available for fp32 activation rows", tile);
  return FAR3D_ERR_ARG;
}
