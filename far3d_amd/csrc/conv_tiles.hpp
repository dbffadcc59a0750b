// The table of far3d_conv2d_nhwc's tiles: ONE row per tile id, X(a, id, template arguments of the family's launcher) and the shape in
// words, in one list per kernel family.  Everything that has to know a tile expands these lists:
//   * the dispatchers: FAR3D_TILES_GEMM(TILE_LAUNCH, launch_gemm1x1_pipe) is the `case id: return launch_gemm1x1_pipe<...>(P, st);`
//     lines of a switch; each translation unit expands the families it owns, so it instantiates exactly its own kernels;
//   * far3d_conv_tile_caps (include/far3d_hip.h): FAR3D_TILES_GEMM(TILE_CAPS, Gemm1x1PipeShape) asks the launcher's constexpr shape
//     description (igemm_kernels.hpp, conv_ws.hpp) -- geometry, storage, channel sums and pixels per tile are computed from the
//     template arguments, never restated.  far3d_amd/ops.py, the tuner and the tests ask that export.
// A new tile is one row here (plus its id in the tests' lists).
//
// How the ids relate (separate rows where the pair rows carry NT / PAIR arguments the bf16 rows do not have):
//   pair id = bf16 id + 100 (split products, NT = 3): 3x3 150-198 are 50-98, 1x1 170-181 are 70-81; 330 / 331 3x3 stride 2;
//   hi planes only (NT = 1) = pair id + 100: 252, 260, 265, 279, 280;
//   fp32 rows x split weights 479-481 = the pair GEMMs 179-181 + 300; 482-494 exact fp32 on the same kernel;
//   grouped launch (far3d_conv2d_nhwc_grouped) = persistent 3x3 id + 100, derived from the mark on the 4xx row (FAR3D_TILES_WS_CONV3).
#pragma once

#define TILE_LAUNCH(fn, id, ...) case id: return fn<__VA_ARGS__>(P, st);
#define TILE_CAPS(shape, id, ...) case id: return shape<__VA_ARGS__>::caps;

// ---- igemm.hip and igemm_pair.hip: register-staged kernel, ANY storage, kernel size and stride (launch_igemm<TIn, TC, WGM, WGN, WM, WN>:
// the dispatcher supplies the two types); channels x pixels
#define FAR3D_TILES_IGEMM(X, a)                                                                                                                       \
  X(a, 1, 2, 2, 2, 2)                                           /* 128 x 128 */                                                                       \
  X(a, 2, 2, 2, 1, 2)                                           /* 64 x 128 */                                                                        \
  X(a, 3, 2, 2, 1, 1)                                           /* 64 x 64 */                                                                         \
  X(a, 4, 2, 2, 2, 1)                                           /* 128 x 64 */                                                                        \
  X(a, 5, 1, 4, 2, 2)                                           /* 64 x 256 */

// ---- igemm.hip: plain bf16, Cin % 32 == 0 (LDS-DMA)
// launch_igemm_dma<WGM, WGN, WM, WN, NS[, KPS]>.  On a bf16 layer ids 1-4 mean these rows; unaligned rows take the register-staged kernel.
// global_load_lds ring kernel (any kernel size / stride): (channels x pixels, ring depth) 1 128x128/3  2 64x128/4  3 64x64/4
// 4 128x64/4; 5 falls back to the register-staged 64x256
#define FAR3D_TILES_DMA(X, a)                                                                                                                         \
  X(a, 1, 2, 2, 2, 2, 3)                                                                                                                              \
  X(a, 2, 2, 2, 1, 2, 4)                                                                                                                              \
  X(a, 3, 2, 2, 1, 1, 4)                                                                                                                              \
  X(a, 4, 2, 2, 2, 1, 4)                                                                                                                              \
  /* several 32-channel K chunks per barrier step */                                                                                                  \
  X(a, 18, 2, 2, 1, 1, 3, 3)                                    /* 64x64, 3 chunks/step */                                                            \
  /* 2-deep rings: less LDS -> more resident workgroups per CU */                                                                                     \
  X(a, 43, 2, 2, 2, 2, 2)                                       /* 128x128 */                                                                         \
  X(a, 46, 2, 2, 2, 1, 2)                                       /* 128x64 */                                                                          \
  X(a, 48, 2, 2, 1, 1, 2)                                       /* 64x64 */

// launch_gemm1x1_pipe<WGM, WGN, WM, WN[, NT, PAIR, NS]>: pipelined 1x1 / stride 1 GEMM (channels x pixels, waves)
#define FAR3D_TILES_GEMM(X, a)                                                                                                                        \
  X(a, 70, 2, 2, 2, 2)                                          /* 128 x 128, 4 waves */                                                              \
  X(a, 71, 2, 4, 2, 1)                                          /* 128 x 128, 8 waves */                                                              \
  X(a, 72, 2, 4, 2, 2)                                          /* 128 x 256, 8 waves */                                                              \
  X(a, 73, 4, 2, 2, 2)                                          /* 256 x 128, 8 waves */                                                              \
  X(a, 74, 2, 2, 1, 2)                                          /* 64 x 128, 4 waves */                                                               \
  X(a, 75, 2, 4, 1, 1)                                          /* 64 x 128, 8 waves */                                                               \
  X(a, 76, 2, 2, 2, 1)                                          /* 128 x 64, 4 waves */                                                               \
  X(a, 77, 4, 4, 2, 1)                                          /* 256 x 128, 16 waves */                                                             \
  X(a, 78, 2, 4, 1, 2)                                          /* 64 x 256, 8 waves */                                                               \
  X(a, 79, 4, 2, 1, 2)                                          /* 128 x 128, 8 waves (1x2 tiles per wave) */                                         \
  X(a, 80, 2, 2, 1, 1)                                          /* 64 x 64, 4 waves */                                                                \
  X(a, 81, 4, 4, 1, 1)                                          /* 128 x 128, 16 waves */                                                             \
  /* deeper LDS rings (NS - 1 steps of 64 channels in flight, counted vmcnt) */                                                                       \
  X(a, 82, 4, 2, 1, 2, 1, false, 3)                             /* 128 x 128, 8 waves, 3 stages */                                                    \
  X(a, 83, 2, 2, 1, 2, 1, false, 3)                             /* 64 x 128, 4 waves, 3 stages */                                                     \
  X(a, 84, 2, 2, 2, 2, 1, false, 3)                             /* 128 x 128, 4 waves, 3 stages */                                                    \
  X(a, 85, 4, 2, 2, 2, 1, false, 3)                             /* 256 x 128, 8 waves, 3 stages */                                                    \
  X(a, 86, 2, 2, 1, 2, 1, false, 4)                             /* 64 x 128, 4 waves, 4 stages */                                                     \
  X(a, 87, 2, 2, 1, 1, 1, false, 4)                             /* 64 x 64, 4 waves, 4 stages */                                                      \
  X(a, 88, 2, 2, 1, 1, 1, false, 3)                             /* 64 x 64, 4 waves, 3 stages */                                                      \
  X(a, 89, 2, 2, 2, 1, 1, false, 3)                             /* 128 x 64, 4 waves, 3 stages */                                                     \
  /* 256 x 256 tiles: half the L2 -> LDS bytes per MFMA of the 128 x 128 tiles (the GEMMs are fill-bound) */                           \
  X(a, 110, 4, 2, 2, 4)                                         /* 8 waves of 64 ch x 128 px */                                                       \
  X(a, 111, 2, 4, 4, 2)                                         /* 8 waves of 128 ch x 64 px */                                                       \
  X(a, 112, 4, 4, 2, 2)                                         /* 16 waves of 64 x 64 */                                                             \
  X(a, 113, 2, 2, 4, 4)                                         /* 4 waves of 128 x 128 */                                                            \
  X(a, 114, 2, 4, 2, 4)                                         /* 128 ch x 512 px, 8 waves of 64 x 128 */                                            \
  X(a, 115, 4, 2, 4, 2)                                         /* 512 ch x 128 px */                                                                 \
  X(a, 116, 2, 4, 4, 1)                                         /* 256 ch x 128 px, 8 waves of 128 x 32 */                                            \
  X(a, 117, 4, 2, 1, 4)                                         /* 128 ch x 256 px, 8 waves of 32 x 128 */

// full-line DMA pieces (8 rows x 128 B per instruction, 128-byte LDS rows)
// launch_gemm1x1_wide<WGM, WGN, WM, WN[, NS]>
#define FAR3D_TILES_GEMM_WIDE(X, a)                                                                                                                   \
  X(a, 120, 4, 2, 1, 2)                                         /* 128 x 128, 8 waves */                                                              \
  X(a, 121, 2, 2, 2, 2)                                         /* 128 x 128, 4 waves */                                                              \
  X(a, 122, 4, 2, 2, 2)                                         /* 256 x 128, 8 waves */                                                              \
  X(a, 123, 4, 2, 2, 4)                                         /* 256 x 256, 8 waves */                                                              \
  X(a, 124, 2, 2, 1, 2)                                         /* 64 x 128, 4 waves */                                                               \
  X(a, 125, 2, 2, 1, 1)                                         /* 64 x 64, 4 waves */                                                                \
  X(a, 126, 2, 4, 2, 2)                                         /* 128 x 256, 8 waves */                                                              \
  X(a, 127, 2, 4, 1, 2)                                         /* 64 x 256, 8 waves */                                                               \
  X(a, 128, 4, 4, 1, 1)                                         /* 128 x 128, 16 waves */                                                             \
  X(a, 129, 4, 2, 1, 2, 3)                                      /* 128 x 128, 8 waves, 3 stages */

// split rings, wave-specialised DMA issue (round 5): weight ring NSA deep, activation ring NSB deep (channels x pixels)
// launch_gemm1x1_split<WGM, WGN, WM, WN, NSA, NSB>
#define FAR3D_TILES_GEMM_SPLIT(X, a)                                                                                                                  \
  X(a, 140, 4, 2, 2, 4, 2, 3)                                   /* 256 x 256, 8 waves of 64 ch x 128 px, rings 2 + 3 (160 KiB) */                     \
  X(a, 141, 2, 2, 4, 4, 2, 3)                                   /* 256 x 256, 4 waves of 128 ch x 128 px (256 accumulator registers), rings 2 + 3 */  \
  X(a, 142, 2, 4, 2, 2, 2, 4)                                   /* 128 x 256, 8 waves of 64 x 64, rings 2 + 4 (160 KiB) */                            \
  X(a, 143, 4, 2, 2, 2, 2, 4)                                   /* 256 x 128, 8 waves of 64 x 64, rings 2 + 4 (128 KiB) */                            \
  X(a, 144, 4, 2, 2, 4, 2, 2)                                   /* 256 x 256, rings 2 + 2: tile 123 with the specialised issue (control) */           \
  X(a, 145, 4, 4, 2, 2, 2, 3)                                   /* 256 x 256, 16 waves of 64 x 64, rings 2 + 3 */

// launch_conv3x3_pipe<WGM, WGN, WM, WN[, NSW, RPS, NT, PAIR, STRIDE]>
// pipelined LDS-patch 3x3 kernel: (channels x rows-of-32-pixels, waves)
// software-pipelined kernel (register double-buffered fragments, immediate-offset LDS addressing)
#define FAR3D_TILES_CONV3(X, a)                                                                                                                       \
  X(a, 50, 2, 2, 1, 2)                                          /* 64 x 4 rows */                                                                     \
  X(a, 51, 1, 4, 2, 1)                                          /* 64 x 4 rows (1x4 waves) */                                                         \
  X(a, 52, 1, 4, 1, 1)                                          /* 32 x 4 rows */                                                                     \
  X(a, 53, 2, 2, 2, 2)                                          /* 128 x 4 rows */                                                                    \
  X(a, 54, 1, 4, 1, 2)                                          /* 32 x 8 rows */                                                                     \
  X(a, 55, 2, 2, 1, 1)                                          /* 64 x 2 rows */                                                                     \
  X(a, 57, 2, 2, 1, 4)                                          /* 64 x 8 rows */                                                                     \
  X(a, 58, 2, 2, 2, 1)                                          /* 128 x 2 rows */                                                                    \
  X(a, 59, 1, 4, 3, 1)                                          /* 96 x 4 rows */                                                                     \
  /* 8 / 16 waves per workgroup sharing one patch + weight slab */                                                                                    \
  X(a, 60, 2, 4, 1, 2)                                          /* 64 x 8 rows, 8 waves */                                                            \
  X(a, 61, 2, 4, 1, 1)                                          /* 64 x 4 rows, 8 waves */                                                            \
  X(a, 62, 4, 2, 1, 2)                                          /* 128 x 4 rows, 8 waves */                                                           \
  X(a, 63, 2, 8, 1, 1)                                          /* 64 x 8 rows, 16 waves */                                                           \
  X(a, 64, 1, 8, 2, 1)                                          /* 64 x 8 rows, 8 waves of 64 ch x 1 row */                                           \
  X(a, 65, 1, 8, 1, 1)                                          /* 32 x 8 rows, 8 waves */                                                            \
  X(a, 66, 4, 4, 1, 1)                                          /* 128 x 4 rows, 16 waves */                                                          \
  X(a, 67, 4, 2, 1, 1)                                          /* 128 x 2 rows, 8 waves */                                                           \
  /* 3-deep weight ring (kernel rows prefetched two steps ahead) */                                                                                   \
  X(a, 90, 2, 4, 1, 2, 3)                                       /* 64 x 8 rows, 8 waves */                                                            \
  X(a, 91, 2, 4, 1, 1, 3)                                       /* 64 x 4 rows, 8 waves */                                                            \
  X(a, 92, 1, 8, 1, 1, 3)                                       /* 32 x 8 rows, 8 waves */                                                            \
  X(a, 93, 1, 4, 1, 1, 3)                                       /* 32 x 4 rows, 4 waves */                                                            \
  X(a, 94, 2, 2, 1, 2, 3)                                       /* 64 x 4 rows, 4 waves */                                                            \
  X(a, 95, 2, 8, 1, 1, 3)                                       /* 64 x 8 rows, 16 waves */                                                           \
  X(a, 96, 1, 8, 2, 1, 3)                                       /* 64 x 8 rows, 8 waves of 64 ch x 1 row */                                           \
  X(a, 97, 2, 2, 1, 1, 3)                                       /* 64 x 2 rows, 4 waves */                                                            \
  /* whole-chunk steps (9 taps per barrier) for the layers with a single workgroup per CU */                                                          \
  X(a, 100, 2, 4, 1, 2, 2, 3)                                   /* 64 x 8 rows, 8 waves */                                                            \
  X(a, 101, 1, 8, 1, 1, 2, 3)                                   /* 32 x 8 rows, 8 waves */                                                            \
  X(a, 102, 1, 4, 1, 1, 2, 3)                                   /* 32 x 4 rows, 4 waves */                                                            \
  X(a, 103, 2, 4, 1, 1, 2, 3)                                   /* 64 x 4 rows, 8 waves */                                                            \
  /* whole-chunk steps, deeper rings (NSW - 1 chunks in flight, counted vmcnt).  Measured in round 4 and NOT faster anywhere */                       \
  /* (profiles/r4/tune_bf16_3x3_deep_rings.log: stage-4 c1 21 -> 22 us, stage-5 c1 9.2 -> 10 us): the K-short layers are not */                       \
  /* waiting for their DMA round trips; kept as tested tiles */                                                                                       \
  X(a, 104, 2, 4, 1, 1, 3, 3)                                   /* 64 x 4 rows, 8 waves, 3 chunks (150 KB) */                                         \
  X(a, 105, 1, 4, 1, 1, 3, 3)                                   /* 32 x 4 rows, 4 waves, 3 chunks (94 KB) */                                          \
  X(a, 106, 1, 4, 1, 1, 4, 3)                                   /* 32 x 4 rows, 4 waves, 4 chunks (126 KB) */                                         \
  /* fat tiles (round 5): 2x2 .. 2x4 / 4x2 / 5x1 MFMA tiles per wave -- half to a third of the L2 -> LDS bytes and of the */                          \
  /* fragment reads per MFMA of the 1x2 tiles above, workgroups that live 4-8x longer (per-workgroup set-up, first fill and */                        \
  /* epilogue amortised); for the layers with >= 4 rounds of workgroups (stem2, stage 2, stage 3, FPN / 2D-head level 0) */                           \
  X(a, 130, 2, 4, 2, 2)                                         /* 128 x 8 rows, 8 waves of 64 ch x 2 rows */                                         \
  X(a, 131, 2, 4, 2, 4)                                         /* 128 x 16 rows, 8 waves of 64 ch x 4 rows */                                        \
  X(a, 132, 1, 8, 4, 1)                                         /* 128 x 8 rows, 8 waves of 128 ch x 1 row */                                         \
  X(a, 133, 2, 4, 1, 4)                                         /* 64 x 16 rows, 8 waves of 32 ch x 4 rows */                                         \
  X(a, 134, 1, 8, 5, 1)                                         /* 160 x 8 rows, 8 waves of 160 ch x 1 row (stage 3: all channels) */                 \
  X(a, 135, 1, 8, 5, 1, 3)                                      /* 134 with a 3-deep weight ring */                                                   \
  X(a, 136, 2, 2, 2, 4)                                         /* 128 x 8 rows, 4 waves of 64 ch x 4 rows */                                         \
  X(a, 137, 2, 4, 2, 2, 3)                                      /* 130 with a 3-deep weight ring */                                                   \
  X(a, 138, 1, 8, 2, 2)                                         /* 64 x 16 rows, 8 waves of 64 ch x 2 rows (stem2: Cout 64) */                        \
  X(a, 139, 1, 8, 3, 1)                                         /* 96 x 8 rows, 8 waves of 96 ch x 1 row */                                           \
  /* 3x3 / stride 2 / pad 1 on the LDS-patch kernel (round 5; de-interleaved patch rows): (channels x output rows of 32 pixels, waves) */             \
  X(a, 30, 4, 2, 1, 2, 2, 1, 1, false, 2)                       /* 128 x 4 rows, 8 waves */                                                           \
  X(a, 31, 2, 2, 1, 1, 2, 1, 1, false, 2)                       /* 64 x 2 rows, 4 waves */                                                            \
  X(a, 32, 4, 2, 1, 1, 2, 1, 1, false, 2)                       /* 128 x 2 rows, 8 waves */                                                           \
  X(a, 33, 2, 4, 1, 1, 2, 1, 1, false, 2)                       /* 64 x 4 rows, 8 waves */                                                            \
  X(a, 34, 2, 2, 1, 2, 2, 1, 1, false, 2)                       /* 64 x 4 rows, 4 waves */                                                            \
  X(a, 35, 4, 2, 1, 2, 3, 1, 1, false, 2)                       /* 30 with a 3-deep weight ring */

// ---- igemm_pair.hip: pair-stored activations x split weights (the fast path of the bf16x3 precision mode)
// launch_gemm1x1_pipe<WGM, WGN, WM, WN, NT, PAIR>: 1x1 / stride 1 (channels x pixels, waves); tile 0 on such a layer = 179
#define FAR3D_TILES_PAIR_GEMM(X, a)                                                                                                                   \
  X(a, 170, 2, 2, 2, 2, 3, true)                                /* 128 x 128, 4 waves */                                                              \
  X(a, 171, 2, 4, 2, 1, 3, true)                                /* 128 x 128, 8 waves */                                                              \
  X(a, 172, 2, 4, 2, 2, 3, true)                                /* 128 x 256, 8 waves */                                                              \
  X(a, 173, 4, 2, 2, 2, 3, true)                                /* 256 x 128, 8 waves */                                                              \
  X(a, 174, 2, 2, 1, 2, 3, true)                                /* 64 x 128, 4 waves */                                                               \
  X(a, 175, 2, 4, 1, 1, 3, true)                                /* 64 x 128, 8 waves */                                                               \
  X(a, 176, 2, 2, 2, 1, 3, true)                                /* 128 x 64, 4 waves */                                                               \
  X(a, 177, 4, 4, 2, 1, 3, true)                                /* 256 x 128, 16 waves */                                                             \
  X(a, 178, 2, 4, 1, 2, 3, true)                                /* 64 x 256, 8 waves */                                                               \
  X(a, 179, 4, 2, 1, 2, 3, true)                                /* 128 x 128, 8 waves (1x2 tiles per wave) */                                         \
  X(a, 180, 2, 2, 1, 1, 3, true)                                /* 64 x 64, 4 waves */                                                                \
  X(a, 181, 4, 4, 1, 1, 3, true)                                /* 128 x 128, 16 waves */                                                             \
  /* round 6: pixel tiles of 160 / 96 for the maps a 128-pixel grid leaves half empty (stage 5's 4 200 pixels x 1 024 channels are 264 */             \
  /* workgroups of 128 x 128 = 1.03 per CU; 128 x 160 is 216 -- one round: 64 -> 58 us; FPN lateral 1: 33 -> 29 us).  192-channel tiles */            \
  /* for stage 4 (792 workgroups = 3.09 per CU) were measured too and are SLOWER than 128 x 128 (142-168 against 116-135 us, */                       \
  /* profiles/r6/tune_pair_fill_tiles.log): two co-resident workgroups per CU already even that grid out. */                                          \
  X(a, 185, 2, 5, 2, 1, 3, true)                                /* 128 x 160, 10 waves */                                                             \
  X(a, 186, 4, 1, 1, 5, 3, true)                                /* 128 x 160, 4 waves of 32 ch x 160 px */                                            \
  X(a, 187, 2, 3, 1, 1, 3, true)                                /* 64 x 96, 6 waves */                                                                \
  X(a, 188, 1, 3, 2, 1, 3, true)                                /* 64 x 96, 3 waves */                                                                \
  X(a, 279, 4, 2, 1, 2, 1, true)                                /* hi only: 128 x 128, 8 waves */                                                     \
  X(a, 280, 2, 2, 1, 1, 1, true)                                /* hi only: 64 x 64, 4 waves */

// launch_conv3x3_pipe<WGM, WGN, WM, WN, NSW, RPS, NT, PAIR[, STRIDE]>: 3x3 / stride 1 / pad 1 (channels x rows of 32 pixels); tile 0 = 160
#define FAR3D_TILES_PAIR_CONV3(X, a)                                                                                                                  \
  X(a, 150, 2, 2, 1, 2, 2, 1, 3, true)                          /* 64 x 4 rows */                                                                     \
  X(a, 152, 1, 4, 1, 1, 2, 1, 3, true)                          /* 32 x 4 rows */                                                                     \
  X(a, 153, 2, 2, 2, 2, 2, 1, 3, true)                          /* 128 x 4 rows */                                                                    \
  X(a, 154, 1, 4, 1, 2, 2, 1, 3, true)                          /* 32 x 8 rows */                                                                     \
  X(a, 155, 2, 2, 1, 1, 2, 1, 3, true)                          /* 64 x 2 rows */                                                                     \
  X(a, 157, 2, 2, 1, 4, 2, 1, 3, true)                          /* 64 x 8 rows, 4 waves */                                                            \
  X(a, 159, 1, 4, 3, 1, 2, 1, 3, true)                          /* 96 x 4 rows */                                                                     \
  X(a, 160, 2, 4, 1, 2, 2, 1, 3, true)                          /* 64 x 8 rows, 8 waves */                                                            \
  X(a, 161, 2, 4, 1, 1, 2, 1, 3, true)                          /* 64 x 4 rows, 8 waves */                                                            \
  X(a, 162, 4, 2, 1, 2, 2, 1, 3, true)                          /* 128 x 4 rows, 8 waves */                                                           \
  X(a, 163, 2, 8, 1, 1, 2, 1, 3, true)                          /* 64 x 8 rows, 16 waves */                                                           \
  X(a, 164, 1, 8, 2, 1, 2, 1, 3, true)                          /* 64 x 8 rows, 8 waves of 64 ch x 1 row */                                           \
  X(a, 165, 1, 8, 1, 1, 2, 1, 3, true)                          /* 32 x 8 rows, 8 waves */                                                            \
  X(a, 166, 4, 4, 1, 1, 2, 1, 3, true)                          /* 128 x 4 rows, 16 waves */                                                          \
  X(a, 167, 4, 2, 1, 1, 2, 1, 3, true)                          /* 128 x 2 rows, 8 waves */                                                           \
  X(a, 168, 2, 4, 2, 1, 2, 1, 3, true)                          /* 128 x 4 rows, 8 waves of 64 ch x 1 row */                                          \
  /* 7 rows: stage 4's 40-row maps are 6 x 7 (252 workgroups of 64 channels on 256 CUs) instead of 5 x 8 (210) */                                     \
  X(a, 169, 2, 7, 1, 1, 2, 1, 3, true)                          /* 64 x 7 rows, 14 waves */                                                           \
  X(a, 190, 1, 7, 1, 1, 2, 1, 3, true)                          /* 32 x 7 rows, 7 waves */                                                            \
  X(a, 198, 1, 7, 2, 1, 2, 1, 3, true)                          /* 64 x 7 rows, 7 waves of 64 ch x 1 row */                                           \
  /* 3-deep weight ring */                                                                                                                            \
  X(a, 191, 2, 4, 1, 1, 3, 1, 3, true)                          /* 64 x 4 rows, 8 waves */                                                            \
  X(a, 192, 1, 8, 1, 1, 3, 1, 3, true)                          /* 32 x 8 rows, 8 waves */                                                            \
  X(a, 193, 1, 4, 1, 1, 3, 1, 3, true)                          /* 32 x 4 rows, 4 waves */                                                            \
  X(a, 197, 2, 2, 1, 1, 3, 1, 3, true)                          /* 64 x 2 rows, 4 waves */                                                            \
  /* hi planes only */                                                                                                                                \
  X(a, 260, 2, 4, 1, 2, 2, 1, 1, true)                          /* 64 x 8 rows, 8 waves */                                                            \
  X(a, 265, 1, 8, 1, 1, 2, 1, 1, true)                          /* 32 x 8 rows, 8 waves */                                                            \
  X(a, 252, 1, 4, 1, 1, 2, 1, 1, true)                          /* 32 x 4 rows, 4 waves */                                                            \
  /* 3x3 / stride 2 / pad 1 (de-interleaved patch rows): the LDS holds 2 output rows */                                                               \
  X(a, 330, 2, 2, 1, 1, 2, 1, 3, true, 2)                       /* 64 x 2 rows, 4 waves */                                                            \
  X(a, 331, 1, 2, 1, 1, 2, 1, 3, true, 2)                       /* 32 x 2 rows, 2 waves */

// ---- igemm_pair.hip: fp32 activation rows on the pipelined GEMM kernel, launch_gemm1x1_pipe<..., NT, PAIR, NS, F32B[, F32X, KS]> (the rows
// are handed over as if pair-stored: the caller doubles P.ldx and P.x_img_stride; 1x1 / stride 1, Cin % 32 == 0)
// x pre-split weights (F32B): the pair ids 179-181 + 300; tile 0 on such a layer = 479 / 480
#define FAR3D_TILES_F32_GEMM(X, a)                                                                                                                    \
  X(a, 479, 4, 2, 1, 2, 3, true, 2, true)                       /* 128 x 128, 8 waves (1x2 tiles per wave) */                                         \
  X(a, 480, 2, 2, 1, 1, 3, true, 2, true)                       /* 64 x 64, 4 waves */                                                                \
  X(a, 481, 4, 4, 1, 1, 3, true, 2, true)                       /* 128 x 128, 16 waves */                                                             \
  /* x fp32 weight rows, EXACT fp32 MFMA (F32X) */                                                                                                    \
  X(a, 482, 2, 2, 1, 1, 3, true, 2, true, true)                 /* 64 x 64, 4 waves, 2 stages */                                                      \
  X(a, 483, 2, 2, 1, 1, 3, true, 4, true, true)                 /* 64 x 64, 4 waves, 4 stages (3 steps in flight) */                                  \
  X(a, 484, 4, 2, 1, 2, 3, true, 3, true, true)                 /* 128 x 128, 8 waves, 3 stages */                                                    \
  X(a, 485, 4, 4, 1, 1, 3, true, 2, true, true)                 /* 128 x 128, 16 waves, 2 stages */                                                   \
  X(a, 486, 2, 4, 1, 1, 3, true, 2, true, true)                 /* 64 x 128, 8 waves, 2 stages */                                                     \
  /* K groups inside the workgroup (igemm_kernels.hpp, KS): (channels x rows) tile, waves = groups x waves per group */                               \
  X(a, 487, 2, 2, 1, 1, 3, true, 2, true, true, 2)              /* 64 x 64, 2 groups x 4 waves */                                                     \
  X(a, 488, 2, 2, 1, 1, 3, true, 2, true, true, 4)              /* 64 x 64, 4 groups x 4 waves */                                                     \
  X(a, 489, 1, 2, 1, 1, 3, true, 2, true, true, 4)              /* 32 x 64, 4 groups x 2 waves */                                                     \
  X(a, 490, 2, 1, 1, 1, 3, true, 2, true, true, 4)              /* 64 x 32, 4 groups x 2 waves */                                                     \
  X(a, 491, 1, 1, 1, 1, 3, true, 2, true, true, 4)              /* 32 x 32, 4 groups x 1 wave */                                                      \
  X(a, 492, 1, 1, 1, 1, 3, true, 2, true, true, 8)              /* 32 x 32, 8 groups x 1 wave */                                                      \
  X(a, 493, 1, 2, 1, 1, 3, true, 2, true, true, 2)              /* 32 x 64, 2 groups x 2 waves */                                                     \
  X(a, 494, 2, 2, 1, 1, 3, true, 3, true, true, 2)              /* 64 x 64, 2 groups x 4 waves, 3 stages */

// ---- conv_ws.hip: persistent wave-specialised kernels (conv_ws.hpp); bias + activation + pair / bf16 store only
// launch_conv3x3_ws<WGM, WGN, WM, WN, NP, PAIR, DBUF[, NSW, FLAGS, GRP, DEFER]>: 3x3 / stride 1 / pad 1.  The mark after the id:
//   SINGLE         far3d_conv2d_nhwc only
//   GROUPED        id + 100 is the same workgroup as a grouped launch (launch_conv3x3_ws_grouped with the row's arguments)
//   GROUPED_PLAIN  the same, but the grouped launch keeps the epilogue in place (DEFER off): 505 shipped and was measured that way
// 400-419 pair storage, one hand-over per tap; 420-423 plain bf16; 440-445 LDS counters; 450-459 one hand-over per kernel row
// (consumer grid WGM x WGN, tiles per consumer WM x WN, producers, pair, double-buffered fragments[, ring stages, FLAGS, taps per
// hand-over, deferred epilogue])
#define FAR3D_TILES_WS_CONV3(X, a)                                                                                                                    \
  X(a, 400, GROUPED, 2, 4, 2, 2, 4, true, true)                 /* 128 ch x 8 rows: 8 consumers of 64 ch x 2 rows + 4 producers */                    \
  X(a, 401, SINGLE, 1, 8, 2, 1, 4, true, true)                  /* 64 ch x 8 rows: 8 consumers of 64 ch x 1 row (Cout 64) */                          \
  X(a, 402, SINGLE, 1, 8, 5, 1, 4, true, false)                 /* 160 ch x 8 rows: 8 consumers of 160 ch x 1 row (stage 3) */                        \
  X(a, 403, SINGLE, 2, 4, 3, 1, 4, true, true)                  /* 192 ch x 4 rows: 8 consumers of 96 ch x 1 row (stage 4) */                         \
  X(a, 404, SINGLE, 2, 2, 1, 2, 2, true, true, 3, false, 1, true)/* 64 ch x 4 rows: 4 consumers of 32 ch x 2 rows + 2 producers (2 per CU) */         \
  X(a, 405, GROUPED_PLAIN, 2, 4, 2, 1, 4, true, true, 3, false, 1, true)/* 128 ch x 4 rows: 8 consumers of 64 ch x 1 row */                           \
  X(a, 406, SINGLE, 2, 4, 1, 2, 4, true, true, 3, false, 1, true)/* 64 ch x 8 rows: 8 consumers of 32 ch x 2 rows */                                  \
  X(a, 407, SINGLE, 1, 4, 5, 1, 2, true, false)                 /* 160 ch x 4 rows: 4 consumers of 160 ch x 1 row + 2 producers */                    \
  X(a, 408, SINGLE, 1, 4, 3, 1, 2, true, true)                  /* 96 ch x 4 rows: 4 consumers + 2 producers (2 per CU) */                            \
  X(a, 409, SINGLE, 2, 4, 2, 2, 2, true, true)                  /* 400 with 2 producers */                                                            \
  /* deeper weight rings (the producers run NSW - 1 steps ahead) */                                                                                   \
  X(a, 410, SINGLE, 2, 4, 2, 2, 4, true, true, 4)               /* 400 with 4 stages (154 KB) */                                                      \
  X(a, 411, SINGLE, 2, 4, 2, 1, 4, true, true, 6)               /* 405 (128 ch x 4 rows) with 6 stages */                                             \
  X(a, 412, SINGLE, 2, 4, 1, 2, 4, true, true, 8, false, 1, true)/* 406 (64 ch x 8 rows) with 8 stages */                                             \
  X(a, 413, SINGLE, 1, 8, 2, 1, 4, true, true, 8)               /* 401 (64 ch x 8 rows, Cout 64) with 8 stages */                                     \
  X(a, 414, SINGLE, 1, 4, 5, 1, 2, true, false, 5)              /* 407 (160 ch x 4 rows) with 5 stages */                                             \
  X(a, 415, SINGLE, 2, 2, 1, 2, 2, true, true, 6, false, 1, true)/* 404 (64 ch x 4 rows, 2 per CU) with 6 stages */                                   \
  X(a, 416, SINGLE, 2, 4, 3, 1, 4, true, true, 4)               /* 403 (192 ch x 4 rows) with 4 stages */                                             \
  X(a, 417, SINGLE, 2, 4, 2, 1, 4, true, true, 4)               /* 405 with 4 stages */                                                               \
  X(a, 418, SINGLE, 4, 2, 2, 2, 4, true, true, 3)               /* 256 ch x 4 rows: 8 consumers of 64 ch x 2 rows (148 KB) */                         \
  X(a, 419, SINGLE, 4, 2, 2, 1, 4, true, true, 3)               /* 256 ch x 2 rows: 8 consumers of 64 ch x 1 row */                                   \
  /* hand-over through LDS counters instead of a workgroup barrier per step (FLAGS): consumer waves run free of each other.  Measured */              \
  /* SLOWER than the barrier form (profiles/r6/ws_ab_pair.txt: s2.c1 281 us against 212, s4.c1 59 against 38): the polls cost more than */            \
  /* the lockstep they remove.  Kept as tested tiles for the record. */                                                                               \
  X(a, 440, SINGLE, 2, 4, 2, 2, 4, true, true, 3, true)         /* 400 */                                                                             \
  X(a, 444, SINGLE, 2, 2, 1, 2, 2, true, true, 3, true)         /* 404 (64 ch x 4 rows, 2 per CU) */                                                  \
  X(a, 445, SINGLE, 2, 4, 2, 1, 4, true, true, 6, true)         /* 411 (128 ch x 4 rows, 6 stages) */                                                 \
  /* one barrier per KERNEL ROW (3 taps) instead of per tap, ring of 2 or 3 rows (GRP = 3) */                                                         \
  X(a, 450, SINGLE, 2, 4, 2, 1, 4, true, true, 6, false, 3, true)/* 128 ch x 4 rows, ring of 2 rows (149 KB) */                                       \
  X(a, 451, SINGLE, 2, 4, 1, 2, 4, true, true, 6, false, 3, true)/* 64 ch x 8 rows, ring of 2 rows */                                                 \
  X(a, 452, GROUPED, 2, 4, 1, 2, 4, true, true, 9, false, 3, true)/* 64 ch x 8 rows, ring of 3 rows (160 KB) */                                       \
  X(a, 453, SINGLE, 1, 8, 2, 1, 4, true, true, 6, false, 3, true)/* 64 ch x 8 rows (Cout 64), ring of 2 rows */                                       \
  X(a, 454, SINGLE, 1, 8, 2, 1, 4, true, true, 9, false, 3)     /* 64 ch x 8 rows (Cout 64), ring of 3 rows */                                        \
  X(a, 455, SINGLE, 1, 7, 2, 1, 4, true, true, 9, false, 3)     /* 64 ch x 7 rows: stage 4's 40 rows = 6 x 7 -> 252 items on 256 CUs */               \
  X(a, 456, GROUPED, 2, 7, 1, 1, 2, true, true, 9, false, 3, true)/* 64 ch x 7 rows, 14 consumers of 32 ch x 1 row + 2 producers */                   \
  X(a, 457, SINGLE, 2, 2, 1, 2, 2, true, true, 6, false, 3, true)/* 64 ch x 4 rows, 4 consumers + 2 producers */                                      \
  X(a, 458, SINGLE, 1, 4, 3, 1, 2, true, true, 6, false, 3)     /* 96 ch x 4 rows, 4 consumers + 2 producers */                                       \
  X(a, 459, GROUPED, 2, 4, 1, 1, 4, true, true, 9, false, 3, true)/* 64 ch x 4 rows, 8 consumers of 32 ch x 1 row, ring of 3 rows */                  \
  X(a, 420, SINGLE, 2, 4, 2, 2, 4, false, true)                 /* plain bf16: 128 ch x 8 rows */                                                     \
  X(a, 421, SINGLE, 1, 8, 2, 1, 4, false, true, 3, false, 1, true)/* plain bf16: 64 ch x 8 rows */                                                    \
  X(a, 422, SINGLE, 1, 8, 5, 1, 4, false, true)                 /* plain bf16: 160 ch x 8 rows */                                                     \
  X(a, 423, SINGLE, 2, 4, 3, 1, 4, false, true)                 /* plain bf16: 192 ch x 4 rows */

// launch_gemm1x1_ws<WGM, WGN, WM, WN, NP, NSW, GRP>: 1x1 / stride 1 on pair-stored maps, channel sums allowed (channels x pixels)
// (consumer grid WGM x WGN, tiles per consumer WM x WN, producers, ring stages, steps per hand-over)
#define FAR3D_TILES_WS_GEMM(X, a)                                                                                                                     \
  X(a, 460, 4, 2, 1, 2, 4, 4, 1)                                /* 128 x 128: 8 consumers of 32 ch x 64 px + 4 producers, 4 stages (128 KB) */        \
  X(a, 461, 4, 2, 1, 2, 4, 4, 2)                                /* 460 with a hand-over every 2 steps */                                              \
  X(a, 462, 2, 4, 2, 1, 4, 4, 2)                                /* 128 x 128: 8 consumers of 64 ch x 32 px */                                         \
  X(a, 463, 2, 2, 2, 2, 4, 4, 2)                                /* 128 x 128: 4 consumers of 64 x 64 + 4 producers */                                 \
  X(a, 464, 4, 2, 2, 2, 4, 3, 1)                                /* 256 x 128: 8 consumers of 64 x 64, 3 stages of 48 KB */                            \
  X(a, 465, 4, 2, 1, 2, 2, 4, 2)                                /* 461 with 2 producers */                                                            \
  X(a, 466, 2, 2, 1, 2, 4, 6, 3)                                /* 64 x 128: 4 consumers of 32 ch x 64 px, 6 stages of 24 KB, hand-over every 3 */    \
  X(a, 467, 2, 4, 1, 1, 4, 6, 2)                                /* 64 x 128: 8 consumers of 32 x 32, 6 stages */                                      \
  X(a, 468, 2, 2, 1, 2, 2, 3, 1)                                /* 64 x 128: 4 consumers + 2 producers, 3 stages (72 KB: 2 per CU) */                 \
  X(a, 469, 4, 2, 1, 2, 4, 2, 1)                                /* 460 with 2 stages (64 KB: 2 per CU) */                                             \
  X(a, 470, 2, 4, 2, 2, 4, 3, 1)                                /* 128 x 256: 8 consumers of 64 x 64, 3 stages of 48 KB */                            \
  X(a, 471, 2, 2, 4, 2, 4, 3, 1)                                /* 256 x 128: 4 consumers of 128 ch x 64 px */                                        \
  X(a, 473, 4, 2, 2, 2, 2, 3, 1)                                /* 464 with 2 producers */                                                            \
  X(a, 474, 3, 2, 2, 2, 4, 3, 1)                                /* 192 x 128: 6 consumers of 64 x 64, 3 stages of 40 KB */                            \
  X(a, 475, 2, 2, 2, 2, 4, 4, 1)                                /* 463 with a hand-over per step */                                                   \
  X(a, 476, 2, 4, 2, 2, 2, 3, 1)                                /* 470 with 2 producers */
