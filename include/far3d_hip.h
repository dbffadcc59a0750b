/* far3d_hip.h -- C ABI of libfar3d_hip.so: the MI355X (gfx950) kernels of the Far3D inference hot path.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every `const void*` / `float*` tensor argument is a DEVICE pointer
 *     to a contiguous buffer unless the parameter comment says "host";
 *   - `stream` is a hipStream_t (NULL = default stream); kernels are enqueued, never synchronised;
 *   - return 0 on success, negative FAR3D_ERR_* otherwise; far3d_last_error() gives the reason
 *     (thread-local, valid until the next failing call on the same thread);
 *   - dtype codes: FAR3D_DT_F32 = 0, FAR3D_DT_BF16 = 1 (raw bfloat16 bits).
 * Citations `ref:` are file:line under the reference checkout (projects/mmdet3d_plugin/...).
 */
#ifndef FAR3D_HIP_H
#define FAR3D_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FAR3D_DT_F32 0
#define FAR3D_DT_BF16 1
/* weight-dtype code of far3d_conv2d_nhwc only: fp32 activations, products computed as a two-term bf16 split
 * (x = hi + lo, both round-to-nearest-even bf16; hi*hi' + hi*lo' + lo*hi' on the bf16 MFMA, fp32 accumulation): ~1e-5 relative
 * operand error at ~5x the fp32 matrix rate.  The "bf16x3" precision mode of the engine.  The weight buffer has the byte size
 * and row stride of the fp32 layout, but holds the split: every 32-channel block of a row (128 B) is 32 hi bf16 followed by
 * 32 lo bf16 (hi = bf16(w), lo = bf16(w - hi)). */
#define FAR3D_DT_F32_BF16X3 2
/* activation storage code ("pair"): a map of C logical channels (C % 32 == 0) holds fp32 values as 2C bf16 per pixel; every
 * 32-channel block is 32 hi = bf16(x) followed by 32 lo = bf16(x - hi) (hi + lo is exact in fp32 and carries 16 significant bits
 * at fp32's byte size).  Pointers, pixel strides and image strides of pair tensors count bf16 elements of the 2C-wide rows; channel
 * slices start at multiples of 32 logical channels.  Accepted by far3d_conv2d_nhwc (x / y / res, with w_dt = FAR3D_DT_F32_BF16X3:
 * the 64-byte hi / lo runs are what the LDS-DMA kernels stream, each product = 3 bf16 MFMAs), far3d_ese_nhwc,
 * far3d_groupnorm_nhwc, far3d_maxpool3x3s2_nhwc (dt) and far3d_stem_im2col (out_dt).  The "bf16x3" engine mode stores every
 * conv-stage activation this way. */
#define FAR3D_DT_BF16_PAIR 3
/* upper bound on the per-image partial-sum workgroups of far3d_ese_nhwc / far3d_groupnorm_nhwc (sizes their scratch) */
#define FAR3D_SUMS_MAX_PARTS 32
/* fraction bits of the fixed-point channel sums of far3d_conv2d_nhwc (chan_sums) */
#define FAR3D_SUMS_FRAC_BITS 18
/* partial sums [N][PARTS][C][2] + gates / group statistics [N][C] */
#define FAR3D_SUMS_SCRATCH_FLOATS(N, C) ((long)(N) * (C) * (2 * FAR3D_SUMS_MAX_PARTS + 1))

#define FAR3D_OK 0
#define FAR3D_ERR_ARG (-1)
#define FAR3D_ERR_LAUNCH (-2)
#define FAR3D_ERR_UNSUPPORTED (-3)

const char* far3d_last_error(void);
int far3d_abi_version(void);
int far3d_device_count(void);
int far3d_device_arch(int dev, char* buf, int buflen);

/* Multi-scale deformable attention, forward.
 * Replaces: mmcv-full 1.6.2 `ms_deform_attn_forward` as reached through
 *   MultiScaleDeformableAttnFunction.apply(value, spatial_shapes, level_start_index,
 *                                          sampling_locations, attention_weights, im2col_step)
 *   ref: models/utils/detr3d_transformer.py:561-563 (and models/utils/sparse_blocks.py:334-336).
 * value (bs,S,H,Dh) f32|bf16; spatial_shapes (L,2) int64 (h,w) DEVICE; level_start_index (L) int64 DEVICE;
 * sampling_loc (bs,Q,H,L,P,2) f32, (x,y) in [0,1]; attn_weight (bs,Q,H,L,P) f32; out (bs,Q,H*Dh) f32.
 * Semantics: out[b,q,h,:] = sum_l sum_p w * bilinear(value_l[b,:,h,:], x*W_l-0.5, y*H_l-0.5), zeros outside
 * (== grid_sample(align_corners=False, padding_mode='zeros')).  Dh must be a multiple of 4. */
int far3d_msda_forward(const void* value, int value_dtype, const int64_t* spatial_shapes,
                       const int64_t* level_start_index, const float* sampling_loc,
                       const float* attn_weight, float* out, int bs, int S, int H, int Dh, int L, int Q,
                       int P, void* stream);

/* Fused perspective-aware aggregation (3D deformable cross-attention sampling), forward, one sample.
 * Replaces, in one launch: DeformableFeatureAggregationCuda.feature_sampling
 *   ref: models/utils/detr3d_transformer.py:544-569 (projection :547-552, replication :555, MSDA :561,
 *   cross-camera sum :565-569), the key-point construction :524-525, and the softmax/permute of
 *   _get_weights :540-542.  Operator shape family follows the reference's own (unused) fused op
 *   ref: models/utils/deformable_aggregation.py:17-29.
 * feat (N,S,C=256) f32|bf16 token-major value maps; ref (A,3) f32 normalised reference points;
 * offsets (A,P,3) f32 = learnable_fc(x); lidar2img (N,4,4) f32 row-major;
 * U (A,L*P*G) f32 and Vc (N,L*P*G) f32 with logits[a,n,(l*P+p)*G+g] = U[a,.] + Vc[n,.]
 *   ( = weights_fc((x+pos)[a] + cam_embed[n]) split by linearity; bias lives in Vc );
 * level_hw (L,2) int32 HOST (h,w); level_start (L) int32 HOST; pc_range 6 floats HOST;
 * ldU / ldOffs: row strides in floats of U and offsets (0 = dense; U rows must stay 16-byte aligned) so both can be column
 * blocks of one merged-GEMM output.
 * pad_h/pad_w = img_metas['pad_shape'] (ref :551-552).  out (A,C) of dtype out_dt (f32 | bf16).  perm: optional (A) int32 DEVICE permutation giving
 * the order in which queries are assigned to workgroups (camera-sorted order keeps one XCD's L2 on 1-2 cameras); it never
 * changes results (row a of `out` is always query a); an entry ~a (negative) means "row a holds no query": a zero row is
 * written and nothing else is done (far3d_agg_order produces such entries).  With perm, A counts the ENTRIES of perm (workgroups);
 * the rows they name may lie anywhere in ref / offsets / U / out (a subset of a larger query set).  Requires C=256, G=8, L<=4, N<=16,
 * N*P<=256, N*P*L<=384; a batch of samples of this family is far3d_aggregate_batched (below), and every other shape runs as
 * far3d_agg_operands -> far3d_msda_forward -> far3d_camera_sum (below).
 * cam_tables: the per-layer softmax factors of Vc from far3d_agg_tables / far3d_agg_order ((2+N)*L*P*G floats), or NULL.
 * variant: 0 = default: kernel 8 when cam_tables is given and N<=8, P<=16, value maps < 4 GiB, else kernel 7; 9 = kernel 8 with sibling
 * workgroups for heavy queries (below).
 *   8: two waves per query with specialised front ends (wave 0 projects and deals, wave 1 does the softmax statistics; two
 *      barriers), softmax factored into a query part (8 exp per lane) and the per-frame camera tables, (camera, level) items dealt to the waves by estimated work, bilinear taps merged per token row through the tent
 *      form of the interpolation weights (no atomics), padded LDS row lists, 16-byte row gathers from 32-bit byte offsets;
 *   7: round 2/3's kernel (two waves, levels split by parity, full 7-camera softmax from Vc, three barriers); 11 = 7 with its
 *      cross-lane reductions on the VALU and packed FMAs; 3 = round-1 kernel (workgroup per query, one gather per sample corner
 *      pair) -- 3, 7, 11 need Vc and are kept for A/B measurements; 12 = kernel 8 with round 4's greedy dealing of the items (kernel 8
 *      deals them by a contiguous split at the midpoints of the running work estimate since round 6; A/B).  All give the same result up
 *      to fp32 rounding. */
int far3d_aggregate_forward(const void* feat, int feat_dtype, const float* ref, const float* offsets,
                            const float* lidar2img, const float* U, const float* Vc, const float* cam_tables,
                            const int32_t* perm, void* out, int out_dt, int A,
                            int N, int S, int C, int G, int P, int L, const int32_t* level_hw,
                            const int32_t* level_start, const float* pc_range, float pad_h, float pad_w,
                            int ldU, int ldOffs, int variant, float* split_partials, int32_t* split_tickets, int split_extra,
                            const float* qbase, void* stream);
/* qbase != NULL (round 6, kernel 8 only, needs perm): SORTED mode.  U and offsets hold the row of the query of perm entry e AT ROW e
 * (launch order: their producers stored through far3d_agg_order's inv), qbase is far3d_agg_order's (A, 4) table and `ref` is not
 * read: every operand load of a workgroup depends on its block index only, perm[e] is needed for the hole test and the output row
 * alone.  out row a is query a as always, and the result is BIT-IDENTICAL to the unsorted call (same arithmetic in the same order).
 * Needs L * P <= 52 (the two hinted cameras' weight rows live in LDS).
 * The unsorted call costs a dependent round trip (perm[e] -> ref / offsets / U rows) before the first useful instruction. */
/* variant 13 (round 6, A/B measurement only): the sorted-mode kernel as TWO launches -- a list-build launch that writes every wave's row
 * list (offset + 8 weights per entry, <= 1024 entries per wave) and the softmax denominators to a global workspace, and a pure gather
 * launch (one workgroup per query) that reads them: VERDICT r5 item 3 (c).  Same entries in the same order (bit-identical on bf16 rows, 1 ulp on fp32 rows); measured 1.5 - 2.1x SLOWER than the fused launch.  Needs qbase,
 * perm, P = 13; split_partials = FAR3D_AGG_LISTS_FLOATS(A) floats (16-byte aligned), split_tickets = 2 * 8 * ceil(A / 8) int32. */
#define FAR3D_AGG_LISTS_FLOATS(A) ((long)(((A) + 7) / 8 * 8) * (2L * 1024 * 9 + 8))
/* variant 9 (round 5) = kernel 8 + SIBLING workgroups for heavy queries: the launch ends with its slowest wave, and the slowest waves
 * belong to the queries two cameras see.  far3d_agg_order(split_extra) marks those queries (flag 1 << 29 on their perm entry) and appends
 * one sibling entry per marked query (perm[A + e] = row | 1 << 30 | 1 << 29; unused slots 0x7fffffff); the launch runs split_extra extra
 * workgroups for them.  The two workgroups of a marked query deal its items into four shares instead of two, each publishes its
 * unnormalised 256-float sum in split_partials ([rows][2][256] f32) and draws a ticket from split_tickets ([rows] int32, ZERO at rest,
 * returned to zero); the second arrival adds the partials in part order and writes the row -- deterministic, run to run and graph vs
 * eager.  Unmarked queries take kernel 8's path unchanged.  The three split_* arguments are ignored by the other variants. */

/* far3d_aggregate_forward for a BATCH of samples in one launch: kernel 8 (cam_tables given, N<=8, P<=16, one sample's value maps
 * < 4 GiB) or kernel 7 (otherwise; needs Vc) with the sample as the grid's second index -- variant 0's choice, per sample.
 * feat (B,N,S,C=256) f32|bf16 contiguous (the reference's feat_flatten (B*N,S,C)); ref (B,A,3) f32; offsets and U: rows b*A + a of ONE
 * 2-D f32 buffer each, row strides ldOffs / ldU in floats (0 = dense; U rows 16-byte aligned, ldU % 4 == 0), as far3d_agg_operands
 * takes them; lidar2img (B,N,4,4) f32; Vc (B,N,J) f32 or NULL, J = L*P*G; cam_tables (B,2+N,J) f32 from far3d_agg_tables with
 * layers = B, or NULL; out (B,A,256) of dtype out_dt; the remaining arguments and the shape family (C=256, G=8, L<=4, N<=16,
 * N*P<=256, N*P*L<=384, N*S*C of ONE sample < 2^31) are far3d_aggregate_forward's; B <= 65535.  The offsets between samples are
 * formed in 64 bits: B*N*S*C may pass 2^31.  No perm, no sorted mode, no sibling split, no A/B variants: those belong to the engine's
 * one-sample call.
 * B == 0 or A == 0: FAR3D_OK, nothing launched.  Anything refused: FAR3D_ERR_ARG with the sizes in far3d_last_error(), nothing launched.
 * Contract: out[b] is BIT-IDENTICAL to far3d_aggregate_forward on sample b's operands (variant = 0, perm = NULL, qbase = NULL, that
 * sample's tables); it does not depend on B, and it is the same from run to run. */
int far3d_aggregate_batched(const void* feat, int feat_dtype, const float* ref, const float* offsets,
                            const float* lidar2img, const float* U, const float* Vc, const float* cam_tables,
                            void* out, int out_dt, int B, int A, int N, int S, int C, int G, int P, int L,
                            const int32_t* level_hw, const int32_t* level_start, const float* pc_range,
                            float pad_h, float pad_w, int ldU, int ldOffs, void* stream);

/* far3d_aggregate_batched with a HOLE of unused query rows per sample (the fixed-capacity threshold proposal mode and the multi-depth
 * extra rows of several scene streams: streams.StreamBatch(hole_rows=True)).  The arguments are far3d_aggregate_batched's, then the hole
 * in far3d_attention_streams' convention: hole_count NULL (no hole) or a DEVICE int32 array of B counts; sample b's rows
 * [hole_start + hole_count[b], hole_end) hold no query; hole_start and hole_end are shared by all samples.  A count outside
 * [0, hole_end - hole_start] is clamped into that range (far3d_proposal_gather never writes one).
 * Contract: a hole row of out[b] is an exact zero row in either out_dt and none of its operands (ref / offsets / U rows, which may hold
 * anything, NaN included) is read -- what the one-sample kernels do for a perm entry ~a.  Every other row has the bits
 * far3d_aggregate_batched writes, so out[b] as a whole is BIT-IDENTICAL to far3d_aggregate_forward on sample b with
 * perm = far3d_agg_order(..., hole_count[b], hole_start, hole_end); it does not depend on B or on the other samples' counts, and it is the
 * same from run to run.  hole_count == NULL: exactly far3d_aggregate_batched (hole_start / hole_end are ignored).
 * Refused with FAR3D_ERR_ARG, the hole named in far3d_last_error(), nothing launched: hole_count != NULL with hole_start < 0,
 * hole_end > A or hole_start > hole_end.  Every other rule (B == 0 / A == 0: FAR3D_OK, the sizes) is far3d_aggregate_batched's: the two
 * entries share one host path.  The count is one scalar load per workgroup, issued with the loads that do not depend on the query. */
int far3d_aggregate_batched_holes(const void* feat, int feat_dtype, const float* ref, const float* offsets,
                                  const float* lidar2img, const float* U, const float* Vc, const float* cam_tables,
                                  void* out, int out_dt, int B, int A, int N, int S, int C, int G, int P, int L,
                                  const int32_t* level_hw, const int32_t* level_start, const float* pc_range,
                                  float pad_h, float pad_w, int ldU, int ldOffs, const int32_t* hole_count, int hole_start,
                                  int hole_end, void* stream);

/* Softmax factors of the aggregation logits' camera part, for `layers` decoder layers in one launch (block = layer):
 * Vc (layers, N, J) f32 (far3d_cam_embed_chain's output, J = L*P*G, J % 4 == 0) -> tables (layers, 2+N, J) f32 =
 * [ mV = max_n Vc | EV = sum_n eV[n] | eV[n] = exp(Vc[n] - mV) ].  softmax_{n,j}(U[a][j] + Vc[n][j]) (ref models/utils/
 * detr3d_transformer.py:539-540) = exp(U[a][j] + mV[j] - m_a) * eV[n][j] / sum_j exp(U[a][j] + mV[j] - m_a) EV[j]: the camera
 * factors depend on the layer and the frame only, the per-query part shrinks to 8 exp per lane. */
int far3d_agg_tables(const float* Vc, float* tables, int layers, int N, int J, void* stream);

/* The aggregation's two MSDA operands, in the reference's own layout, for any shape and batch (csrc/agg_operands.hip).
 * DeformableFeatureAggregationCuda builds `points_2d` (ref: models/utils/detr3d_transformer.py:547-555) and `weights` (:535-542) and hands
 * them to the MSDA operator; far3d_aggregate_forward never materialises them and takes one shape family, one sample.  This entry point
 * writes both, so that  far3d_agg_operands -> far3d_msda_forward(bs = B*N) -> far3d_camera_sum  is the whole module for every shape the
 * reference class accepts, and an independent statement to hold the fused kernel against.  A fallback and an inspection path: the
 * operands (about 3 * B*N*A*L*P*G floats) go through HBM; never the default for the fused family.
 * Inputs = far3d_aggregate_forward's, with a batch dimension: ref (B,A,3) f32 normalised; offsets (B,A,P*3) f32, row stride ldOffs;
 * lidar2img (B,N,4,4) f32; U (B,A,J) f32, row stride ldU (rows b*A + a of ONE 2-D buffer; 0 = dense); Vc (B,N,J) f32; J = L*P*G indexed
 * (l*P + p)*G + g; pc_range 6 floats HOST; pad_h / pad_w as above.
 * Outputs: loc (B*N, A, G, L, P, 2) f32 -- with expand = 0 the compact (B*N, A, P, 2) (the reference repeats the P points over groups
 * and levels, :555); weights (B*N, A, G, L*P) f32; key_points (B, A, P, 3) f32 in metres (:524-525), or NULL.
 * fp32 throughout, as the reference states it: ref_m = ref*(hi-lo)+lo; key = ref_m + offset; (x,y,z) = rows 0..2 of lidar2img . [key,1];
 * zc = fmaxf(z, 1e-5f); u = (x / zc) / pad_w, v = (y / zc) / pad_h (true divisions); weights = softmax over the N*L*P entries of
 * U[a] + Vc[n] per (a, g): max subtracted, expf, a fixed summation order, a division by the sum.  One launch (workgroup per (b, a)), no
 * workspace, no atomics; the result does not depend on B or expand and is bit-identical from run to run.
 * Sizes: 1 <= N <= 32, 1 <= L <= 8, 1 <= P <= 64, 1 <= G <= 64, N*L*P <= 8192; anything else is FAR3D_ERR_ARG and nothing is launched.
 * 16-byte accesses are used where J % 4 == 0 (U rows: also ldU % 4 == 0) and the buffers are 16-byte aligned; up to J = 16384 a camera's
 * weights leave as one contiguous run. */
int far3d_agg_operands(const float* ref, const float* offsets, const float* lidar2img, const float* U, const float* Vc,
                       float* loc, float* weights, float* key_points, int B, int A, int N, int G, int P, int L,
                       const float* pc_range, float pad_h, float pad_w, int ldU, int ldOffs, int expand, void* stream);

/* Cross-camera sum behind the MSDA operator (ref: models/utils/detr3d_transformer.py:565-569): x (B*N, A, C) f32 -> out (B, A, C) f32,
 * cameras added in ascending order (((x0 + x1) + x2) + ...).  One streaming launch, 16-byte accesses where A*C % 4 == 0. */
int far3d_camera_sum(const float* x, float* out, int B, int N, int A, int C, void* stream);

/* Implicit-GEMM convolution / linear layer on the matrix cores (bf16 MFMA, or exact-fp32 MFMA when w_dt = F32).
 * Replaces the torch/cuDNN convolutions and nn.Linear GEMMs of the path:
 *   VoVNet conv+BN(eval)+ReLU  ref: models/backbones/vovnet.py:114-139,218-238 (BN folded into w/bias by the host),
 *   mmdet FPN laterals/outputs (ref cfg projects/configs/far3d.py:50-57; in-tree cousin models/necks/cp_fpn.py:156-208),
 *   YOLOX towers conv+BN+Swish ref: models/dense_heads/yolox_head.py:197-258, depth head convs
 *   ref: models/depth_predictor/depth_predictor.py:41-86, and every Linear of FarHead / the decoder
 *   (ref: models/dense_heads/farhead.py:228-282, models/utils/detr3d_transformer.py:503-512,525-540).
 * x: NHWC activations (x_dt), pixel stride ldx elements, image stride x_img_stride elements; the pointer is
 *    pre-offset to the first input channel (channel slices of a wider buffer are fine).
 * w: packed weights (w_dt) [R][KH*KW][ceil(Cin/32)*32] with R >= Cout + 256 rows (zero rows past Cout: channel tiles of up to
 *    256 rows over-read), zero padded in Cin; bias [R] f32 (16-byte aligned) or NULL.
 * y: NHWC output (y_dt), pixel stride ldy, image stride y_img_stride.  v = act(conv + bias) + res.
 * act: 0 none, 1 ReLU, 2 Swish.  res (optional, res_dt): NHWC Hr x Wr map added with nearest-neighbour upsampling
 *    (FPN top-down path); Hr=Ho, Wr=Wo gives a plain residual.
 * y2 (optional, y2_dt): second output y2 = y2_scale[n][m] * v + y2_shift[n][m] (FarHead's camera-aware MLN,
 *    ref: models/utils/misc.py:182-190, models/dense_heads/farhead.py:553-563) so that the FPN output conv writes
 *    the modulated token-major value maps directly.
 * tile: 0 auto (host callers pass the measured choice of far3d_amd/data/tuning_mi355x*.json), else an id of the table in
 *    far3d_amd/csrc/conv_tiles.hpp -- one row per id with its workgroup shape; far3d_conv_tile_caps answers what an id takes.
 *    The families: 1-5 register-staged kernel (any dtype, kernel size and stride).  bf16 x bf16 with Cin % 32 == 0 (LDS-DMA): 1-4,
 *    18, 43-48 ring kernel (any kernel size / stride), 30-35 3x3/s2/p1, 50-139 3x3/s1/p1 LDS-patch kernel, 70-145 1x1/s1 pipelined
 *    GEMMs.  x_dt = FAR3D_DT_BF16_PAIR (w_dt must be FAR3D_DT_F32_BF16X3; y_dt pair or f32; res_dt any): bf16 id + 100 = the same
 *    shape with split products (150-198, 330 / 331), + 200 = the hi halves only (252, 260, 265, 279, 280: ONE bf16 product per term, a
 *    single-bf16 layer inside a pair-stored network).  x_dt = FAR3D_DT_F32, 1x1/s1, Cin % 32 == 0, x 16-byte aligned with strides
 *    that are multiples of 4 floats: 479-481 (auto) with w_dt = FAR3D_DT_F32_BF16X3 -- the pair GEMM on fp32 rows, hi / lo split in
 *    registers; 482-494 with w_dt = FAR3D_DT_F32 -- the EXACT fp32 MFMA on the same kernel (487-494 split K between wave groups inside
 *    the workgroup); the bits of an output row depend on the tile and on Cin only, never on the number of rows in the call.
 *    400-459 (3x3/s1/p1; pair storage, 420-423 bf16) and 460-476 (1x1/s1, pair storage): the PERSISTENT wave-specialised kernels
 *    (csrc/conv_ws.hpp) -- Cin % 32 == 0, Cout % 32 == 0, same storage in and out, 16-byte aligned rows, NO res / y2 (3x3: no
 *    chan_sums either; 1x1: chan_sums when Ho*Wo >= the tile's pixels and Cin >= 64 x the tile's steps per hand-over, input below
 *    2 GB); bit-identical to the pipelined kernels (same products in the same order).
 *    An id the layer cannot use is an error (FAR3D_ERR_ARG, nothing launched), never a silent fallback.
 * chan_sums (optional, DEVICE int64 [N][Cout]; 1x1/s1 layers on a tile with FAR3D_TILE_SUMS, bf16 or pair output, Ho*Wo >= the
 *    tile's pixel count): every STORED output element v (for a pair output: its hi and its lo half) ADDS
 *    rint(v * 2^FAR3D_SUMS_FRAC_BITS) to chan_sums[n][channel] -- the global average pool of VoVNet's eSE block (ref
 *    models/backbones/vovnet.py:173-185) comes out of the concat convolution's epilogue instead of a second pass over its output.
 *    Integer sums are associative: the result does not depend on tile shapes, workgroup order or the number of images in the launch
 *    (bit-identical run to run, hipGraph vs eager, camera-sharded vs single rank) although they are accumulated with atomics.
 *    The caller provides zeros; far3d_ese_nhwc(chan_sums) consumes them and returns them to zero. */
int far3d_conv2d_nhwc(const void* x, int x_dt, const void* w, int w_dt, const float* bias, void* y, int y_dt,
                      int N, int H, int W, int Cin, int ldx, long x_img_stride, int Ho, int Wo, int Cout, int ldy,
                      long y_img_stride, int KH, int KW, int stride, int pad, int act, const void* res, int res_dt,
                      int ldr, long res_img_stride, int Hr, int Wr, void* y2, int y2_dt, int ldy2,
                      long y2_img_stride, const float* y2_scale, const float* y2_shift, long long* chan_sums, int tile,
                      void* stream);

/* One problem of far3d_conv2d_nhwc_grouped: a 3x3 / stride 1 / pad 1 convolution on pair-stored maps with split weights
 * (x_dt = y_dt = FAR3D_DT_BF16_PAIR, w_dt = FAR3D_DT_F32_BF16X3), sizes and strides as in far3d_conv2d_nhwc (Ho = H, Wo = W). */
typedef struct {
  const void* x;             /* (N, H, W) pair-stored map, pixel stride ldx, image stride x_img_stride; channel offset pre-applied */
  const void* w;             /* packed split weights of the layer (rows padded as for far3d_conv2d_nhwc) */
  const float* bias;         /* [Cout padded] or NULL */
  void* y;                   /* (N, H, W) pair-stored output, pixel stride ldy, image stride y_img_stride */
  float* y2;                 /* optional fp32 second output y2 = y2_scale[n][m] * v + y2_shift[n][m] (v: the fp32 value before storage), or NULL */
  const float* y2_scale;     /* [N][Cout] */
  const float* y2_shift;     /* [N][Cout] */
  long x_img_stride, y_img_stride, y2_img_stride;
  int N, H, W, Cin, Cout, ldx, ldy, ldy2;
  int act;                   /* 0 none, 1 relu, 2 swish */
} far3d_conv_problem;
/* problems per far3d_conv2d_nhwc_grouped launch */
#define FAR3D_WS_GROUP_MAX 16

/* n (1..FAR3D_WS_GROUP_MAX) independent 3x3 convolutions (far3d_conv_problem, host array) of ONE Cin as one launch of the persistent
 * wave-specialised kernel: its workgroups walk the concatenated (problem, pixel tile, channel tile) item list, largest problem first.
 * Each output element is bit-identical to the same problem launched by far3d_conv2d_nhwc (every 3x3 tile of the split-product kernels
 * adds the same products in the same order).  tile: 500-559, the workgroup of persistent tile (tile - 100).  Mixed Cin, more than
 * FAR3D_WS_GROUP_MAX problems, unaligned rows or an unknown tile are errors; nothing is launched then. */
int far3d_conv2d_nhwc_grouped(const far3d_conv_problem* probs, int n, int tile, void* stream);

/* What tile id `tile` of far3d_conv2d_nhwc / far3d_conv2d_nhwc_grouped is, for activations x_dt and weights w_dt: a mask of the bits
 * below, or -1 when there is no such tile for that storage (0 = auto is no tile).  Host arithmetic on the table of
 * far3d_amd/csrc/conv_tiles.hpp and the launchers' own compile-time constants; no device needed.  Ids 1-5 exist for every storage
 * far3d_conv2d_nhwc accepts (on bf16 x bf16, 1-4 are the LDS-DMA ring kernel where rows are aligned). */
#define FAR3D_TILE_GEOM 3          /* caps & 3: the layer geometry the tile takes */
#define FAR3D_TILE_ANY 0           /*   any kernel size / stride / padding */
#define FAR3D_TILE_1X1 1           /*   1x1 / stride 1 / pad 0 */
#define FAR3D_TILE_3X3 2           /*   3x3 / stride 1 / pad 1 */
#define FAR3D_TILE_3X3S2 3         /*   3x3 / stride 2 / pad 1 */
#define FAR3D_TILE_STORE(caps) (((caps) >> 2) & 7)   /* input storage: */
#define FAR3D_TILE_BF16 0          /*   bf16 x bf16 */
#define FAR3D_TILE_PAIR 1          /*   pair-stored x split weights */
#define FAR3D_TILE_F32_SPLIT 2     /*   fp32 rows x split weights */
#define FAR3D_TILE_F32 3           /*   fp32 x fp32, exact */
#define FAR3D_TILE_F32_BF16 4      /*   fp32 x bf16 weights (ids 1-5 only) */
#define FAR3D_TILE_HI_ONLY 32      /* pair storage, the hi planes only (one bf16 product per term) */
#define FAR3D_TILE_PERSISTENT 64   /* persistent wave-specialised kernel: bias + activation + store only (no res / y2) */
#define FAR3D_TILE_HAS_GROUP 128   /* tile + 100 launches the same workgroup through far3d_conv2d_nhwc_grouped */
#define FAR3D_TILE_GROUPED 256     /* an id of far3d_conv2d_nhwc_grouped (geometry and storage of tile - 100) */
#define FAR3D_TILE_SUMS 512        /* chan_sums possible (the map must still hold a pixel tile) */
#define FAR3D_TILE_LDS_DMA 1024    /* operands go to LDS by DMA: Cin % 32 == 0 */
#define FAR3D_TILE_PIXELS(caps) ((caps) >> 16)       /* output pixels per workgroup tile */
int far3d_conv_tile_caps(int tile, int x_dt, int w_dt);

/* How a single-problem launch of the persistent 3x3 kernel deals its items to its workgroups (host arithmetic, no device needed; the
 * kernel evaluates the same inline function).  A launch has n_full full items and n_light light ones (the items of a partly empty last
 * channel tile, costed at half a full item).  Returns the k-th item of workgroup wg of grid: 0 .. n_full - 1 = that full item,
 * n_full .. n_full + n_light - 1 = a light item, -1 = the workgroup has fewer than k + 1 items.  Bad arguments (grid < 1, wg outside
 * the grid, negative counts) also return -1. */
int far3d_ws_deal(int n_full, int n_light, int grid, int wg, int k);

/* Multi-head self-attention core: out = softmax(q k^T * scale) v per head (flash-style, no score tensor in HBM).
 * Replaces the bmm/softmax/bmm inside torch.nn.MultiheadAttention as wrapped by mmcv's MultiheadAttention
 *   (ref cfg projects/configs/far3d.py:112-116; call site models/utils/detr3d_transformer.py:385-394; in-tree
 *   statement of the wrapper models/utils/petr_transformer.py:286-326).  The in/out projections are
 *   far3d_conv2d_nhwc calls.
 * q (Aq, heads*32), k/v (Nk, heads*32) of `dtype` (F32 -> exact fp32 MFMA fed from registers, BF16 -> bf16 MFMA), row strides
 * ldq/ldk/ldv elements; out (Aq, heads*32) of dtype out_dt (f32 | bf16), row stride ldo.  head_dim must be 32.
 * The one mask of the inference path -- the "query hole" of the fixed-capacity proposal mode (see FAR3D "hole" below): with
 * hole_count != NULL (DEVICE int32) the keys [hole_start + *hole_count, hole_end) are excluded from every softmax; their K / V
 * rows must hold finite numbers.  hole_count NULL: no mask. */
int far3d_attention_forward(const void* q, const void* k, const void* v, int dtype, void* out, int out_dt, int Aq, int Nk,
                            int heads, int head_dim, int ldq, int ldk, int ldv, int ldo, float scale,
                            const int32_t* hole_count, int hole_start, int hole_end, void* stream);

/* A/B switch for the fp32 instantiation far3d_attention_forward launches (process-wide; tools/probe/attn_f32_ab.py): 0 = the default
 * (register-fed kernel, 64-query workgroups x 4 key parts), 14 / 118 other shapes of it, 4 / 2 the LDS-staged kernel of earlier rounds.
 * Returns the previous value; variant < 0 only reads.  Every variant computes the same products in fp32 (the summation order and
 * the exp differ at the last bit). */
int far3d_attention_f32_variant(int variant);

/* far3d_attention_forward for B samples in ONE launch: the engine's attention kernel with the sample as one more grid index (several
 *   scene streams on one engine, Far3DEngine.decoder_streams).  out[b] has the BITS of far3d_attention_forward on sample b's operands
 *   and hole_count[b], whatever B is: a workgroup moves its q / k / v / out bases by b times the batch stride and runs the one-sample
 *   code.
 * q (B, Aq, heads*32), k/v (B, Nk, heads*32) of `dtype`, row strides ldq/ldk/ldv and batch strides bsq/bsk/bsv in elements (views of
 *   one (B, rows, layers*3*E) QKV buffer are read in place); out (B, Aq, heads*32) of out_dt (f32 | bf16), row stride ldo, batch
 *   stride bso.  dtype, out_dt, head_dim = 32, scale and the alignment rules are far3d_attention_forward's; the batch strides are
 *   16-byte aligned too and not negative.
 * hole_count: NULL (no mask) or a DEVICE int32 array of B counts, one per sample; hole_start / hole_end are shared by all samples:
 *   sample b excludes the keys [hole_start + hole_count[b], hole_end).
 * far3d_attention_f32_variant does NOT apply: this entry always launches the default fp32 form (the register-fed kernel, 64-query
 *   workgroups x 4 key parts), so with a non-default variant set the one-sample entry gives other last bits than this one.
 * Bad arguments (null q/k/v/out, head_dim != 32, B / Aq / Nk / heads < 1, a hole outside [0, Nk], misalignment) return FAR3D_ERR_ARG,
 *   set far3d_last_error() and launch nothing. */
int far3d_attention_streams(const void* q, const void* k, const void* v, int dtype, void* out, int out_dt, int B, int Aq, int Nk,
                            int heads, int head_dim, int ldq, int ldk, int ldv, int ldo, long bsq, long bsk, long bsv, long bso,
                            float scale, const int32_t* hole_count, int hole_start, int hole_end, void* stream);

/* Batched, masked multi-head attention core: per sample b and head h
 *   out[b] = softmax(q[b] k[b]^T * scale + M[b,h] + P[b]) v[b]      (flash-style, no score tensor in HBM; ONE launch for all samples).
 * The attention of torch.nn.MultiheadAttention with `attn_mask` and `key_padding_mask`, as mmcv's wrapper calls it for any batch size
 *   (call site models/utils/detr3d_transformer.py:385-394; the mask is the one models/dense_heads/farhead.py `prepare_for_dn` builds).
 *   far3d_attention_forward stays the engine's one-sample kernel; this entry does not know the engine's key hole.
 * q (B, Aq, heads*32), k/v (B, Nk, heads*32) of `dtype` (F32 -> exact fp32 MFMA, BF16 -> bf16 MFMA): row strides ldq/ldk/ldv and batch
 *   strides bsq/bsk/bsv in elements (views of one (B, rows, 768) QKV buffer are read in place); out (B, Aq, heads*32) of out_dt
 *   (f32 | bf16), row stride ldo, batch stride bso.  head_dim must be 32.  Pointers, row and batch strides 16-byte aligned.
 * attn_mask, mask_kind: 0 = none (attn_mask ignored); 1 = bytes with torch.bool semantics, nonzero = the key is EXCLUDED for that query;
 *   2 = f32 added to the scaled scores (may hold -inf).  One (Aq, Nk) matrix with row stride ldm >= Nk per (sample, head) pair, matrix
 *   b * heads + h at attn_mask + (b * heads + h) * mask_bstride elements -- the (B*heads, Aq, Nk) layout of torch; mask_bstride = 0: one
 *   matrix shared by all samples and heads.
 * key_padding (optional, NULL = none): (B, Nk) contiguous bytes, nonzero = the key is excluded for every query of the sample.
 * A query whose keys are all excluded gets NaN in every element of its row (torch: 0 / 0); other rows are unaffected.  K / V rows of
 *   excluded keys must hold finite numbers (an excluded probability is an exact 0 that still multiplies V).
 * Probabilities are exp2((s - m) * log2e) with the running maximum m subtracted first; far3d_attention_f32_variant is not read.  The
 *   bits of sample b depend on its own operands only (not on B).
 * Bad arguments (null q/k/v/out, head_dim != 32, B / Aq / Nk / heads < 1, unknown mask_kind, ldm < Nk, misalignment) return
 *   FAR3D_ERR_ARG, set far3d_last_error() and launch nothing. */
int far3d_attention_batched(const void* q, const void* k, const void* v, int dtype, void* out, int out_dt, int B, int Aq, int Nk,
                            int heads, int head_dim, int ldq, int ldk, int ldv, int ldo, long bsq, long bsk, long bsv, long bso,
                            float scale, const void* attn_mask, int mask_kind, int ldm, long mask_bstride,
                            const uint8_t* key_padding, void* stream);

/* y = act(LayerNorm_C(x) * gamma + beta); optional y2 = y + add (next GEMM's "query + query_pos").
 * Replaces nn.LayerNorm at ref models/utils/detr3d_transformer.py:304-307,398-400,506-512 and
 * models/dense_heads/farhead.py:230-239,274-277.  x,y,add,y2: f32 rows with strides ldx,ldy,lda,ldy2 (multiples of 4);
 * gamma/beta may be NULL (no affine).  act: 0 none, 1 ReLU.  C multiple of 4, <= 1024.  y2 has dtype y2_dt (f32 | bf16);
 * yb (optional) receives a copy of y in dtype yb_dt (f32 | bf16; row stride ldyb) -- the next GEMM's operands without a
 * conversion pass; y2 and yb may be the two halves of one [y+add | y] row (merged-GEMM input). */
int far3d_layernorm(const float* x, const float* gamma, const float* beta, float* y, int rows, int C, int ldx,
                    int ldy, float eps, int act, const float* add, int lda, void* y2, int ldy2, int y2_dt, void* yb, int ldyb,
                    int yb_dt, void* stream);
/* far3d_layernorm with a ROW MAP for the two GEMM-operand outputs: row i of y2 / yb is stored at row out_rows[i] (y itself stays in
 * place).  The exact-fp32 decoder uses it to hand the aggregation's logit / offset GEMM its operand rows in the aggregation kernel's
 * launch order (far3d_agg_order's inv), so that the GEMM's output is in that order with no change to the GEMM.  out_rows (rows) int32
 * DEVICE, a permutation of [0, rows) (or any injective map into the caller's buffers). */
int far3d_layernorm_rows(const float* x, const float* gamma, const float* beta, float* y, int rows, int C, int ldx,
                         int ldy, float eps, int act, const float* add, int lda, void* y2, int ldy2, int y2_dt, void* yb, int ldyb,
                         int yb_dt, const int32_t* out_rows, void* stream);

/* ROW-RESIDENT CHAINS of a decoder layer (bf16 decoder, embed dims 256, FFN hidden 1024): the row-local work between the
 * attention core and the aggregation kernel, and between the aggregation kernel and the next layer's attention core, in one
 * launch each -- a workgroup owns 16 query rows, keeps them in LDS across projections / residuals / LayerNorms and streams the
 * weights from L2 in MFMA fragment order.  They replace sequences of far3d_conv2d_nhwc + far3d_layernorm calls (the default
 * path of far3d_amd.engine, which stays available) and compute the same arithmetic: bf16 operands, fp32 accumulation, epilogue
 * order bias -> activation -> residual, far3d_layernorm's reduction tree; only the K order of the fp32 accumulation differs.
 * Rows never interact: a row's result does not depend on M or on the rows launched with it.
 * Packed weights: a (N, K) bf16 row-major weight (K % 256 == 0, rows zero-padded to a multiple of 16) re-ordered to
 * [N / 16][K / 32][64 lanes][8]: element j of lane l of (tile t, step s) is W[16 t + (l & 15)][32 s + 8 (l >> 4) + j]
 * (far3d_amd.ops.pack_rowchain).  Biases are f32 and cover the padded rows.  All pointers 16-byte aligned, row strides in
 * elements (bf16 rows: multiples of 8, f32 rows: multiples of 4).
 *
 * far3d_rowchain_attn_out: x1 = LN0(att W_out^T + b_out + x);  ul = [x1 + qpos | x1] W_wl^T + b_wl.
 *   Replaces the self-attention output projection + residual + norm (ref models/utils/detr3d_transformer.py:385-400) and the
 *   attention-weight / key-point-offset linears of the aggregation (:522-531; merged into one (n_wl, 512) weight whose first
 *   256 input columns see query + query_pos and whose last 256 see the query, as in the unfused path).
 *   att (M,256) bf16; x, qpos (M,256) f32; x1 (M,256) f32 out; ul (M, n_wl) f32 out, 448 < n_wl <= 464. */
int far3d_rowchain_attn_out(const void* att, int ld_att, const float* x, int ldx, const float* qpos, int ldq,
                            const void* w_out, const float* b_out, const float* g0, const float* be0,
                            const void* w_wl, const float* b_wl, int n_wl, float* x1, int ldx1, float* ul, int ldu,
                            const int32_t* ul_rows, int M, float eps, void* stream);
/*   ul_rows: optional (M) int32 DEVICE -- row i of the logits / offsets is stored at row ul_rows[i] of `ul` (far3d_agg_order's inv:
 *   the aggregation kernel's launch order); NULL = row i. */

/* far3d_rowchain_ffn: x2 = LN1(agg W_o^T + b_o + x1);  out = LN2(relu(x2 W_1^T + b_1) W_2^T + b_2 + x2);
 *   with w_qkv: qkv = [out + qpos | out] W_qkv^T + b_qkv (bf16; the NEXT layer's merged q / k / v in-projection).
 *   Replaces the aggregation's output projection + residual (ref detr3d_transformer.py:566-569), norm, FFN, norm (:398-422)
 *   and the next layer's in-projection (:378-384).  agg (M,256) bf16; x1, qpos (M,256) f32; out (M,256) f32;
 *   qkv (M,768) bf16 or NULL with w_qkv NULL; xop (optional, M x 512 bf16): [out + qpos | out], the operand the unfused
 *   in-projection reads. */
int far3d_rowchain_ffn(const void* agg, int ld_agg, const float* x1, int ldx1, const float* qpos, int ldq,
                       const void* w_o, const float* b_o, const float* g1, const float* be1,
                       const void* w_1, const float* b_1, const void* w_2, const float* b_2,
                       const float* g2, const float* be2, const void* w_qkv, const float* b_qkv,
                       float* out, int ldo, void* qkv, int ldqkv, void* xop, int ldxop, int M, float eps, void* stream);

/* far3d_rowchain_qkv: qkv = [x + qpos | x] W_qkv^T + b_qkv (bf16), the in-projection alone -- the operand is built and the GEMM
 *   run by the code of far3d_rowchain_ffn's tail, so for the same x (that kernel's `out`) and qpos the result is BIT-IDENTICAL
 *   to the tail's.  For the query-sharded decoder, where a layer's output rows exist on every rank only after the exchange.
 *   x, qpos (M,256) f32; qkv (M,768) bf16. */
int far3d_rowchain_qkv(const float* x, int ldx, const float* qpos, int ldq, const void* w_qkv, const float* b_qkv,
                       void* qkv, int ldqkv, int M, void* stream);

/* far3d_rowchain_branches: the shared classification and regression branches over the decoder outputs of all layers,
 *   cls = L2(relu(LN(L1(relu(LN(L0(h)))))));  reg = L2'(relu(L1'(relu(L0'(h)))))   (L: 256 -> 256 linears, the last ones -> n_cls / n_reg)
 *   Replaces 6 far3d_conv2d_nhwc + 2 far3d_layernorm launches (ref models/dense_heads/farhead.py:230-245, applied at :646-664).
 *   h (M,256) bf16; cls (M, n_cls) f32, reg (M, n_reg) f32, n_cls, n_reg <= 32; weights packed as above (the last linears as TWO
 *   16-row tiles, zero rows past their outputs), biases covering 32 rows. */
int far3d_rowchain_branches(const void* h, int ldh, const void* w_c0, const float* b_c0, const float* g_c0, const float* be_c0,
                            const void* w_c1, const float* b_c1, const float* g_c1, const float* be_c1,
                            const void* w_c2, const float* b_c2, int n_cls, const void* w_r0, const float* b_r0,
                            const void* w_r1, const float* b_r1, const void* w_r2, const float* b_r2, int n_reg,
                            float* cls, int ld_cls, float* reg, int ld_reg, int M, float eps, void* stream);

/* VoVNet eSE block on NHWC maps: y = x * hsigmoid(fc(mean_hw(x))) (+ identity).
 * Replaces eSEModule + the identity add, ref models/backbones/vovnet.py:173-185,232-236.
 * x,identity,y: NHWC `dt` with (pixel stride, image stride) pairs; fcw (C,C) f32 row-major, fcb (C) f32;
 * scratch: device workspace of FAR3D_SUMS_SCRATCH_FLOATS(N, C) floats; never needs zeroing.  The average pool writes
 * per-workgroup partial channel sums with plain stores and the gate kernel adds them in index order, so the sums are
 * deterministic: no atomics, bit-identical run to run and hipGraph vs eager.  C a multiple of 4, <= 1024.
 * chan_sums (optional, bf16 / pair maps): the fixed-point channel sums [N][C] that far3d_conv2d_nhwc accumulated while it wrote x;
 * the pooling pass is skipped, the gate is computed from them and the apply kernel returns them to zero for the next producer. */
int far3d_ese_nhwc(const void* x, int dt, const float* fcw, const float* fcb, const void* identity, void* y,
                   float* scratch, int N, int HW, int C, int ldx, long x_img_stride, int ldi, long i_img_stride,
                   int ldy, long y_img_stride, long long* chan_sums, void* stream);

/* The same block for maps whose channel sums came out of the concat convolution (chan_sums REQUIRED; dt bf16 or pair), with the stage-end
 * pooling of ref models/backbones/vovnet.py:249-250 fused into the apply pass: the gate launch of far3d_ese_nhwc, then ONE streaming launch
 * that writes y = x * gate (+ identity) in 16-byte pieces and, pooled != NULL, MaxPool2d(3, 2, ceil_mode=True)(y) ((Hp, Wp) its ceil-mode
 * size) computed from x with every tap rounded to the storage format first -- bit-identical to far3d_maxpool3x3s2_nhwc of the stored y.
 * y == NULL: only the pooled map is written (the caller needs the stage output at half resolution only).
 * gate: N*C floats of workspace (16-byte aligned); chan_sums come back zeroed.
 * C % 8 == 0 (pair: % 32), <= 1024; every pointer / stride a multiple of 16 bytes. */
int far3d_ese_fused_nhwc(const void* x, int dt, const float* fcw, const float* fcb, const void* identity, void* y, void* pooled,
                         float* gate, int N, int H, int W, int C, int ldx, long x_img_stride, int ldi,
                         long i_img_stride, int ldy, long y_img_stride, int Hp, int Wp, int ldp, long p_img_stride,
                         long long* chan_sums, void* stream);

/* GroupNorm(groups, C) (+ReLU) on dense NHWC maps.  Replaces nn.GroupNorm(32, 256)+ReLU of the depth head,
 * ref models/depth_predictor/depth_predictor.py:43-45.  scratch: FAR3D_SUMS_SCRATCH_FLOATS(N, C) floats (no zeroing needed);
 * statistics are reduced deterministically from per-workgroup partial sums. */
int far3d_groupnorm_nhwc(const void* x, int dt, const float* gamma, const float* beta, void* y, float* scratch, int N,
                         int HW, int C, int groups, float eps, int relu, void* stream);

/* MaxPool2d(kernel 3, stride 2, ceil_mode=True), dense NHWC input, output with pixel stride ldy / image stride
 * y_img_stride (so it can land in the first C channels of the next OSA concat buffer)
 * (ref models/backbones/vovnet.py:249-250). */
int far3d_maxpool3x3s2_nhwc(const void* x, int dt, void* y, int N, int H, int W, int C, int Ho, int Wo, int ldy,
                            long y_img_stride, void* stream);

/* Depthwise 3x3 convolution, pad 1, stride 1 or 2, no bias, no activation: nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False), the
 * first half of the `dw_conv3x3` layers of VoVNet's depthwise specs (ref models/backbones/vovnet.py:100-121; the pointwise 1x1 + BN +
 * ReLU that follows is a far3d_conv2d_nhwc call -- there is no nonlinearity between the two).
 * x, y: NHWC maps of storage `dt` with dense rows, pixel strides ldx / ldy and image strides in stored elements, pointers pre-offset to
 * the first channel (channel slices of wider buffers are fine).  dt: FAR3D_DT_F32 or FAR3D_DT_BF16 with C % 8 == 0, FAR3D_DT_BF16_PAIR
 * with C % 32 == 0 (hi + lo read, the fp32 result stored split).  w: [9][C] f32, w[ky*3 + kx][c] = weight[c][0][ky][kx].
 * Ho = (H-1)/stride + 1, Wo = (W-1)/stride + 1.  Every pointer and stride a multiple of 16 bytes.  x and y must not overlap.
 * fp32 accumulation in the fixed tap order (0,0) ... (2,2) with pinned fmas: the bits of an output element depend on its own window
 * and weights only, never on N or the launch's other pixels.  The kernel is far3d_dwconv3x3_act_nhwc's, instantiated with one weight
 * set and without bias and activation code; both entries run the same argument checks.  Bad arguments return FAR3D_ERR_ARG and launch
 * nothing. */
int far3d_dwconv3x3_nhwc(const void* x, int dt, const float* w, void* y, int N, int H, int W, int C, int ldx, long x_img_stride,
                         int Ho, int Wo, int ldy, long y_img_stride, int stride, void* stream);

/* far3d_dwconv3x3_nhwc with a bias, an activation and one or two weight sets per window: the depthwise half of mmcv's
 * DepthwiseSeparableConvModule (conv + BN + activation, BN folded by the caller) as the light YOLOX towers use it
 * (ref models/dense_heads/yolox_head.py:197-219).  y[..., r*C + c] = act(dw(x[..., c]; w[r]) + bias[r][c]) for r < reps: the output map
 * has reps*C logical channels (ldy >= reps*C stored channels), and with reps = 2 both towers' first layers read their common FPN map once.
 * Operand rules of far3d_dwconv3x3_nhwc (storage, C % 8 / C % 32, pad 1, stride 1 or 2, 16-byte alignment, no overlap).
 * w: [reps][9][C] f32; bias: [reps][C] f32 or NULL; reps: 1 or 2; act: 0 none / 1 ReLU / 2 Swish (x * sigmoid(x), full-precision expf).
 * Arithmetic: the nine pinned fmas of far3d_dwconv3x3_nhwc in its tap order, then one fp32 add of the bias (none when bias is NULL), then
 * the activation -- the bits of an output element depend on its own window, weights and bias only, never on N, the launch's other pixels
 * or reps; reps = 1, bias = NULL, act = 0 returns far3d_dwconv3x3_nhwc's bits.  Bad arguments return FAR3D_ERR_ARG and launch nothing. */
int far3d_dwconv3x3_act_nhwc(const void* x, int dt, const float* w, const float* bias, void* y, int N, int H, int W, int C, int ldx,
                             long x_img_stride, int Ho, int Wo, int ldy, long y_img_stride, int stride, int reps, int act, void* stream);

/* A depthwise-separable layer as ONE launch: y = act2( W_pw . round_storage( act1( dw3x3(x; w9) + b1 ) ) + b2 ), i.e.
 * far3d_dwconv3x3_act_nhwc (one weight set) followed by the pointwise 1x1 far3d_conv2d_nhwc, without the scratch map between them.
 * x, y: NHWC views under the operand rules of far3d_dwconv3x3_act_nhwc (16-byte alignment, ldx / ldy / image strides in stored
 * elements, channel slices of wider buffers, pad 1, stride 1 or 2, Ho = (H-1)/stride + 1, Wo = (W-1)/stride + 1); x and y must not
 * overlap (disjoint channel slices of one buffer with a common pixel stride are fine).  dt: FAR3D_DT_BF16 with w_dt = FAR3D_DT_BF16
 * (bf16 MFMA), or FAR3D_DT_BF16_PAIR with w_dt = FAR3D_DT_F32_BF16X3 (the split products hi.hi + hi.lo + lo.hi); y has x's storage.
 * C % 32 == 0, Cout % 32 == 0, Cout <= 256.  w9: [9][C] f32; b1: [C] f32 or NULL; w_pw, b2: the packed weights (rows >= Cout + 256,
 * Cin padded to 32; split weights as [32 hi | 32 lo] per 32-channel block) and padded bias (or NULL) of a 1x1 far3d_conv2d_nhwc layer;
 * act1, act2: 0 none / 1 ReLU / 2 Swish (full-precision expf).
 * Depthwise half: the nine pinned fmas of far3d_dwconv3x3_nhwc in its tap order, the bias add, the activation, then the rounding of
 * that kernel's store (bf16 round-to-nearest-even; pair hi = bf16(v), lo = bf16(v - hi); vector load, activation and rounding are one
 * source for both kernels, csrc/dw_core.hpp) -- the MFMA operand holds bit for bit what
 * the two-launch path writes to its scratch map; only the accumulation order of the pointwise sums differs from far3d_conv2d_nhwc.
 * Anything else (f32 storage, other sizes, overlap, misalignment) returns FAR3D_ERR_ARG and launches nothing. */
int far3d_dwsep_conv_nhwc(const void* x, int dt, const float* w9, const float* b1, int act1, const void* w_pw, int w_dt, const float* b2,
                          int act2, void* y, int N, int H, int W, int C, int ldx, long x_img_stride, int Ho, int Wo, int Cout, int ldy,
                          long y_img_stride, int stride, void* stream);

/* NCHW fp32 image (N,3,H,W) -> NHWC (N,Ho,Wo,32) im2col of the stride-2 3x3 stem conv: channel = (ky*3+kx)*3 + c for the
 * 27 taps, 5 zero channels; Ho = (H-1)/2+1.  The first VoVNet conv (ref models/backbones/vovnet.py:306-311) then runs as
 * a K=32 far3d_conv2d_nhwc 1x1. */
int far3d_stem_im2col(const float* img, void* out, int out_dt, int N, int H, int W, void* stream);

/* The same convolution in ONE launch for bf16 engines: y = act(conv3x3 / stride 2 / pad 1 (img) + bias) with the folded-BN weights of
 * VoVNet's first stem layer, read straight from the NCHW fp32 image -- the im2col map is never written.  w: bf16 [>= 64][32] rows of the
 * layer packed like far3d_stem_im2col's consumer (k = (ky*3 + kx)*3 + c, 5 zero columns), bias [64] f32 or NULL; y: bf16 NHWC
 * (N, Ho, Wo, 64 channels) with pixel stride ldy, Ho = (H-1)/2+1, Wo = (W-1)/2+1; act 0 none / 1 ReLU.  Same products in the same order as
 * far3d_stem_im2col + far3d_conv2d_nhwc (bit-identical output).  Replaces ref models/backbones/vovnet.py:306-311 (stem_1). */
int far3d_stem_conv(const float* img, const void* w, const float* bias, void* y, int N, int H, int W, int ldy, long y_img_stride,
                    int act, void* stream);

/* 2D proposal scoring + ordered fixed-capacity selection (no host sync).
 * Replaces YOLOXHeadCustom.get_bboxes' score / 3x3-peak / threshold steps, ref models/dense_heads/yolox_head.py:426-438,
 * and its boolean-mask indexing :452-467.  cls[l] (N,h,w,ncls) f32 logits, reg[l] (N,h,w,nreg) f32 with channels
 * (dx,dy,log w,log h,objectness) -- HOST arrays of L device pointers.  level_hw (L,2), strides (L) int32 HOST.
 * scratch_sw, weights: (N,S) f32 device; weights receives sample_weight*(sample_weight==maxpool3x3).
 * mode 0: keep weights > thr (first `cap` in flat-index order); mode 1: the cap largest per camera (ties -> lower index).
 * sel_idx (N,cap) int32 ascending flat indices (camera-local, level-major), sel_cnt (N) int32. */
int far3d_proposal_select(const float* const* cls, const float* const* reg, int ncls, int nreg, int N, int L,
                          const int32_t* level_hw, const int32_t* strides, float* scratch_sw, float* weights, int* sel_idx,
                          int* sel_cnt, int cap, float thr, int mode, void* stream);

/* Adaptive-query construction from the selected 2D peaks: 2D box decode (ref yolox_head.py:491-501 + xyxy->cxcywh :457),
 * depth bin argmax at round(centre/stride) (ref models/dense_heads/farhead.py:736-747), LID un-binning (:521-527),
 * un-projection with img2lidar = inverse(lidar2img) and pc_range normalisation (:792-811), context = value-map token ||
 * log-odds(score) - log-odds(thr) (:576-581,773-784; the score is clamped to >= 1e-6 first so that zero-weight padding rows
 * of the static top-K mode stay finite).  Camera n's rows start at sum(sel_cnt[:n]) (camera-major, like the reference).
 * Outputs: ref2d (M,3), ctx (M,C+1), box2d (M,4 cxcywh), score (M).
 * FIXED-CAPACITY MODE (rows_total > 0; the reference's data-dependent M = sum(sel_cnt), ref yolox_head.py:429-458, farhead.py:
 * 576-581, without a host sync and with static shapes -- "cap + count"): the outputs have rows_total rows; rows [0, M) are
 * the proposals in the reference's order, rows [M, rows_total) are zero-filled and form the HOLE that the consumers
 * mask: *m_out = min(M, rows_total) (DEVICE int32; the `hole_count` of far3d_attention_forward / far3d_head_finalize /
 * far3d_agg_order), *overflow_out = 1 when proposals were dropped (M > rows_total) or a camera filled its `cap` (peaks may have
 * been lost in far3d_proposal_select), else 0 -- the host checks it after the fact instead of syncing on M.
 * rows_total = 0: legacy behaviour (rows past M untouched; m_out / overflow_out must be NULL). */
int far3d_proposal_gather(const float* const* reg, int nreg, int N, int L, const int32_t* level_hw, const int32_t* strides,
                          const int* sel_idx, const int* sel_cnt, int cap, const float* weights,
                          const float* depth_logit, int hd, int wd, int nd, int depth_stride, float depth_min,
                          float depth_max, int depth_bins, const float* img2lidar, const void* feat, int feat_dt, int C,
                          const float* pc_range, float score_thr, float* ref2d, float* ctx, float* box2d, float* score,
                          int rows_total, int32_t* m_out, int32_t* overflow_out, void* stream);

/* Multi-depth 2D proposals (ref farhead.py:754-805, multi_depth_config.topk = K in [2, 8]), part 1 of 2, per camera block: the
 * primary rows exactly as far3d_proposal_gather writes them (bit for bit), plus a record per primary for part 2:
 * md_flags (rows) int32 = 1 when the primary's best depth bin >= range_min_bin; md_info (rows, 2K) int32 = camera, the K best bins
 * (by logit, lower bin first on ties; the first is far3d_proposal_gather's bin), then the K-1 ratios p_k / p_0 of the fp32 softmax
 * probabilities (float bits).  primary_rows > 0: rows past it are dropped (fixed capacity); 0: N * cap rows.  nd <= 256.
 * Writes no count, flag or hole: far3d_proposal_extra_rows does, after every camera's primaries exist. */
int far3d_proposal_gather_md(const float* const* reg, int nreg, int N, int L, const int32_t* level_hw, const int32_t* strides,
                             const int* sel_idx, const int* sel_cnt, int cap, const float* weights,
                             const float* depth_logit, int hd, int wd, int nd, int depth_stride, float depth_min,
                             float depth_max, int depth_bins, const float* img2lidar, const void* feat, int feat_dt, int C,
                             const float* pc_range, float score_thr, float* ref2d, float* ctx, float* box2d, float* score,
                             int primary_rows, int topk, int range_min_bin, int32_t* md_flags, int32_t* md_info, void* stream);

/* Multi-depth 2D proposals, part 2 of 2, all cameras: with Mp = min(sum sel_cnt, primary_rows) primaries in rows [0, Mp) and V of
 * them valid, rows [Mp, Mp + (K-1) V) receive the extra rows in the reference's k-major order (k = 1 .. K-1, valid primaries in
 * row order): the primary's box2d / score / ctx[:C], ctx[C] = its log-odds * p_k / p_0, ref2d from the box centre, bin k's depth
 * and the camera's img2lidar.  Rows past rows_total are dropped in that order.  fill_hole: zero rows [M', rows_total).
 * m_out (optional) = M' = min(Mp + (K-1) V, rows_total); overflow_out (optional) = 1 when a row was dropped (sum sel_cnt >
 * primary_rows, M' > rows_total, or -- sel_cap > 0 -- a camera reached its selection capacity sel_cap), else 0.  The grid depends
 * on primary_rows only; no host sync. */
int far3d_proposal_extra_rows(const int* sel_cnt, int N, int sel_cap, int primary_rows, int topk, const int32_t* md_flags,
                              const int32_t* md_info, const float* img2lidar, float depth_min, float depth_max, int depth_bins,
                              const float* pc_range, int C, float* ref2d, float* ctx, float* box2d, float* score, int rows_total,
                              int fill_hole, int32_t* m_out, int32_t* overflow_out, void* stream);

/* Ordered stream compaction of a token mask (far3d_amd/csrc/foreign.hip): the selection of a FOREIGN 2D head -- the reference's
 * `valid_indices` -- in the form the proposal kernels consume.  Replaces the boolean-mask indexing feat_flatten[valid_indices]
 * (ref models/dense_heads/farhead.py:578-579; yolox_head.py:454,467).  valid (N,S): one byte per token, non-zero = selected
 * (torch.bool storage as it is); any N >= 1, any S >= 1 (no alignment asked of S or of the pointer).
 * sel_idx (N,cap) int32: the first min(count_n, cap) selected flat indices of camera n, ascending (entries past that are not
 * written); sel_cnt (N) int32 = min(count_n, cap); *overflow_out (optional, DEVICE int32) = 1 when some count_n > cap, else 0: it is
 * cleared by a 4-byte memset on `stream` in front of the launch, and the workgroups that overflow all store the same 1.
 * One kernel launch of N workgroups (the grid depends on N only, the loop on S); no host sync; no atomics. */
int far3d_mask_compact(const uint8_t* valid, int N, int S, int* sel_idx, int* sel_cnt, int cap, int32_t* overflow_out, void* stream);

/* Adaptive-query rows from GIVEN 2D boxes (far3d_amd/csrc/foreign.hip; ref farhead.py:711-827): far3d_proposal_gather /
 * far3d_proposal_gather_md without the box decode.  boxes (rows,4) f32 cx,cy,w,h in padded-image pixels, camera-major: camera n's
 * boxes are rows [sum box_cnt[:n], + box_cnt[n]); box_cnt (N) int32 DEVICE; scores (rows) f32, row-aligned with boxes.  The j-th box
 * of camera n pairs with token sel_idx[n,j] of far3d_mask_compact (sel_idx (N,cap), sel_cnt (N)); S = tokens per camera.
 * depth: f32 map of nd = depth_bins + 1 values per cell, depth_layout 0 = (N,hd,wd,nd), 1 = (N,nd,hd,wd) (the reference's
 * pred_depth as it is); depth_is_prob 0 = logits, 1 = probabilities (the bins are ranked on the values either way).  nd <= 256.
 * Per row: the depth cell round(centre / depth_stride), half to even, clamped to the map (:736-742) -- the rule of
 * far3d_proposal_gather; the best bin, lowest bin on ties; LID un-binning (:521-527); un-projection with img2lidar (N,4,4) and
 * pc_range normalisation (:792-811) -> ref2d (rows,3); ctx (rows,C+1) = the token feat[n, sel_idx[n,j], :] (feat (N,S,C) f32|bf16)
 * || log-odds(max(score,1e-6)) - log-odds(score_thr) (:773-784).  Output row = input row.
 * topk = 1: md_flags / md_info are not touched (may be NULL).  topk = K in 2 ... 8: every written row also leaves its record in
 * md_flags (rows) / md_info (rows,2K), the layout of far3d_proposal_gather_md: flag = best bin >= range_min_bin; camera, the K best
 * bins, the K-1 ratios p_k / p_0 (float bits) -- for a probability map the quotient of the two map values, for logits
 * (e_k / s) / (e_0 / s) of the fp32 softmax exactly as far3d_proposal_gather_md forms them.  Run far3d_proposal_extra_rows next with
 * primary_rows = sum box_cnt and boxes / scores as its box2d / score (buffers of rows_total rows, the extra rows' copies are appended).
 * Fed with far3d_proposal_gather(_md)'s own box2d, score, sel_idx, sel_cnt and its logits, ref2d / ctx / records are the same bit for bit.
 * *mismatch_out (optional, DEVICE int32) = 1 when box_cnt[n] != sel_cnt[n] for some camera, else 0; rows are then still written for
 * min(box_cnt[n], sel_cnt[n]) boxes per camera (never past `rows`), and the host refuses the frame.  Rows of boxes past the counts are
 * not touched.  One launch whose grid depends on cap and N only; no host sync; no atomics. */
int far3d_proposal_from_boxes(const float* boxes, const int* box_cnt, const float* scores, int rows, const int* sel_idx,
                              const int* sel_cnt, int cap, int N, int S, const float* depth, int depth_layout, int depth_is_prob,
                              int hd, int wd, int nd, int depth_stride, float depth_min, float depth_max, int depth_bins,
                              const float* img2lidar, const void* feat, int feat_dt, int C, const float* pc_range, float score_thr,
                              float* ref2d, float* ctx, int topk, int range_min_bin, int32_t* md_flags, int32_t* md_info,
                              int32_t* mismatch_out, void* stream);

/* Proposals of camera BLOCKS -> the frame's layout (far3d_amd/csrc/md_blocks.hip).  nblocks (1 .. 16) blocks in ascending camera
 * order, block b = cameras [first_cam[b], first_cam[b] + block_cams[b]) (contiguous, together all N), each processed on its own by
 * far3d_proposal_gather / far3d_proposal_gather_md into its own buffers of block_rows[b] rows, whose rows [0, count_b) hold its
 * primaries camera-major.  ref2d / ctx / box2d / score / md_flags / md_info / sel_cnt / count_dev / overflow are HOST arrays of
 * nblocks DEVICE pointers; count_b = *count_dev[b] when that pointer is given, else count_host[b] when count_host is given and
 * >= 0 (static top-K), else min(sum sel_cnt of the block, block_rows[b]) (what far3d_proposal_gather_md kept; a sum above
 * block_rows[b] counts as that block's overflow flag); it is clamped to [0, block_rows[b]].  count_dev, count_host, overflow and their entries may be NULL.
 * Writes, with Mp = min(sum count_b, primary_rows): rows [0, Mp) of the frame's o_ref2d (rows_total,3), o_ctx (rows_total,C+1),
 * o_box2d (rows_total,4), o_score (rows_total) = the blocks' rows back to back; o_sel_cnt (N) = the blocks' sel_cnt;
 * *m_out = Mp; *overflow_out = OR of the blocks' flags | (sum count_b > primary_rows) (both optional).
 * Records given (md_flags, md_info, o_md_flags (primary_rows), o_md_info (primary_rows, 2 topk) all non-NULL; multi-depth): rows
 * [0, Mp) of the records too, the camera field of md_info rebased by first_cam[b]; rows [Mp, rows_total) are NOT touched -- run
 * far3d_proposal_extra_rows next, which writes the extra rows, M', the final flag and the hole.  Records NULL (single depth): rows
 * [Mp, rows_total) are zero-filled, the result is that of far3d_proposal_gather(rows_total) on all cameras.
 * Equal to the all-camera call bit for bit when block_rows[b] >= min(primary_rows, block_cams[b] * cap).  One launch whose grid
 * depends on the static sizes only; no atomics, no order between workgroups, no host sync.  The frame's buffers must not overlap a
 * block's. */
int far3d_proposal_merge_blocks(int nblocks, const float* const* ref2d, const float* const* ctx, const float* const* box2d,
                                const float* const* score, const int32_t* const* md_flags, const int32_t* const* md_info,
                                const int32_t* const* sel_cnt, const int32_t* const* count_dev, const int32_t* count_host,
                                const int32_t* const* overflow, const int32_t* first_cam, const int32_t* block_cams,
                                const int32_t* block_rows, int N, int C, int topk, int primary_rows, int rows_total,
                                float* o_ref2d, float* o_ctx, float* o_box2d, float* o_score, int32_t* o_md_flags,
                                int32_t* o_md_info, int32_t* o_sel_cnt, int32_t* m_out, int32_t* overflow_out, void* stream);

/* One multi-depth camera block -> ONE contiguous record of 4-byte words (far3d_amd/csrc/md_blocks.hip): what a rank of the
 * camera-sharded runner puts into the frame's exchange, and what far3d_proposal_merge_blocks then reads in place on every rank.
 * The block: `cams` cameras (0 .. per; 0 = the empty block of an idle rank, every source NULL and block_rows 0) processed by
 * far3d_proposal_gather_md into buffers of block_rows rows (<= rows).  The record: `per` camera slots and `rows` rows, sections in
 * this order, each starting on a 16-byte boundary (record_words must equal the end of the last one, rounded up to 4 words):
 *   header[4] = (cams, count, overflow flag, 0) | sel_cnt[per] | img2lidar[per*16] | ref2d[rows*3] | ctx[rows*(C+1)] |
 *   box2d[rows*4] | score[rows] | md_flags[rows] | md_info[rows*2*topk]
 * count = count_host when >= 0 (static top-K: cams * K), else min(sum sel_cnt, block_rows), and then the flag is
 * (sum sel_cnt > block_rows); *overflow_in (optional device int32) is OR-ed into the flag.  The same rule as
 * far3d_proposal_merge_blocks.  Exactly `count` rows of every array and `cams` entries of sel_cnt / img2lidar are copied; every
 * other word of the record -- padding slots, rows past the count, alignment gaps -- is zero: the record is a function of the valid
 * rows alone (the empty block's is all zeros) and safe to replay from a graph.  md_info keeps the block's own camera indices (the
 * merge rebases them).  One launch whose grid depends on the static sizes only; no host sync.  The record must be 16-byte aligned
 * and must not overlap a source. */
int far3d_proposal_pack_block(int cams, int per, int block_rows, int rows, int C, int topk, const int32_t* sel_cnt,
                              const float* img2lidar, const float* ref2d, const float* ctx, const float* box2d, const float* score,
                              const int32_t* md_flags, const int32_t* md_info, int count_host, const int32_t* overflow_in,
                              float* record, long record_words, void* stream);

/* Blocks of rows -> one compact run (camera-sharded fixed-capacity mode): src (nblocks, rows_per_block, D) f32 of which the first
 * counts[b] rows of block b are valid; dst (dst_rows, D): rows [0, M) the valid rows in block order, the rest zero,
 * *m_out = M = min(sum counts, dst_rows); *overflow_out is OR-ed with (sum counts > dst_rows) (initialise it). */
int far3d_compact_rows(const float* src, const int32_t* counts, int nblocks, int rows_per_block, int D, float* dst, int dst_rows,
                       int32_t* m_out, int32_t* overflow_out, void* stream);

/* y[r] = gamma[r] * LN_noaffine(x[r]) + beta[r] (+ add[r]);  C = 256.  ldg / lda = 0 broadcast one row.  do_ln = 0 skips
 * the normalisation (MLN with use_ln=False).  Replaces MLN.forward, ref models/utils/misc.py:182-190, at
 * models/dense_heads/farhead.py:292-303. */
int far3d_row_affine_ln(const float* x, const float* gamma, const float* beta, const float* add, float* y, int rows, int C,
                        int ldx, int ldg, int lda, int ldy, float eps, int do_ln, void* stream);

/* --- fused FarHead bookkeeping kernels (far3d_amd/csrc/glue.hip); each replaces a chain of tiny tensor ops ------------- */

/* pos2posemb3d, ref models/utils/positional_encoding.py:13-25.  pos (R,3) f32, dim_t128 (128) f32 = 1e4^(2*floor(i/2)/128),
 * out (R,384) f32 = cat(emb(y), emb(x), emb(z)). */
int far3d_posemb3d(const float* pos, const float* dim_t128, float* out, int R, void* stream);

/* Streaming-memory pre-update + temporal codes, ref models/dense_heads/farhead.py:453-477,287,297-303.
 * state: emb (L,E) ref (L,3) ts (L) f64 pose (L,4,4) velo (L,2); ego_pose_inv (4,4); timestamp (1) f64 DEVICE;
 * pseudo_ref (P,3) normalised; prev_exists 0/1; fresh != 0: the state is the all-zero first-frame memory (no ego warp).
 * out: the pre-updated memory m_*, temp_ref (L,3) normalised, nerf (L,180) f32, tpos (L,256) f32 (pos2posemb1d in f64). */
int far3d_memory_prepare(const float* emb, const float* ref, const double* ts, const float* pose, const float* velo,
                         const float* ego_pose_inv, const double* timestamp, const float* pseudo_ref, const float* dim_t256,
                         float prev_exists, int fresh, const float* pc_range, int L, int E, int P, float* m_emb, float* m_ref,
                         double* m_ts, float* m_pose, float* m_velo, float* temp_ref, float* nerf, float* tpos, void* stream);

/* Box-code finalisation of the shared reg branch + memory scores, ref models/dense_heads/farhead.py:649-664,490.
 * reg (layers*A, code) f32, ref (A,3), cls_all (layers,A,ncls) logits (may be NULL with score NULL); score (A) from the last
 * layer.  hole_count != NULL (DEVICE int32): the query rows [hole_start + *hole_count, hole_end) hold no query (fixed-capacity
 * proposal mode): their score and their logits in EVERY layer are set to -inf, so neither the memory top-k nor the decode can pick
 * them.  hole_count NULL: cls_all is only read. */
int far3d_head_finalize(const float* reg, const float* ref, float* cls_all, float* box, float* score, int layers, int A,
                        int code_size, int num_classes, const float* pc_range, const int32_t* hole_count, int hole_start, int hole_end,
                        void* stream);

/* Streaming-memory post-update, ref models/dense_heads/farhead.py:479-508: the K top-scoring queries (topk_idx, int64
 * DEVICE) are pushed in front, the queue is truncated to L and warped by ego_pose; writes the persistent state in place. */
int far3d_memory_post_update(const float* m_emb, const float* m_ref, const double* m_ts, const float* m_pose, const float* m_velo,
                             const int64_t* topk_idx, const float* dec_last, const float* box_last, const float* ego_pose,
                             const double* timestamp, int L, int E, int K, int code_size, float* emb, float* ref, double* ts,
                             float* pose, float* velo, void* stream);

/* out_sum = a + b (sum_dt), out_a = a (a_dt, optional); a, b dense (rows, C) f32, outputs with row strides ld_sum / ld_a elements
 * (multiples of 4): the decoder's [query + query_pos | query] merged-GEMM operand in one pass. */
int far3d_add_cast(const float* a, const float* b, void* out_sum, int sum_dt, void* out_a, int a_dt, int rows, int C, long ld_sum,
                   long ld_a, void* stream);

/* Query order for far3d_aggregate_forward's `perm`: queries sorted by (nearest camera, 8x8 image cell) of their reference
 * point, one single-workgroup launch (keys + LDS counting sort).  A <= 8192, N <= 16.  Scheduling only -- except that with
 * hole_count != NULL the rows [hole_start + *hole_count, hole_end) (no query there: fixed-capacity proposal mode) are entered as
 * ~a (negative): far3d_aggregate_forward writes a zero row for such an entry and does no work.
 * row_base: order the A rows [row_base, row_base + A) of `ref` (a rank's share of the queries in the query-sharded decoder); the
 * entries of perm are ABSOLUTE row indices (the hole is given in absolute rows too), so far3d_aggregate_forward is then called
 * with the full-size ref / offsets / U / out buffers, A = the share's row count and this perm.
 * tables != NULL: the same launch also computes far3d_agg_tables(Vc, tables, layers, N, J) in `layers` extra workgroups (both are
 * per-frame preparations of the aggregation; one launch instead of two). */
int far3d_agg_order(const float* ref, const float* lidar2img, int32_t* perm, int A, int N, const float* pc_range, float pad_h,
                    float pad_w, const int32_t* hole_count, int hole_start, int hole_end, int row_base,
                    const float* Vc, float* tables, int layers, int J, int split_extra, int32_t* inv, float* qbase, void* stream);
/* inv / qbase (both optional, round 6): the operands of far3d_aggregate_forward's SORTED mode.  inv (A) int32: inv[i] = the perm slot
 * (= workgroup) that handles row row_base + i, i.e. perm[inv[i]] names row row_base + i; the producers of the per-layer logits /
 * key-point offsets store their row i at row inv[i] (far3d_rowchain_attn_out's ul_rows, far3d_layernorm_rows).  qbase (A, 4) f32,
 * 16-byte aligned: qbase[slot] = (X, Y, Z, hint) -- the reference point of the query in that slot in metres (ref
 * models/utils/detr3d_transformer.py:524-525) and, as an int32 bit pattern, hint = cam0 | cam1 << 8: the two cameras the reference point
 * projects closest to.  The aggregation kernel forms the softmax weights against those two cameras ahead of its item loop (an item of
 * any other camera forms its own: the hint never changes a result).
 * split_extra > 0 (far3d_aggregate_forward variant 9): perm has A + split_extra entries; the first split_extra queries IN ROW ORDER whose
 * reference point projects into two or more cameras are marked and get a sibling entry behind the A main ones (see above). */

/* Descending top-K of n <= 40960 floats (ties -> lower index), one workgroup: idx_out (K) int64, val_out (K) f32 or NULL.
 * Replaces torch.topk in post_update_memory, ref models/dense_heads/farhead.py:488-491 (K <= 1024). */
int far3d_topk(const float* vals, int n, int K, int64_t* idx_out, float* val_out, void* stream);

/* NMS-free box decode of the last decoder layer in ONE launch.  Replaces NMSFreeCoder.decode_single
 * (ref core/bbox/coders/nms_free_coder.py:39-91), denormalize_bbox (ref core/bbox/util.py:25-52) and the z shift of
 * FarHead.get_bboxes (ref models/dense_heads/farhead.py:1236-1238).  cls_last (A,num_classes) logits, box_last (A,code_size)
 * = (cx,cy,cz,log w,log l,log h,sin,cos[,vx,vy]); post_center_range 6 floats HOST.  Outputs, sorted by descending score:
 * boxes (K,code_size-1) = (cx,cy,cz-h/2,w,l,h,atan2(sin,cos)[,vx,vy]), scores (K) = sigmoid, labels (K) int64,
 * keep (K) uint8 = centre (before the z shift) inside post_center_range (the reference drops the others).
 * K <= 1024.  A*num_classes <= 40960: one launch, workspace may be NULL.  Larger inputs (the reference's threshold proposal mode
 * on a busy frame): every 40960-logit chunk is ranked by its own workgroup and a second launch ranks the chunks' K best; that needs
 * `workspace` = FAR3D_DECODE_WS_BYTES(A*num_classes, K) bytes of 8-byte aligned DEVICE memory (contents irrelevant) and
 * ceil(A*num_classes / 40960) * K <= 40960.  Ties: the lower flat index (query-major, then class) first, in both paths. */
#define FAR3D_DECODE_WS_BYTES(n, K) ((((long)(n) + 40959) / 40960) * (long)(K) * 8)
int far3d_decode_topk(const float* cls_last, const float* box_last, int A, int num_classes, int code_size, int K,
                      const float* post_center_range, float* boxes, float* scores, int64_t* labels, unsigned char* keep,
                      void* workspace, long workspace_bytes, void* stream);
/* far3d_decode_topk + far3d_topk(mem_scores, mem_n, mem_K, mem_idx_out) in ONE launch of two workgroups (round 6): the decode and the
 * memory update's top-k (ref models/dense_heads/farhead.py:488-491) both rank outputs of the last layer and do not depend on each
 * other.  Same results as the two calls.  Shapes outside the fused launch (A*num_classes > 40960 or mem_n > 4096) run as the two calls. */
int far3d_decode_topk_mem(const float* cls_last, const float* box_last, int A, int num_classes, int code_size, int K,
                          const float* post_center_range, float* boxes, float* scores, int64_t* labels, unsigned char* keep,
                          void* workspace, long workspace_bytes, const float* mem_scores, int mem_n, int mem_K,
                          int64_t* mem_idx_out, void* stream);
/* far3d_decode_topk_mem for B >= 1 scene streams in ONE launch of 2 * B workgroups: the same kernel with the stream as a second grid
 * index (B <= 65535).  Every pointer names stream 0's operand; stream b's lies b * batch_strides[i] ELEMENTS of that operand behind it
 * (64-bit), batch_strides = 8 longs on the HOST in the order cls_last, box_last, boxes, scores, labels, keep, mem_scores, mem_idx_out.
 * For B > 1 a stride may not be below one stream's extent of its operand (A*num_classes, A*code_size, K*(code_size-1), K, K, K,
 * mem_n, mem_K): two streams never share an address.  post_center_range and all sizes are shared.  Stream b's boxes / scores /
 * labels / keep / mem_idx_out are bit for bit those of far3d_decode_topk_mem on stream b's operands and do not depend on B (same
 * instantiations, chosen by A*num_classes <= 4096 / 16384 / 40960; same tie rule).
 * Shapes outside the fused launch (A*num_classes > 40960 or mem_n > 4096): far3d_decode_topk_mem is issued per stream, stream b with
 * the workspace slice [b * workspace_bytes, (b+1) * workspace_bytes) -- `workspace` then holds B * workspace_bytes bytes of 8-byte
 * aligned DEVICE memory, workspace_bytes >= FAR3D_DECODE_WS_BYTES(A*num_classes, K) and a multiple of 8 (NULL / 0 otherwise).
 * A bad argument (a null pointer, B < 1, a stride below the extent, any size rule of the one-stream entry) returns FAR3D_ERR_ARG with
 * far3d_last_error() naming the argument, and nothing is launched for any stream. */
int far3d_decode_topk_mem_streams(const float* cls_last, const float* box_last, int B, int A, int num_classes, int code_size, int K,
                                  const float* post_center_range, float* boxes, float* scores, int64_t* labels, unsigned char* keep,
                                  void* workspace, long workspace_bytes, const float* mem_scores, int mem_n, int mem_K,
                                  int64_t* mem_idx_out, const long* batch_strides, void* stream);
/* far3d_decode_topk_mem_streams that also says which query every decoded box came from: query_out (K) int32 per stream, stream b's
 * query_stride elements behind stream 0's (>= K for B > 1) -- query_out[i] = (flat index of output i in cls_last) / num_classes, the
 * row whose logit labels[i] ranked, with the decode's tie rule (the ranking is the same).  Both decode paths write it: the fused
 * launch, and for A*num_classes > 40960 (or mem_n > 4096) per stream far3d_topk plus the one- or two-launch decode.  All other
 * arguments, rules and outputs are those of far3d_decode_topk_mem_streams, bit for bit (the same kernels, instantiated with the
 * extra store). */
int far3d_decode_topk_tracked(const float* cls_last, const float* box_last, int B, int A, int num_classes, int code_size, int K,
                              const float* post_center_range, float* boxes, float* scores, int64_t* labels, unsigned char* keep,
                              void* workspace, long workspace_bytes, const float* mem_scores, int mem_n, int mem_K,
                              int64_t* mem_idx_out, const long* batch_strides, int32_t* query_out, long query_stride, void* stream);

/* Track ids: the identity of a detection across the frames of a scene stream, carried through the streaming memory.  One launch for
 * B >= 1 streams (one workgroup each), no host read.  State per stream, updated IN PLACE: mem_track (L) int64, one id per memory slot
 * (0 = no identity; the caller zeroes it wherever it zeroes the memory), and next_id (1) int64, the next id to hand out (starts at 1;
 * never reset by a scene change, so an id is unique in its stream).  Per frame, from topk_idx (K) int64 -- the memory update's ranked
 * query rows, far3d_decode_topk_mem's mem_idx_out -- and score (A) f32, far3d_head_finalize's score plane, which holds PROBABILITIES
 * (max-class sigmoid; -inf in the rows of a hole):
 *  1. id of query row r: mem_track[r - row_start] as it stood before this call if row_start <= r < row_start + P (a propagated query:
 *     row_start = num_query + adaptive rows, the static split the engine uses in the hole modes too), else 0;
 *  2. birth, in rank order: a ranked row with id 0 whose score is finite and >= birth_thr (a probability; compared as doubles) gets
 *     next_id + (births before it in this frame); next_id advances by the number of births.  A row at -inf is never born;
 *  3. queue: mem_track = cat(ids of topk_idx[0 .. K), old mem_track)[:L] -- far3d_memory_post_update's shift.  Every old slot is read
 *     before any is written;
 *  4. detections (Kdec > 0): track_ids[i] (Kdec) int64 = the id after step 2 of query row query_idx[i] (int32, far3d_decode_topk_tracked's
 *     query_out), 0 for a row outside the top-k.  Two boxes of one query (two classes) share their id.
 * K <= 1024, K <= L <= 4096, Kdec <= 1024, P <= K (a slot carried over in the queue must not be propagated again: its id would be
 * live twice).  batch_strides: 6 longs on the HOST, elements between stream b and b + 1 of topk_idx, score, query_idx, mem_track,
 * next_id, track_ids (for B > 1 none below one stream's extent). */
int far3d_track_update(const int64_t* topk_idx, const float* score, const int32_t* query_idx, int64_t* mem_track, int64_t* next_id,
                       int64_t* track_ids, int B, int A, int K, int L, int Kdec, int row_start, int P, double birth_thr,
                       const long* batch_strides, void* stream);

/* Track records: what a tracker output needs beside the ids -- an age per id, ONE primary box per id and frame, a velocity -- from
 * state the streaming memory already carries plus one counter plane.  Launched behind far3d_track_update on the same stream, one
 * launch for B >= 1 streams (one workgroup each), no host read.  State per stream, updated IN PLACE: mem_hits (L) int32, the number
 * of frames the id in that slot of mem_track has been ranked (> 0 exactly where mem_track != 0; zeroed wherever mem_track is).
 * Inputs per stream: topk_idx (K) int64 and mem_track (L) int64 AS far3d_track_update LEFT IT (its first K entries are the ranked
 * rows' ids); query_idx (Kdec) int32, track_ids (Kdec) int64, keep (Kdec) bytes and boxes (Kdec rows of box_stride >= 3 floats, the
 * centre in metres first) of the decode; m_ref (L,3) f32 and m_ts (L) f64 of this frame's far3d_memory_prepare: a slot's previous
 * centre warped into the current lidar frame, and the seconds since it was written.  With rank t < K, row r = topk_idx[t]:
 *  1. rank t inherited its id iff row_start <= r < row_start + P and mem_hits[r - row_start] > 0 before this call;
 *  2. hits of rank t: the old mem_hits[r - row_start] + 1 if inherited, else 1 if mem_track[t] != 0 (a birth), else 0;
 *     mem_hits = cat(hits of ranks [0, K), old mem_hits)[:L], every old slot read before any is written;
 *  3. track_age[j] (Kdec) int32 = hits of the rank whose row is query_idx[j], minus 1 (0: born this frame); -1 where track_ids[j]
 *     is 0 or no rank has that row (rows outside [0, A) match none, as in far3d_track_update step 4);
 *  4. track_primary[j] (Kdec) bytes = 1 iff track_ids[j] != 0, keep[j] != 0 and no j' < j has the same id with keep set: in the
 *     decode's descending score order the best kept box of its id, so a frame never has two primaries of one id;
 *  5. track_velocity[j] (Kdec,3) f32 = (boxes[j][0:3] - m_ref[s]) / (float)m_ts[s] for a box whose rank inherited its id, with
 *     s = query_idx[j] - row_start and m_ts[s] finite and > 0: fp32, one subtraction and one division per component; metres per
 *     second in the current lidar frame, ego motion removed.  Every other box gets +0.0.
 * Sizes as far3d_track_update: K <= 1024, K <= L <= 4096, Kdec <= 1024, P <= K <= A.  batch_strides: 12 longs on the HOST,
 * elements between stream b and b + 1 of topk_idx, mem_track, query_idx, track_ids, keep, boxes, m_ref, m_ts, mem_hits, track_age,
 * track_primary, track_velocity (for B > 1 none below one stream's extent). */
int far3d_track_records(const int64_t* topk_idx, const int64_t* mem_track, const int32_t* query_idx, const int64_t* track_ids,
                        const unsigned char* keep, const float* boxes, const float* m_ref, const double* m_ts, int32_t* mem_hits,
                        int32_t* track_age, unsigned char* track_primary, float* track_velocity, int B, int A, int K, int L, int Kdec,
                        int row_start, int P, int box_stride, const long* batch_strides, void* stream);

/* Duplicate suppression of the decoded boxes by their rotated bird's-eye-view footprints (far3d_amd/csrc/dedup.hip; executable in
 * tests/dedup_refs.py).  One launch for B >= 1 streams (one workgroup each), no host read, no atomics.  Inputs per stream, in the
 * decode's order (descending score): boxes (Kdec rows of box_stride >= 7 floats: x, y, z, d3, d4, h, yaw, ...), scores (Kdec) f32,
 * labels (Kdec) int64, keep (Kdec) bytes.  None is written.
 *  - a box is a CANDIDATE iff keep != 0, its score is finite and (double)score >= score_thr;
 *  - its footprint is the rectangle centred at (x, y) that extends d3 along (cos yaw, sin yaw) and d4 along (-sin yaw, cos yaw);
 *  - a candidate with a non-finite x, y, d3, d4 or yaw, or with d3 <= 0 or d4 <= 0, is UNJUDGEABLE: it neither suppresses nor is
 *    suppressed;
 *  - a JUDGED pair is (j, i), j < i, both judgeable candidates, with equal labels if class_aware != 0.  Its overlap o: mode 0
 *    (iou_bev) the IoU of the two footprints, a hit iff o > thr; mode 1 (centre) the squared distance of the centres in m^2, a hit
 *    iff o < thr * thr;
 *  - greedy in index order: box i is suppressed iff a j < i with dup_keep[j] = 1 hits it (a suppressed box suppresses nobody).
 * Outputs: dup_keep (Kdec) bytes, 1 exactly for candidates that are not suppressed; dup_of (Kdec) int32, the smallest surviving j
 * that hit i, -1 for every box that is not suppressed.  overlap_out: NULL, or (Kdec, Kdec) f32 whose entry [i][j] is the fp32 o of
 * the judged pair (j, i) -- 0 where mode 0 rejects the pair by the distance of the centres against the sum of the circumradii --
 * and 0 everywhere else.  The arithmetic is fp32 in the suppressor's frame; the contract is the exact value on the fp32 inputs, so a
 * pair whose o lies within rounding of thr may fall on either side.  Kdec <= 1024 (0: nothing is written); thr in [0, 1) for mode 0,
 * finite and > 0 for mode 1; score_thr in [0, 1].  batch_strides: 7 longs on the HOST, elements between stream b and b + 1 of boxes,
 * scores, labels, keep, dup_keep, dup_of, overlap_out (for B > 1 none below one stream's extent; the last is not read with
 * overlap_out NULL). */
int far3d_box_dedup(const float* boxes, const float* scores, const int64_t* labels, const unsigned char* keep,
                    unsigned char* dup_keep, int32_t* dup_of, float* overlap_out, int B, int Kdec, int box_stride, int mode,
                    int class_aware, double thr, double score_thr, const long* batch_strides, void* stream);

/* Per-frame camera calibration in one launch: img2lidar (N,4,4) = inverse(lidar2img) (ref models/dense_heads/farhead.py:798;
 * Gauss-Jordan with partial pivoting in f64) and c14 (N,14) = [fx/1e3, fy/1e3, extrinsics[:3,:4]] (ref farhead.py:553-556).
 * Either output may be NULL. */
int far3d_camera_prep(const float* lidar2img, const float* intrinsics, const float* extrinsics, float* img2lidar, float* c14,
                      int N, void* stream);

/* torch.nan_to_num (nan -> 0, +-inf -> +-FLT_MAX) in place on n floats (multiple of 4), ref models/dense_heads/farhead.py:646;
 * bf16_copy (optional) receives the sanitised values as bf16. */
int far3d_nan_to_num(float* x, void* bf16_copy, long n, void* stream);

/* Camera embedding chain of ALL decoder layers in one launch (ref models/utils/detr3d_transformer.py:497-505, 531-538):
 * out[l][n][:] = W3[l] LN(ReLU(W2[l] ReLU(W0[l] l2i[n] + b0[l]) + b2[l])) + b3[l]   (cam_embed -> camera term of weights_fc).
 * l2i: row n holds lidar2img[n][:3,:] flattened in its first 12 floats, row stride ld_l2i (16 = the (N,4,4) tensor in place); weights fp32, TRANSPOSED to [in][out]: w0t [L][12][Hd], w2t [L][Hd][256],
 * w3t [L][256][J]; b0 [L][Hd], b2/ln_g/ln_b [L][256], b3 [L][J]; out [L][N][J].  Embedding width 256, hidden Hd <= 256. */
int far3d_cam_embed_chain(const float* l2i, const float* w0t, const float* b0, const float* w2t, const float* b2,
                          const float* ln_g, const float* ln_b, const float* w3t, const float* b3, float* out, int N, int L,
                          int J, int Hd, float eps, int ld_l2i, void* stream);

/* --- device image pre-processing (far3d_amd/csrc/preproc.hip) ------------------------------------
 * Pillow-exact 8-bit separable resampling (Image.resize as used by AV2ResizeCropFlipRotImageV2._img_transform,
 * ref datasets/pipelines/custom_pipeline.py:277-311) restricted to the crop window, then crop / flip / normalise / pad / HWC->CHW
 * (ref datasets/pipelines/transform_3d.py:89-101, custom_pipeline.py:358-378).  bounds (out_size,2) and coeffs (out_size,ksize)
 * int32 DEVICE: per output position the first input sample, the sample count and the 22-bit fixed-point filter weights, built on
 * the host exactly like Pillow's precompute_coeffs + normalize_coeffs_8bpc (far3d_amd/data_pipeline/resample.py).
 *
 * far3d_image_resample_h: horizontal pass.  src u8 HWC (in_h,in_w,3), row pitch src_pitch bytes; dst u8 (rows,outw,3) = output
 *   columns [x0, x0+outw) of input rows [row0, row0+rows).
 * far3d_image_resample_v: vertical pass over that intermediate for output rows [y0, y0+outh), optional horizontal flip, then
 *   mode 0: u8 HWC (outh,outw,3) (an intermediate image: the portrait camera is resized twice, custom_pipeline.py:71-92), or
 *   mode 1: out (3,pad_h,pad_w) f32|bf16 = (pixel - mean[c]) * stdinv[c] inside the crop, 0 in the padding; mean / stdinv 3 floats
 *   HOST; to_rgb swaps channels 0 and 2 first. */
int far3d_image_resample_h(const unsigned char* src, long src_pitch, int in_h, int in_w, unsigned char* dst, const int32_t* bounds,
                           const int32_t* coeffs, int ksize, int row0, int rows, int x0, int outw, void* stream);
int far3d_image_resample_v(const unsigned char* tmp, int row0, int rows, int outw, const int32_t* bounds, const int32_t* coeffs,
                           int ksize, int y0, int outh, int flip, int mode, void* out, int out_dt, int pad_h, int pad_w,
                           const float* mean, const float* stdinv, int to_rgb, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FAR3D_HIP_H */
