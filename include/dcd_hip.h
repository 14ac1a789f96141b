/*
 * include/dcd_hip.h -- C ABI of libdcd_hip.so, the MI355X (gfx950) implementation of the DGDE hot path.
 *
 * Every entry point is `extern "C"`, takes plain device pointers, sizes and a HIP stream
 * (passed as void* so the header needs no HIP include), enqueues work on that stream without
 * any host synchronisation, and returns an int status:
 *     0 = DCD_OK, 1 = DCD_ERR_BAD_ARG (shape / null pointer / unsupported value),
 *     2 = DCD_ERR_WORKSPACE (workspace too small), 3 = DCD_ERR_LAUNCH (hipGetLastError != success).
 * Nothing is printed; the caller raises.  All tensors are contiguous fp32 NCHW unless stated.
 *
 * Each function cites the reference interface it replaces (paths relative to /root/reference).
 */
#ifndef DCD_HIP_H
#define DCD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCD_OK 0
#define DCD_ERR_BAD_ARG 1
#define DCD_ERR_WORKSPACE 2
#define DCD_ERR_LAUNCH 3

/* Library / build identification: returns e.g. "dcd_hip 0.1 gfx950". */
const char *dcd_version(void);

/* ------------------------------------------------------------------------------------------------
 * Environment.  The library's RESULTS never depend on the process environment (beyond summation order); which of two equivalent
 * launch sequences a call takes can: the variables below are A/B-timing and test switches read through dcd_env()
 * (csrc/tuning_env.h) -- some once per process (static), some per call (marked *).  Building with -DDCD_NO_TUNING_ENV compiles
 * every read out (each switch then keeps the default given here).  tests/test_abi.py checks this list against the sources.
 *   DCD_DCN_HANDOVER     auto (default) | always | never: who takes the far samples of a one-pass DCN backward -- per layer from
 *                        its previous call's far count (auto), the device-side hand-over to the generic kernels armed on every
 *                        call (always), or never armed.  See dcd_dcn_v2_forget below.
 *   DCD_FAR_DIV, DCD_FAR_DIV_WIDE   integer d > 0: hand a one-pass backward call to the generic kernels above 1 far coordinate in
 *                        d (Cout <= 64 / wider).  Default 24 / 16 at >= 4 images, 12 / 8 below.
 *   DCD_BWD_SWEEP *      0: three-pass DCN backward everywhere; 2: layers the dense path takes stay on it; default 1: one-pass
 *                        backward wherever it applies.
 *   DCD_SWEEP_WIDE *     0: one-pass backward for Cout <= 64 only (round 3's limit).  Default: Cout <= 128, and 256 where the
 *                        dense path does not apply.
 *   DCD_SWEEP_SLOTS *    waves of a one-pass backward launch (0: one work unit per wave).  Default: one round of resident waves.
 *   DCD_SWEEP_MIN_ROWS   fewest rows of a one-pass backward work unit (a unit pays ~5 rows of ring warm-up).  Default 3
 *                        (8: the segment choice of rounds 3-4 on under-filled launches).
 *   DCD_DCN_DENSE *      0: never the column-buffer path; 1: every geometry it can take; default: Cin >= 256 only.
 *   DCD_NO_TILE *        set: the workgroup-tiled LDS kernels (forward, generic backward) stand down for the register-gather ones.
 *   DCD_TILE_ROWS        4: forward regions of 4 rows always.  Default 8 rows when that fills the chip.
 *   DCD_FWD_RESCUE_TAPS  1..10: far taps in a region's worst wave that hand the region to the rescue kernel.  Default 5.
 *   DCD_BD_TILE128       1: the tiled generic data-gradient kernel also for Cout 128.  Default off.
 *   DCD_BI_TILE_NBLK     input-channel blocks (of 32) up to which the tiled generic grad_input kernel is used.  Default 2.
 *   DCD_NO_BI_TILE *     set: never the tiled generic grad_input kernel.
 *   DCD_BI_HYBRID        0: one generic grad_input kernel per call, chosen by the call-wide offset radius.  Default: per tile.
 *   DCD_BI_MB *          1 | 2 | 4 | 8: channel blocks per workgroup of the register-gather grad_input kernel.  Default: by size.
 *   DCD_DW_GEN           1: first-generation generic grad_weight kernel.  Default 2.
 *   DCD_DW_ORDER         0: the generic grad_weight kernel walks its tiles row by row.  Default: down column strips.
 *   DCD_CONV_GEOM *      0 | 1: pin the Winograd region shape (8 x 32 / 12 x 20 px), no split contraction.  Default: by cost model.
 *   DCD_CONV_MINCHUNK    smallest number of 8-channel chunks a split of the Winograd contraction keeps.  Default 4.
 *   DCD_CONV_DIRECT_MINCHUNK  the same for the direct bf16 form's 16-channel chunks.  Default 16.
 *   DCD_CONV_DIRECT_P *  4: 16 x 32 px regions (one workgroup per CU) instead of 8 x 32 in the direct bf16 form.  Default 2.
 *   DCD_CONV_WRW_DIRECT * 0: the one-product weight gradient stays on the Winograd-domain kernel.  Default 1 (direct, Cout > 32).
 *   DCD_CONV_DIRECT_MODE * operand residency of the direct bf16 form: 0 weights in registers, 1 window operands in registers, 2 both
 *                        streamed from LDS (four waves per SIMD).  Default 1.
 *   DCD_CONV_DIRECT_WX * 2: 8 x 64 px regions (eight waves) in the direct bf16 form.  Default 1 (8 x 32).
 *   DCD_BN_SMALL         0: no single-workgroup-per-channel BatchNorm kernels for small maps.  Default on.
 *   DCD_CHANNEL_SUM_ONE_LAUNCH   1 | 0: pin the per-channel sums to the one-launch / two-launch form.  Default: by grid size.
 *   DCD_UP_FWD_OLD, DCD_UP_BWD_OLD   set: the round-1 depthwise up-sampling kernels.
 * ---------------------------------------------------------------------------------------------- */

/* ------------------------------------------------------------------------------------------------
 * DCNv2 (modulated deformable convolution).
 * Replaces `_ext.dcn_v2_forward` / `_ext.dcn_v2_backward`
 *   DGDE/model/backbone/DCNv2/DCN/src/dcn_v2.h:9-46, :48-92            (dispatch)
 *   DGDE/model/backbone/DCNv2/DCN/src/cuda/dcn_v2_cuda.cu:42-172, :206-341 (host)
 *   DGDE/model/backbone/DCNv2/DCN/src/cuda/dcn_v2_im2col_cuda.cu:125-327   (kernels)
 * and the three extern "C" launchers in cuda/dcn_v2_im2col_cuda.h:68-99 (fused away: no column buffer).
 *
 * input  (B,Cin,H,W)            weight (Cout,Cin,kh,kw)       bias (Cout)
 * offset (B,dg*2*kh*kw,Ho,Wo)   interleaved (dh,dw) per tap   mask (B,dg*kh*kw,Ho,Wo)
 * output / grad_output (B,Cout,Ho,Wo), Ho = (H+2ph-(dh*(kh-1)+1))/sh+1, likewise Wo.
 *
 * precision: 0 = DCD_PREC_F32    exact fp32 MFMA (v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32)
 *            1 = DCD_PREC_BF16X3 split-bf16 (hi*hi + hi*lo + lo*hi on the bf16 MFMAs, fp32 accumulate;
 *                                ~2^-16 relative per product).  Permits, does not oblige: geometries
 *                                without a split kernel run the exact fp32 kernels.
 *            2 = DCD_PREC_BF16   mixed precision (MODEL.FP16, DGDE/model/detector.py:34-36): both operands of the weight
 *                                contraction rounded to bf16 (nearest even), ONE product on the bf16 MFMAs, fp32
 *                                accumulate; sampling / coordinate arithmetic, storage and every sum stay fp32.
 *                                ~2^-9 relative per operand.  Permits, does not oblige (kernels without the one-product
 *                                form run the split-bf16 or the exact fp32 one).
 * workspace: device scratch of at least dcd_dcn_v2_workspace_bytes(...) bytes, 256-byte aligned,
 *            owned by the caller; contents are dead after the call's kernels complete.  Its layout -- byte offset and length of
 *            every region, for both passes -- is csrc/dcn_workspace.h (DcnWorkspace); the size depends on the per-call
 *            switches DCD_DCN_DENSE and DCD_BWD_SWEEP, so query it under the environment of the call.
 * ---------------------------------------------------------------------------------------------- */
#define DCD_PREC_F32 0
#define DCD_PREC_BF16X3 1
#define DCD_PREC_BF16 2

size_t dcd_dcn_v2_workspace_bytes(int B, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw,
                                  int ph, int pw, int dh, int dw, int dg);

int dcd_dcn_v2_forward(void *stream, const float *input, const float *weight, const float *bias,
                       const float *offset, const float *mask, float *output, int B, int Cin, int H, int W,
                       int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int dg,
                       int precision, void *workspace, size_t workspace_bytes);

/* All five gradients are fully overwritten (the callee zero-fills what it accumulates into).
 * grad_input and grad_weight are summed with fp32 atomics where work units overlap, like the reference's col2im
 * (cuda/dcn_v2_im2col_cuda.cu:249: order-nondeterministic sums); grad_offset / grad_mask are bit-reproducible on the
 * one-pass path (3x3, stride 1, pad 1, one group, Cout <= 64: csrc/dcn_bwd_sweep.inc) when no sample is displaced by
 * 3 px or more. */
int dcd_dcn_v2_backward(void *stream, const float *input, const float *weight, const float *bias,
                        const float *offset, const float *mask, const float *grad_output, float *grad_input,
                        float *grad_offset, float *grad_mask, float *grad_weight, float *grad_bias, int B,
                        int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                        int dw, int dg, int precision, void *workspace, size_t workspace_bytes);

/* Per-layer launch policy of the DCNv2 op (csrc/dcn_v2.hip, "Who takes the far samples").  The library remembers, per
 * (device, weight pointer), the far-sample count of the layer's last backward call (a word of mapped pinned host memory the
 * call's last kernel stores to) and chooses the next call's launch sequence from it -- never its result.
 *   dcd_dcn_v2_forget(weight)   the owner of `weight` (current device) tells the library that this address no longer names that
 *                               layer (tensor freed, moved, re-used): the entry is dropped, the next call on that address starts as
 *                               "unknown" (hand-over armed).  weight = NULL: every entry of the current device.  The dropped
 *                               entry's report word is reset and recycled, not unmapped (a HIP graph captured earlier may still
 *                               store to it).
 *   dcd_dcn_v2_policy_state(weight, &far)   0: no entry; 1: entry, no report yet; 2: *far = the last reported far count; -1: error.
 *   dcd_dcn_v2_policy_free()    frees all policy state of the process (all devices).  Only when no captured graph containing
 *                               DCN backward calls will be replayed again.
 *   dcd_dcn_v2_set_handover(mode)   pins the policy for the process: 0 never hand over, 1 always armed, 2 auto (the default), -1 back
 *                               to the DCD_DCN_HANDOVER environment default.  For callers that need two runs of one step to take the
 *                               same launch sequence (a captured graph and its eager twin).
 * A CAPTURED call freezes its decision: a graph captured while a layer's offsets were small replays the "never hand over" sequence
 * (correct for any offsets, slower beyond the far-count limit) until it is captured again. */
int dcd_dcn_v2_forget(const float *weight);
int dcd_dcn_v2_policy_state(const float *weight, unsigned *far_count);
int dcd_dcn_v2_policy_free(void);
int dcd_dcn_v2_set_handover(int mode);

/* ------------------------------------------------------------------------------------------------
 * Edge-constraint depth solver.
 * Replaces Anno_Encoder.decode_pairs_kpts_depth + get_up  (DGDE/model/anno_encoder.py:313-390),
 * PostProcessor.compute_pairs_kpts_depth                  (DGDE/model/head/detector_infer.py:215-225)
 * and GMW compute_z                                        (GMW/main.py:373-416).
 *
 * kps (N,K,2) image pixels; kps3d (N,K,3) object frame; rot_y (N); P (N,3,4) projection matrices;
 * kmask (N,K) uint8 or NULL.  npairs = K*(K-1)/2 pairs enumerated row-major over the upper triangle.
 *   z_ij = |(Y_i-Y_j) + (v'_i C_i - v'_j C_j)| / max(|v'_i - v'_j|, 1e-10), clamped to [zmin,zmax],
 *   v' = (v - P[1][2]) / P[1][1] (or v itself if normalized != 0), C = X sin(rot) - Z cos(rot).
 * topk == 0 : depth (N,npairs) in pair order                (eval; anno_encoder.py:383-384)
 * topk  > 0 : the topk pairs with the largest |v'_i-v'_j|, ordered like torch.topk (descending value,
 *             ties by lower pair index first); depth (N,topk), pair_idx (N,topk) int32,
 *             pair_mask (N,topk) float = kmask_i*kmask_j (only if kmask)      (anno_encoder.py:377-382)
 * Finally subtracts P[2][3] when sub_b3 != 0 (anno_encoder.py:385; not in GMW).
 * K <= 128.
 * ---------------------------------------------------------------------------------------------- */
int dcd_edge_depth_forward(void *stream, const float *kps, const float *kps3d, const float *rot_y,
                           const float *P, const uint8_t *kmask, int N, int K, int topk, float zmin,
                           float zmax, int normalized, int sub_b3, float *depth, int32_t *pair_idx,
                           float *pair_mask);

/* Backward of the above w.r.t. kps (v coordinate only; u does not enter) and kps3d.
 * grad_depth (N,M) with M = topk ? topk : npairs; pair_idx as produced by the forward (NULL if topk==0).
 * grad_kps (N,K,2) and grad_kps3d (N,K,3) are overwritten.  No gradient flows through the clamp's
 * saturated branch, the top-k selection, or max(.,1e-10) when saturated (autograd semantics). */
int dcd_edge_depth_backward(void *stream, const float *kps, const float *kps3d, const float *rot_y,
                            const float *P, const float *grad_depth, const int32_t *pair_idx, int N, int K,
                            int topk, float zmin, float zmax, int normalized, float *grad_kps,
                            float *grad_kps3d);

/* ------------------------------------------------------------------------------------------------
 * Penalty-reduced focal loss.  Replaces FocalLoss.forward (DGDE/model/layers/focal_loss.py:57-86).
 * pred, target: n elements.  out[0] = loss sum, out[1] = number of positives (target == 1).
 * grad_pred (n) may be NULL; if given it receives d(loss_sum)/d(pred) (to be scaled by the caller).
 * `out` must be zero-filled by the callee (it is) -- two floats.  n = 0 gives (0, 0); pred and target may then be NULL.
 * A target outside [0, 1] contributes no loss, no gradient and no positive; alpha and beta may be any positive numbers.
 * ---------------------------------------------------------------------------------------------- */
int dcd_focal_loss(void *stream, const float *pred, const float *target, int64_t n, float alpha, float beta,
                   float *out, float *grad_pred);

/* ------------------------------------------------------------------------------------------------
 * GIoU loss on (l,t,r,b) distances.  Replaces IOULoss.forward (DGDE/model/layers/iou_loss.py:12-49).
 * pred, target (N,4) -> losses (N) = 1 - giou, ious (N); grad_pred (N,4) optional = d losses_i / d pred_i.
 * ---------------------------------------------------------------------------------------------- */
int dcd_giou_loss(void *stream, const float *pred, const float *target, int N, float *losses, float *ious,
                  float *grad_pred);

/* ------------------------------------------------------------------------------------------------
 * Heat-map decode: 3x3 max-pool NMS and per-image top-K.
 * Replaces nms_hm (DGDE/model/layers/utils.py:45-58) and select_topk (:61-100).
 *
 * dcd_nms_hm: out = heat * (maxpool3x3(heat) == heat), same shape (B,C,H,W).
 *
 * dcd_heatmap_topk: heat (B,C,H,W) -> scores (B,K) descending, inds (B,K) int64 = y*W+x of the winner,
 * clses (B,K) float = (c*K + rank_in_class)/K as the reference's true division yields (utils.py:91),
 * ys = floor(ind / W), xs = ind % W as float (utils.py:80-81).  fuse_nms != 0 applies the 3x3 NMS on
 * the fly (one launch for PostProcessor's nms_hm -> select_topk, detector_infer.py:102-106);
 * fuse_nms == 0 ranks `heat` as given (select_topk semantics).
 * Ties: lower linear index first (torch.topk leaves tie order unspecified; pinned by tests).
 * Requires K <= 128, K <= H*W, C*K <= 4096 and H*W <= 2^24.
 * ---------------------------------------------------------------------------------------------- */
int dcd_nms_hm(void *stream, const float *heat, int B, int C, int H, int W, float *out);
int dcd_heatmap_topk(void *stream, const float *heat, int B, int C, int H, int W, int K, int fuse_nms,
                     float *scores, int64_t *inds, float *clses, float *ys, float *xs, void *workspace,
                     size_t workspace_bytes);
size_t dcd_heatmap_topk_workspace_bytes(int B, int C, int H, int W, int K);

/* ------------------------------------------------------------------------------------------------
 * Point-of-interest gather.  Replaces select_point_of_interest (DGDE/model/layers/utils.py:120-145)
 * without the NCHW->NHWC copy.  feat (B,C,H,W), index (B,M) int64 linear y*W+x -> out (B,M,C).
 * Backward scatters grad_out (B,M,C) into grad_feat (B,C,H,W) with atomics (duplicate indices add);
 * the call ADDS to grad_feat: zero-fill it for a plain gradient, or pass a map to accumulate into.
 * An index outside [0, H*W) is not an error: the gather returns exactly 0.0 for that row, the scatter writes
 * nothing for it, whatever M is (both scatter routes, below and from 64 positions per image on).
 * dcd_patch_scatter_add: a tap whose element index base + (t / 3) * pitch + t % 3 falls outside [0, plane)
 * is dropped in the same way, tap by tap (the other taps of that window are still added).
 * ---------------------------------------------------------------------------------------------- */
int dcd_poi_gather(void *stream, const float *feat, const int64_t *index, int B, int C, int H, int W, int M,
                   float *out);
int dcd_poi_scatter_add(void *stream, const float *grad_out, const int64_t *index, int B, int C, int H, int W,
                        int M, float *grad_feat);
/* out (B, C, plane) += the gradient of 3x3 patches gathered at listed cells: grad_patches (B, C*9, M) [row c*9 + tap], base (B, M)
 * = index of the window's top-left element inside the plane, whose rows are `pitch` apart (head trunks evaluated at the object
 * centres only, dcd_amd/model/head/trunk_moments.py; no reference counterpart: the reference evaluates the trunks densely). */
int dcd_patch_scatter_add(void *stream, const float *grad_patches, const int64_t *base, int B, int C, int64_t plane, int pitch, int M,
                          float *out);

/* ------------------------------------------------------------------------------------------------
 * 3-D IoU of N box pairs (a logging metric of the train step).  Replaces get_iou_3d
 * (DGDE/model/layers/iou_loss.py:99-136, a per-object shapely loop on the host).
 * corners (N,8,3): 0..3 bottom face, 4..7 top face, camera frame (y down).  iou (N).
 * ---------------------------------------------------------------------------------------------- */
int dcd_iou3d(void *stream, const float *pred_corners, const float *target_corners, int N, float *iou);

/* ------------------------------------------------------------------------------------------------
 * The 1x1 output layers of the regression heads evaluated at listed rows: the reference applies one nn.Conv2d(256, out_j, 1)
 * per head to its trunk's dense output and concatenates the maps (DGDE/model/head/detector_predictor.py:84-101, :160-170,
 * :198-203); training reads them at the object centres only (detector_loss.py:231-233), so here
 *     y[r][ch0_j + o] = bias_j[o] + sum_k feat[trunk_j][r][k] * weight_j[o][k]        r = 0 .. R-1 (R = B * MAX_OBJECTS)
 * for all heads in ONE launch, and the backward in two (feature gradient per trunk; weight and bias gradients).
 * feat (T, R, K) trunk outputs at the rows, heads ordered by trunk, ch0_j = running sum of out_j, C = their total.
 * ---------------------------------------------------------------------------------------------- */
#define DCD_HEADS_MAX 16
typedef struct dcd_head_rows_args {
    int n_heads, T, R, K, C;
    int trunk[DCD_HEADS_MAX], ch0[DCD_HEADS_MAX], out[DCD_HEADS_MAX];
    const float *weight[DCD_HEADS_MAX];      /* (out_j, K) */
    const float *bias[DCD_HEADS_MAX];        /* (out_j) or NULL */
    const float *feat;                       /* (T, R, K) */
    float *y;                                /* (R, C): forward output */
    const float *grad_y;                     /* (R, C) */
    float *grad_feat;                        /* (T, R, K): every element written */
    float *grad_weight[DCD_HEADS_MAX];       /* (out_j, K) */
    float *grad_bias[DCD_HEADS_MAX];         /* (out_j) or NULL */
} dcd_head_rows_args;

int dcd_head_rows_forward(void *stream, const dcd_head_rows_args *args);
int dcd_head_rows_backward(void *stream, const dcd_head_rows_args *args);

/* ------------------------------------------------------------------------------------------------
 * Per-object rows of the training loss: every term of Loss_Computation.forward that is a sum over the
 * annotated objects (DGDE/model/head/detector_loss.py:405-583) and the decodes of
 * prepare_predictions that feed them (:217-403; DGDE/model/anno_encoder.py:93-128 encode_box3d, :130-145
 * decode_depth, :147-161 decode_location_flatten, :193-224 decode_depth_from_keypoints_batch, :226-252
 * decode_dimension, :254-304 decode_axes_orientation, :392-393 decode_kpts_2d_img), evaluated for all B*M object
 * slots at once: one wave per slot, empty slots masked out of every sum (they read the first annotated object so
 * that all arithmetic stays finite).  Supported configuration = the DGDE run: multi-bin orientation with 4 bins,
 * 10 box keypoints, 'inv_sigmoid' depth, 'exp' dimensions scaled by the class mean, L1 regression losses, corner
 * depth from the edge solver, depth and keypoint-depth uncertainties.
 *
 * Columns (sums over the slots in `sums`, per slot in `cols` (DCD_LOSS_ROWS_NCOL, B*M)), masks already applied:
 *   0 annotated, 1 GIoU loss, 2 IoU, 3 box valid, 4 depth L1 (log), 5 depth L1 with uncertainty, 6 truncated offset,
 *   7 offset, 8 multi-bin, 9 dimensions, 10 3-D IoU, 11 corners L1, 12 keypoints L1, 13 dense 2-D keypoints,
 *   14 their mask count, 15 dense 3-D keypoints, 16 their mask count, 17 pair depth L1 on valid pairs, 18 on invalid
 *   pairs (no gradient), 19 / 20 the pair counts, 21 pair relative error (log), 22 keypoint depth L1 (log),
 *   23 with uncertainty on visible groups, 24 uncertainty-scaled L1 on invisible groups (gradient to the uncertainty).
 *
 * Call order, all on one stream:
 *   dcd_loss_rows_prepare   fills kps_pred/kps_tgt (B*M,K,2 image pixels), kps3d_pred/kps3d_tgt (B*M,K,3), and, each
 *                           stored twice, rot (2,B*M), P_rows (2,B*M,3,4), kmask (2,B*M,K) -- the inputs of
 *                           dcd_edge_depth_forward; with kps_pred|kps_tgt and kps3d_pred|kps3d_tgt adjacent in memory
 *                           one solver call over 2*B*M rows serves both
 *   dcd_edge_depth_forward  (caller): predictions -> pair_depth (+ pair_idx); targets -> pair_mask
 *   dcd_loss_rows_forward   cols, corners_pred / corners_tgt (B*M,8,3), iou3d (B*M), sums (NCOL)
 *   dcd_loss_rows_backward  grad_sums (NCOL) -> grad_pois (B*M,C; every element written), grad_pair (B*M,NP)
 *   dcd_edge_depth_backward (caller): grad_pair -> grad_kps, grad_kps3d
 *   dcd_loss_rows_finish    grad_pois += the solver's gradients (4 * grad_kps on the 2-D keypoint channels)
 * Every output of every call is written for EVERY slot, empty ones included: kps_*, kps3d_*, both copies of rot and P_rows, and
 * corners_pred / corners_tgt hold for an empty slot what the first annotated object gives (slot 0 of the batch if there is none),
 * both copies of kmask are 0 there, cols is 0 there in every column, iou3d whatever dcd_iou3d makes of those corners (possibly not
 * finite; its column and its sum take 0 instead), grad_pois and grad_pair exactly 0; dcd_loss_rows_finish leaves the rows of empty
 * slots as they are.
 * ---------------------------------------------------------------------------------------------- */
#define DCD_LOSS_ROWS_NCOL 25
typedef struct dcd_loss_rows_args {
    int B, M, C, K, NP, num_classes;          /* images, slots per image, head channels, dense keypoints, pairs, classes */
    /* first channel of each regression head inside the C channels (Converter_key2channel, layers/utils.py:22-37) */
    int ch_box2d, ch_offset, ch_corner, ch_corner_unc, ch_dims, ch_ori_cls, ch_ori_off, ch_depth, ch_depth_unc,
        ch_kpts2d, ch_kpts3d;
    int trunc_log;                            /* TRUNCATION_OFFSET_LOSS: 1 = log(1 + l1), 0 = l1 */
    float depth_lo, depth_hi, unc_lo, unc_hi; /* DEPTH_RANGE, UNCERTAINTY_RANGE */
    float depth_weight;                       /* loss weight of depth_loss (inside the uncertainty form, :438-441) */
    float dim_weight[3];                      /* DIMENSION_WEIGHT */
    float down_ratio, kd_eps;                 /* BACKBONE.DOWN_RATIO; Anno_Encoder.EPS */
    const float *pois;                        /* (B*M, C) head outputs at the object centres */
    /* targets, (B, M, ...) as ParamsList stacks them */
    const uint8_t *reg_mask, *trunc_mask, *find_pcl, *ori_mask;
    const int32_t *cls_ids, *centers;         /* (B,M), (B,M,2) */
    const int64_t *pad_size;                  /* (B,2) */
    const float *bboxes, *locations, *rotys, *offset_3D, *dimensions, *orientations;   /* (..,4) (..,3) (..) (..,2) (..,3) (..,8) */
    const float *keypoints, *kp_depth_mask;   /* (B,M,10,3), (B,M,3) */
    const float *kpts2d, *kpts3d;             /* (B,M,K,3) each */
    const float *calib_P;                     /* (B,M,3,4) */
    const float *calib;                       /* (B,6): c_u, c_v, f_u, f_v, b_x, b_y */
    const float *dim_mean;                    /* (num_classes,3) */
    /* solver side */
    float *kps_pred, *kps_tgt, *kps3d_pred, *kps3d_tgt, *rot, *P_rows;
    uint8_t *kmask;
    const float *pair_depth, *pair_mask;      /* (B*M, NP) */
    /* forward outputs */
    float *cols, *corners_pred, *corners_tgt, *iou3d, *sums;
    /* backward */
    const float *grad_sums;
    float *grad_pois, *grad_pair;
    const float *grad_kps, *grad_kps3d;
} dcd_loss_rows_args;

int dcd_loss_rows_prepare(void *stream, const dcd_loss_rows_args *args);
int dcd_loss_rows_forward(void *stream, const dcd_loss_rows_args *args);
int dcd_loss_rows_backward(void *stream, const dcd_loss_rows_args *args);
int dcd_loss_rows_finish(void *stream, const dcd_loss_rows_args *args);

/* out = srcs[0] + ... + srcs[n-1] (n <= 16 device tensors of `numel` floats; `srcs` is a HOST array of
 * device pointers).  Replaces autograd's chain of n-1 pairwise gradient additions where one feature map feeds the twelve
 * head trunks (DGDE/model/head/detector_predictor.py:149-160 call every trunk on the same `features`). */
int dcd_sum_tensors(void *stream, const float *const *srcs, int n, float *out, int64_t numel);

/* The glue between `conv_offset_mask` and the deformable convolution in `DCN.forward` (DGDE/model/backbone/DCNv2/dcn_v2.py:118-123:
 * chunk into o1, o2, mask; offset = cat(o1, o2); mask = sigmoid(mask)) and its adjoint, one launch each.
 *   split: out (B, 3*taps, HW) -> offset (B, 2*taps, HW) = the first 2*taps channels, mask (B, taps, HW) = sigmoid of the rest
 *   merge: grad_out (B, 3*taps, HW) = [grad_offset | grad_mask * mask * (1 - mask)]                       (taps = dg * kh * kw) */
int dcd_dcn_offset_mask_split(void *stream, const float *out, float *offset, float *mask, int B, int taps, int64_t HW);
int dcd_dcn_offset_mask_merge(void *stream, const float *grad_offset, const float *grad_mask, const float *mask, float *grad_out, int B,
                              int taps, int64_t HW);

/* Batched fp32 product on the matrix pipe whose second operand is a set of SHIFTED VIEWS of one buffer:
 *     C[z][s] (M x N, row-major, ldc) = A[z] (M x K, row-major, lda) * B[z] (K x N)   over k in split s,   (+ bias[m] when nsplit == 1)
 *     B[z](k, n) = b_kcontig ? Bbase[z*strideB + b_off[n] + k] : Bbase[z*strideB + b_off[k] + n]
 * b_off: device array (N resp. K entries) of element offsets, any 4-byte aligned position -- e.g. row c of a zero-padded image
 * plane shifted by (dy, dx).  64-row tiles (M is the 64 channels of the head feature map).  It evaluates the 3x3-patch Gram
 * matrix of the regression-head input through its 25 autocorrelation matrices R_d[c,c'] = sum_p x[c,p] x[c',p+d] and the
 * gradient dX = sum_d K_d Xshift_d (dcd_amd/model/head/trunk_moments.py): what the reference spends on eleven dense
 * 3x3 convolutions + BatchNorm statistics of one shared input (DGDE/model/head/detector_predictor.py:104-120, 149-160).
 * Partials of split s go to C + z*strideC + s*strideCs; the caller sums them (in fp64). */
int dcd_sgemm_shifted(void *stream, const float *A, int lda, long long strideA, const float *Bbase, const long long *b_off,
                      long long strideB, int b_kcontig, const float *bias, float *C, int ldc, long long strideC,
                      long long strideCs, int M, int N, int K, int Z, int nsplit);

/* Batched fp32 GEMM on the matrix pipe (csrc/sgemm_f32.inc, 128 x 128 tiles):
 *     C[z] (M x N, row-major, ldc) = alpha * A[z] B[z]  (+ C[z] when accumulate)
 *     A(m,k) = a_kcontig ? A[m*lda + k] : A[k*lda + m]        B(k,n) = b_kcontig ? B[n*ldb + k] : B[k*ldb + n]
 * lower_only: tiles entirely above the diagonal are skipped (symmetric results; entries above the diagonal of the remaining
 * tiles are still written).  A and B 16-byte aligned, lda / ldb / strideA / strideB multiples of 4; C, ldc and strideC need only
 * the alignment of a float.  Elements of C outside the M x N region and in skipped tiles are not touched.  Used for the Schur
 * complement S = diag(c) - G^T diag(1/r) G of the transport layer's backward (GMW/lib/optimal_transport.py:93-100), written
 * straight into the buffer dcd_spd_solve factorises. */
int dcd_sgemm(void *stream, const float *A, int lda, long long strideA, int a_kcontig, const float *B, int ldb, long long strideB,
              int b_kcontig, float *C, int ldc, long long strideC, int M, int N, int K, int Z, float alpha, int accumulate,
              int lower_only);

/* Batched SPD solve  y[b] = S[b]^-1 r[b]  (one right-hand side per matrix) on the fp32 matrix pipe: blocked Cholesky whose panel
 * and trailing updates are MFMA GEMMs, forward substitution carried along with the factorisation, blocked backward substitution
 * (csrc/spd.hip).  Replaces `torch.cholesky` + `torch.cholesky_inverse` of the Schur complement in the backward of the
 * optimal-transport layer (GMW/lib/optimal_transport.py:102-128; n = 2628 edges).
 *   S: batch x rows x n fp32 (row stride n, rows >= n + 1, 16-byte aligned, n % 4 == 0): rows 0..n-1 = the symmetric positive
 *   definite matrix (lower triangle read, overwritten by the factor), row n = the right-hand side (overwritten).  y: batch x n.
 *   info (batch ints, zeroed by the caller, may be NULL): 0, or 1 + the first row of the 128-block in which a pivot was not
 *   positive (the reference raises there; here y is meaningless for that matrix). */
size_t dcd_spd_solve_workspace_bytes(int batch, int n);
int dcd_spd_solve(void *stream, float *S, float *y, int batch, int n, int rows, int *info, void *workspace, size_t workspace_bytes);

/* Context normalisation of GMW's feature extractor (`gcn`, GMW/model/yi2018cvpr/ops.py:5-17): x (rows, K) -> y = (x - mean) /
 * sqrt(var_unbiased + eps) per row, inv (rows) = the scale; backward from (grad_y, y, inv).  rows = batch * channels. */
int dcd_context_norm_forward(void *stream, const float *x, float *y, float *inv, int rows, int K, float eps);
int dcd_context_norm_backward(void *stream, const float *grad_y, const float *y, const float *inv, float *grad_x, int rows, int K);

/* The tail of a residual block of that extractor at inference (conv1d_resnet_block, yi2018cvpr/ops.py:67-131: gcn -> ReLU -> + input)
 * in one pass: y = relu(context_norm(x)) + residual, x / residual / y (rows, K).  No `inv`, no backward: for torch.no_grad() only. */
int dcd_context_norm_relu_add_forward(void *stream, const float *x, const float *residual, float *y, int rows, int K, float eps);

/* GMW inference (GMW/main.py:524-548 `validate` after the extractors; GMW/model/model.py:154-199): edge weights, weighted depth and
 * the refined location of B objects without the K x K distance matrix (csrc/gmw.hip).
 *   f4, f6: (B, C, K) the two extractors' outputs as they lie (points contiguous).  depths: (B, K) edge depths of `compute_z`.
 *   good_idx: (B, num_k) int64 indices into K, as `compute_z` returns them.  raw_location, dim: (B, 3) each, dim = (h, w, l).
 *   weights (B, K) = 1 / d_k with d_k = sqrt(max(sum_c (f4_c / n4 - f6_c / n6)^2, 1e-30)), n = max(L2 norm over C, 1e-12): the
 *     diagonal of `pairwise_l2_dist` of the normalised features, in the difference form (the expanded one cancels for small d).
 *   pred_depth (B) = sum softmax(weights[good_idx]) * depths[good_idx]; pred_location (B, 3): y -= h/2, scale by pred_depth / z,
 *     y += h/2.  An index outside [0, K) makes that object's pred_depth and pred_location NaN.
 * Sums run in a fixed order; an object's result does not depend on B or on its place in the batch.
 * Status: DCD_ERR_BAD_ARG for a null pointer, B / C / K / num_k < 1 or num_k > K. */
int dcd_gmw_refine(void *stream, const float *f4, const float *f6, const float *depths, const long long *good_idx, int num_k,
                   const float *raw_location, const float *dim, int B, int C, int K, float *weights, float *pred_depth,
                   float *pred_location);

/* Decoded candidates -> GMW's inputs, written once (csrc/gmw.hip): what `edge_expand(x).transpose(-2, -1).contiguous()` and the
 * slices of the detector's rows give, for the records a batched evaluation keeps, straight from `dcd_decode_detections`' outputs.
 *   rows (n_rows, 14), k2 (n_rows, nk, 2), k3 (n_rows, nk, 3): the decode's outputs.  src: n int32 row numbers (device memory).
 *   The outputs are buffers of `cap` records; records dst0 .. dst0 + n - 1 are written, the others are left as they are.
 *   pair_i, pair_j: P = nk (nk - 1) / 2 int32 entries each, pair p = (pair_i[p], pair_j[p]) (`GMW.pair_i` / `pair_j` as int32).
 *   e4 (cap, 4, P): channels 0-1 = k2[src][i], 2-3 = k2[src][j].  e6 (cap, 6, P): channels 0-2 = k3[src][i], 3-5 = k3[src][j].
 *   k2_out (cap, nk, 2), k3_out (cap, nk, 3): copies.  rot (cap, 1) = column 12 of the row, loc (cap, 3) = columns 9-11,
 *   dim (cap, 3) = columns 6-8.
 * Data movement only: bit-equal to the torch chain; no atomics.  A src entry outside [0, n_rows) writes a zero record and reads
 * nothing; a table entry outside [0, nk) gives 0.  One workgroup per record; 16-byte stores when P % 4 == 0 and e4, e6 and the
 * tables are 16-byte aligned.
 * Status: DCD_OK without a launch for n == 0; DCD_ERR_BAD_ARG, without a launch, for a null pointer, a negative count,
 * dst0 + n > cap, nk < 2 or nk > 128. */
int dcd_gmw_pack_records(void *stream, const float *rows, const float *k2, const float *k3, int n_rows, int nk, const int *src, int n,
                         int dst0, int cap, const int *pair_i, const int *pair_j, float *e4, float *e6, float *k2_out, float *k3_out,
                         float *rot, float *loc, float *dim);

/* ------------------------------------------------------------------------------------------------
 * Batch normalisation fused with the residual add and ReLU that follow it.  Replaces the stock-op chains
 *   bn -> relu            DGDE/model/backbone/dla_dcn.py:91-93 (BasicBlock), :272-283 (conv levels), :403-410
 *                         (DeformConv.actf); DGDE/model/head/detector_predictor.py:52-60,112-120 (head trunks)
 *   bn -> (+residual) -> relu   dla_dcn.py:95-99 (BasicBlock), :199-205 (Root)
 *   bn                    dla_dcn.py:237-240 (Tree.project)
 * i.e. torch.nn.functional.batch_norm + add + relu and their autograd.  x, residual, y: (B,C,HW) fp32 contiguous
 * (NCHW with HW = H*W).  Statistics are exchanged as fp64 per-channel sums so that a multi-GPU job all-reduces
 * `stats` / `sums` (C x 2 doubles) between the two calls -- the SyncBatchNorm of MODEL.USE_SYNC_BN
 * (DGDE/tools/plain_train_net.py:56-57) -- and passes the global element count.
 *
 * dcd_bn_stats:           stats[c] = (sum x, sum x^2) over this rank's B*HW elements.
 * dcd_bn_train_apply:     mean = S0/count, var = S1/count - mean^2 (biased); y = act((x-mean)*rsqrt(var+eps)*w + b
 *                         [+ residual]); writes save_mean / save_invstd (C); when running_mean/var are given,
 *                         running = (1-momentum)*running + momentum*(mean | var*count/(count-1)) and
 *                         *num_batches_tracked += 1 (all nullable).  weight / bias nullable (1 / 0).
 * dcd_bn_eval_apply:      same formula with the running statistics.
 * dcd_bn_backward_stats:  sums[c] = (sum dz, sum dz*(x-mean)), dz = grad_y * [y > 0] when `y` (the forward output,
 *                         ReLU fused) is given, dz = grad_y when y is NULL.
 * dcd_bn_backward_apply:  grad_x = (dz - S0/count - (x-mean)*invstd^2*S1/count) * invstd * w;
 *                         grad_residual = dz (nullable); grad_weight = S1*invstd, grad_bias = S0 of THIS call's sums
 *                         (nullable; under SyncBN pass the local sums' result, see dcd_amd/norm.py).
 * workspace: dcd_bn_workspace_bytes(C) bytes of device scratch for the two-stage reductions.
 * ---------------------------------------------------------------------------------------------- */
size_t dcd_bn_workspace_bytes(int C);
int dcd_bn_stats(void *stream, const float *x, int B, int C, int64_t HW, double *stats, void *workspace,
                 size_t workspace_bytes);

/* sums[c] = sum over b and positions of x[b][c][...] (fp64 two-stage sum, rounded once): a bias gradient
 * (torch.autograd's grad_bias of the reference's nn.Conv2d, DGDE/model/backbone/DCNv2/dcn_v2.py:111-128 conv_offset_mask).
 * One launch.  workspace: dcd_bn_workspace_bytes(C) bytes whose SECOND half starts with C arrival counters (unsigned) that must
 * be ZERO on entry; the call leaves them zero, so a buffer zeroed once can be reused by later calls ON THE SAME STREAM (calls on
 * different streams need different buffers). */
int dcd_channel_sums(void *stream, const float *x, int B, int C, int64_t HW, float *sums, void *workspace, size_t workspace_bytes);
int dcd_bn_train_apply(void *stream, const float *x, const float *residual, const float *weight, const float *bias,
                       const double *stats, double count, float *running_mean, float *running_var,
                       int64_t *num_batches_tracked, float momentum, float eps, int relu, float *y, float *save_mean,
                       float *save_invstd, int B, int C, int64_t HW);
int dcd_bn_eval_apply(void *stream, const float *x, const float *residual, const float *weight, const float *bias,
                      const float *running_mean, const float *running_var, float eps, int relu, float *y, int B, int C,
                      int64_t HW);
int dcd_bn_backward_stats(void *stream, const float *grad_y, const float *y, const float *x, const float *save_mean,
                          int B, int C, int64_t HW, double *sums, void *workspace, size_t workspace_bytes);
/* dcd_bn_backward for a layer with fused ReLU and NO residual that does not read the forward output: the ReLU mask y > 0 is
 * recomputed as fma(x, scale, shift) > 0 from the saved statistics, weight and bias -- the forward's own expression -- so the
 * backward reads two tensors (grad_y, x) per pass instead of three.  (The reference's nn.BatchNorm2d + F.relu keep and read the
 * output, DGDE/model/backbone/dla_dcn.py:76-101.) */
int dcd_bn_backward_relu_from_x(void *stream, const float *grad_y, const float *x, const float *weight, const float *bias,
                                const float *save_mean, const float *save_invstd, float *grad_x, float *grad_weight, float *grad_bias,
                                int B, int C, int64_t HW, void *workspace, size_t workspace_bytes);
/* The two halves of the same backward under data parallelism (sums all-reduced in between), mask recomputed from x: */
int dcd_bn_backward_stats_params_relu_from_x(void *stream, const float *grad_y, const float *x, const float *weight, const float *bias,
                                             const float *save_mean, const float *save_invstd, int B, int C, int64_t HW, double *sums,
                                             float *grad_weight, float *grad_bias, void *workspace, size_t workspace_bytes);
int dcd_bn_backward_apply_relu_from_x(void *stream, const float *grad_y, const float *x, const float *weight, const float *bias,
                                      const float *save_mean, const float *save_invstd, const double *sums, double count, float *grad_x,
                                      int B, int C, int64_t HW);
/* dcd_bn_backward_stats that also writes THIS rank's parameter gradients from the same sums (grad_weight[c] = sum dz*(x-mean) *
 * invstd, grad_bias[c] = sum dz; either may be NULL): under data parallelism they stay local (DDP averages parameter gradients)
 * while `sums` is all-reduced for the input gradient -- torch.nn.SyncBatchNorm's backward, torch/nn/modules/_functions.py. */
int dcd_bn_backward_stats_params(void *stream, const float *grad_y, const float *y, const float *x, const float *save_mean,
                                 const float *save_invstd, int B, int C, int64_t HW, double *sums, float *grad_weight,
                                 float *grad_bias, void *workspace, size_t workspace_bytes);
int dcd_bn_backward_apply(void *stream, const float *grad_y, const float *y, const float *x, const float *weight,
                          const float *save_mean, const float *save_invstd, const double *sums, double count,
                          float *grad_x, float *grad_residual, float *grad_weight, float *grad_bias, int B, int C,
                          int64_t HW);
/* Batch-norm parameters of the head's regression trunks from the Gram form (model/head/trunk_moments.py; the reference runs the
 * eleven dense conv + BatchNorm2d trunks, DGDE/model/head/detector_predictor.py:78-101).  Row r = (trunk, output channel), R rows,
 * K = 9 Cin.  WG (R, K + 1) = W [G | S1] and Wd (R, K) = W, both fp64.
 *   row_sums:           sums (R, 2) = (sum y, sum y^2) = (WG[r][K], sum_k WG[r][k] Wd[r][k])   [all-reduced by the caller under SyncBN]
 *   finalize_forward:   stats (R, 3) = (mean, biased variance clamped at 0, 1 / sqrt(var + eps)); scale = gamma / sqrt(var + eps),
 *                       shift = beta - mean * scale (fp32)
 *   finalize_backward:  (grad_scale, grad_shift) -> grad_sums (R, 2) fp64, grad_gamma, grad_beta
 *   grad_wg:            grad_WG (R, K + 1): columns k < K = grad_sums[r][1] * Wd[r][k], column K = grad_sums[r][0] */
int dcd_trunk_row_sums(void *stream, const double *WG, const double *Wd, int R, int K, double *sums);
int dcd_trunk_finalize_forward(void *stream, const double *sums, const float *gamma, const float *beta, double count, double eps, int R,
                               float *scale, float *shift, double *stats);
int dcd_trunk_finalize_backward(void *stream, const float *grad_scale, const float *grad_shift, const float *gamma, const double *stats,
                                double count, int R, double *grad_sums, float *grad_gamma, float *grad_beta);
int dcd_trunk_grad_wg(void *stream, const double *grad_sums, const double *Wd, int R, int K, double *grad_WG);

/* BN (+ReLU), training mode, evaluated at listed positions only (the regression-head trunks: the loss reads their output at
 * the object centres and, for one head, the border cells).  pos (B,N) int64 linear pixel indices; x_at, y_at (B,N,C).
 * stats NULL: statistics computed here (workspace needed); else the C x 2 combined (all-reduced) sums with the global count.
 * Backward: dcd_bn_at_backward_sums -> [all-reduce sums] -> dcd_bn_backward_apply(grad_y = NULL: zeros, y = NULL) gives the
 * dense part of grad_x, and dzk (B*N,C) is scatter-added at the positions (dcd_poi_scatter_add). */
int dcd_bn_at_forward(void *stream, const float *x, const int64_t *pos, const float *weight, const float *bias,
                      const double *stats, double count, float *running_mean, float *running_var,
                      int64_t *num_batches_tracked, float momentum, float eps, int relu, float *x_at, float *y_at,
                      float *save_mean, float *save_invstd, int B, int C, int64_t HW, int N, void *workspace,
                      size_t workspace_bytes);
int dcd_bn_at_backward_sums(void *stream, const float *grad_at, const float *x_at, const float *y_at, const float *weight,
                            const float *save_mean, const float *save_invstd, int relu, int total, int C, double *sums,
                            float *dzk);
/* Single-rank shortcuts (no statistics exchange): stats + apply fused into two launches, the apply kernels sum the
 * partials of the two-stage reduction themselves.  Same arithmetic and outputs as the call pairs above with
 * count = B*HW. */
int dcd_bn_train_forward(void *stream, const float *x, const float *residual, const float *weight, const float *bias,
                         float *running_mean, float *running_var, int64_t *num_batches_tracked, float momentum, float eps,
                         int relu, float *y, float *save_mean, float *save_invstd, int B, int C, int64_t HW,
                         void *workspace, size_t workspace_bytes);
int dcd_bn_backward(void *stream, const float *grad_y, const float *y, const float *x, const float *weight,
                    const float *save_mean, const float *save_invstd, float *grad_x, float *grad_residual,
                    float *grad_weight, float *grad_bias, int B, int C, int64_t HW, void *workspace,
                    size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * 3x3 / stride 1 / pad 1 / dilation 1 / groups 1 convolution: forward and backward-data (Winograd
 * F(2x2,3x3) on the fp32 matrix pipe).  Replaces the stock `nn.Conv2d(.., 3, padding=1, bias=False)` calls of
 *   DGDE/model/backbone/dla_dcn.py:76-82 (BasicBlock.conv1/conv2 at stride 1) and
 *   DGDE/model/head/detector_predictor.py:52-58,112-118 (the 64->256 trunks of the class / regression heads) and
 *   DGDE/model/backbone/DCNv2/dcn_v2.py:107-116 (DCN's `conv_offset_mask`, Cin -> 27 with a bias),
 * i.e. torch's cudnn/MIOpen convolution and its input gradient (weight gradient: dcd_conv3x3_wrw below).
 * weight (Cout,Cin,3,3), bias (Cout) or NULL (forward only); residual: NULL or an image of the output's shape that is added to the
 * result (it may BE the output buffer: a gradient accumulated in place, what autograd's separate addition would do).
 *                         backward_data = 0: input (B,Cin,H,W) -> output (B,Cout,H,W);
 *                         backward_data = 1: input = grad_output (B,Cout,H,W) -> output = grad_input (B,Cin,H,W).
 * Requires W % 4 == 0 and H even (bad-argument otherwise).  workspace: dcd_conv3x3_workspace_bytes(B, Cin, H, W, Cout) bytes
 * (transformed weights; partial images when few regions make the call split its contraction), dead after the call's
 * kernels complete.
 * ---------------------------------------------------------------------------------------------- */
size_t dcd_conv3x3_workspace_bytes(int B, int Cin, int H, int W, int Cout);
int dcd_conv3x3(void *stream, const float *input, const float *weight, const float *bias, const float *residual, float *output,
                int B, int Cin, int H, int W, int Cout, int backward_data, void *workspace, size_t workspace_bytes);

/* The same convolution with its Winograd-domain weights prepared ahead: dcd_conv3x3 transforms the weights on every call (one
 * small launch); a training step can prepare both directions in ONE launch during the forward call and hand the backward-data
 * call its weights (they do not change in between).  transform_weights writes dcd_conv3x3_weights_bytes(Cin, Cout, direction)
 * bytes per requested direction (either output may be NULL); dcd_conv3x3_prepared is dcd_conv3x3 with `transformed` (the
 * buffer of ITS direction) in place of `weight`; its workspace (dcd_conv3x3_workspace_bytes, may then be smaller) only holds the
 * partial images of a split contraction. */
size_t dcd_conv3x3_weights_bytes(int Cin, int Cout, int backward_data);
int dcd_conv3x3_transform_weights(void *stream, const float *weight, int Cin, int Cout, float *forward_out, float *backward_out);
/* transform_weights for MANY layers in one launch (a train step: once, right after the optimizer step, instead of one launch
 * per layer).  table: DEVICE array of `entries` records of five 64-bit words {weight pointer, forward_out pointer,
 * backward_out pointer, Cin, Cout}; either output pointer may be 0.  The table is read by the kernel: keep it alive and
 * unchanged until the launch has run. */
int dcd_conv3x3_transform_weights_table(void *stream, const long long *table, int entries);
int dcd_conv3x3_prepared(void *stream, const float *input, const float *transformed, const float *bias, const float *residual,
                         float *output, int B, int Cin, int H, int W, int Cout, int backward_data, void *workspace,
                         size_t workspace_bytes);

/* The same convolution with the Winograd-domain products in split-bf16 (hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16, fp32
 * accumulate: ~2^-16 relative per product, the form DCD_PREC_BF16X3 names for the deformable convolution): transforms stay fp32,
 * operands stay fp32 in HBM.  Weights are prepared in their own layout (dcd_conv3x3_split_weights_bytes /
 * dcd_conv3x3_split_transform_weights: both directions, either pointer may be NULL); workspace holds the partial images of a
 * split contraction only.  Same shape rules as dcd_conv3x3.
 * precision: DCD_PREC_BF16X3, or DCD_PREC_BF16 = one product of bf16-rounded operands (the same prepared weights: their low halves
 * are not read). */
size_t dcd_conv3x3_split_weights_bytes(int Cin, int Cout, int backward_data);
int dcd_conv3x3_split_transform_weights(void *stream, const float *weight, int Cin, int Cout, void *forward_out, void *backward_out);
/* The split-layout transform for many layers in ONE launch: the table of dcd_conv3x3_transform_weights_table (five 64-bit words per
 * entry: weight, forward_out, backward_out, Cin, Cout) with the layer's split-layout buffers as outputs. */
int dcd_conv3x3_split_transform_weights_table(void *stream, const long long *table, int entries);
size_t dcd_conv3x3_split_workspace_bytes(int B, int Cin, int H, int W, int Cout);
int dcd_conv3x3_split_prepared(void *stream, const float *input, const void *transformed, const float *bias, const float *residual,
                               float *output, int B, int Cin, int H, int W, int Cout, int backward_data, int precision, void *workspace,
                               size_t workspace_bytes);

/* The ONE-product form (DCD_PREC_BF16, MODEL.FP16: DGDE/model/detector.py:34-36) as a DIRECT implicit GEMM on
 * v_mfma_f32_32x32x16_bf16 (csrc/conv_direct_bf16.inc): inputs and weights rounded to bf16 once (nearest even), no Winograd
 * transform -- on the bf16 matrix pipe the transform's vector / LDS work, not the multiplies, was the kernel's time -- fp32
 * accumulate, fp32 tensors in HBM.  Own weight layout (both directions, either pointer may be NULL; the table form takes the
 * five-word entries of dcd_conv3x3_transform_weights_table with buffers of dcd_conv3x3_bf16_weights_bytes); workspace: the partial
 * images of a split contraction.  W % 4 == 0; any Cin / Cout / H with (max(Cin, Cout) + 16) H W < 2^29; a split contraction
 * (dcd_conv3x3_bf16_workspace_bytes > 16) needs B Cout H W % 4 == 0.  bias only with backward_data == 0. */
size_t dcd_conv3x3_bf16_weights_bytes(int Cin, int Cout, int backward_data);
int dcd_conv3x3_bf16_transform_weights(void *stream, const float *weight, int Cin, int Cout, void *forward_out, void *backward_out);
int dcd_conv3x3_bf16_transform_weights_table(void *stream, const long long *table, int entries);
size_t dcd_conv3x3_bf16_workspace_bytes(int B, int Cin, int H, int W, int Cout);
int dcd_conv3x3_bf16_prepared(void *stream, const float *input, const void *transformed, const float *bias, const float *residual,
                              float *output, int B, int Cin, int H, int W, int Cout, int backward_data, void *workspace,
                              size_t workspace_bytes);

/* 1x1 convolutions (DLA's Roots and projections: DGDE/model/backbone/dla_dcn.py:187-207, 239-245) in the one-product form
 * (DCD_PREC_BF16; csrc/conv1x1_bf16.inc), fp32 tensors, operands rounded to bf16, fp32 accumulate:
 *   dcd_conv1x1_bf16      output (B, M, HW) = A x, x = the concatenation along the channels of n_inputs (<= 4) tensors
 *                         (B, channels[i], HW) that is never formed; A[m][k] = weight[m * ldw + k], or weight[k * ldw + m] when
 *                         `transposed` (the input gradient of a column slice: pass weight + first column).  inputs / channels are
 *                         HOST arrays.  HW % 4 == 0, channels[i] % 16 == 0.
 *   dcd_conv1x1_wrw_bf16  grad_weight[o * ldw + c] = sum_{b, p} grad_output[b][o][p] input[b][c][p] (overwrites the O x C block;
 *                         partial sums in a fixed order); workspace: dcd_conv1x1_wrw_bf16_workspace_bytes. */
int dcd_conv1x1_bf16(void *stream, const float *weight, int ldw, int transposed, int n_inputs, const float *const *inputs,
                     const int *channels, float *output, int B, int M, long long HW);
size_t dcd_conv1x1_wrw_bf16_workspace_bytes(int B, int O, int C, long long HW);
int dcd_conv1x1_wrw_bf16(void *stream, const float *grad_output, const float *input, float *grad_weight, int ldw, int B, int O, int C,
                         long long HW, void *workspace, size_t workspace_bytes);

/* The same layers in EXACT fp32 (csrc/conv1x1_f32.inc, v_mfma_f32_32x32x2_f32; round 6): same arguments, same restrictions.  They
 * replace, in the fp32 train step, the batched library GEMMs behind `torch.cat` + `nn.Conv2d(.., 1)` of the reference's Root
 * (DGDE/model/backbone/dla_dcn.py:199-205): one launch over all concatenated inputs instead of one GEMM per input. */
int dcd_conv1x1_f32(void *stream, const float *weight, int ldw, int transposed, int n_inputs, const float *const *inputs,
                    const int *channels, float *output, int B, int M, long long HW);
size_t dcd_conv1x1_wrw_f32_workspace_bytes(int B, int O, int C, long long HW);
int dcd_conv1x1_wrw_f32(void *stream, const float *grad_output, const float *input, float *grad_weight, int ldw, int B, int O, int C,
                        long long HW, void *workspace, size_t workspace_bytes);

/* 3x3 / stride 2 / pad 1 convolution in exact fp32 (csrc/conv_s2_f32.inc, round 6): the first convolution of every DLA level
 * (DGDE/model/backbone/dla_dcn.py:76-78, 313-326: `nn.Conv2d(c, k, 3, stride=2, padding=1, bias=False)`).  No LDS for the
 * activations: a lane's nine taps x four output pixels are 27 registers of one channel.  input (B, Cin, H, W) -> output
 * (B, Cout, H/2, W/2); H even, W % 8 == 0, Cin % 16 == 0. */
int dcd_conv3x3_s2_f32(void *stream, const float *input, const float *weight, float *output, int B, int Cin, int H, int W, int Cout);
/* ... its input gradient (grad_output (B, Cout, H/2, W/2) -> grad_input (B, Cin, H, W), every element written; Cout % 16 == 0 too) and
 * its weight gradient (grad_weight (Cout, Cin, 3, 3) overwritten; partial sums per pixel split in a fixed order; H % 4 == 0;
 * workspace: dcd_conv3x3_s2_f32_wrw_workspace_bytes). */
int dcd_conv3x3_s2_f32_backward_data(void *stream, const float *grad_output, const float *weight, float *grad_input, int B, int Cin, int H,
                                     int W, int Cout);
size_t dcd_conv3x3_s2_f32_wrw_workspace_bytes(int B, int Cin, int H, int W, int Cout);
int dcd_conv3x3_s2_f32_wrw(void *stream, const float *input, const float *grad_output, float *grad_weight, int B, int Cin, int H, int W,
                           int Cout, void *workspace, size_t workspace_bytes);

/* Weight gradient of the same convolution (torch's `convolution_backward(..., output_mask=[0,1,0])` for those call sites),
 * also in the Winograd domain: grad_weight (Cout,Cin,3,3) = correlation of input (B,Cin,H,W) with grad_output (B,Cout,H,W).
 * Overwrites grad_weight; the partial sums of the workgroups are added in a fixed order (bitwise reproducible).
 * Same shape requirements; workspace: dcd_conv3x3_wrw_workspace_bytes(B, Cin, H, W, Cout) bytes, dead after the call.
 * precision: DCD_PREC_F32 exact; DCD_PREC_BF16 the sixteen Winograd-domain products on v_mfma_f32_32x32x16_bf16 with both transformed
 * operands rounded to bf16 (fp32 accumulate over the tiles); DCD_PREC_BF16X3 runs the exact kernel. */
size_t dcd_conv3x3_wrw_workspace_bytes(int B, int Cin, int H, int W, int Cout);
int dcd_conv3x3_wrw(void *stream, const float *input, const float *grad_output, float *grad_weight, int B, int Cin, int H, int W,
                    int Cout, int precision, void *workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * The low-channel, full-resolution convolutions of DLA-34's stem (csrc/stem.hip, v_mfma_f32_16x16x4_f32):
 *   base_layer Conv2d(3, 16, 7, padding 3, bias=False)  DGDE/model/backbone/dla_dcn.py:236-240   (Cin 3,  ksize 7)
 *   level0     Conv2d(16, 16, 3, padding 1, bias=False) DGDE/model/backbone/dla_dcn.py:241-242   (Cin 16, ksize 3)
 * i.e. torch's conv2d / convolution_backward for those two call sites; any other (Cin, Cout, ksize) is a bad argument.
 * stride 1, padding ksize/2, W % 4 == 0.  weight (16,Cin,k,k).  backward_data (Cin 16 only): input = grad_output -> output =
 * grad_input.  dcd_conv_stem_wrw overwrites grad_weight (partials are combined with float atomics: order-dependent rounding).
 * Workspaces: dcd_conv_stem_workspace_bytes / dcd_conv_stem_wrw_workspace_bytes, dead after the call's kernels complete.
 * ---------------------------------------------------------------------------------------------- */
size_t dcd_conv_stem_workspace_bytes(int Cin, int Cout, int ksize);
int dcd_conv_stem(void *stream, const float *input, const float *weight, float *output, int B, int Cin, int H, int W, int Cout,
                  int ksize, int backward_data, void *workspace, size_t workspace_bytes);
size_t dcd_conv_stem_wrw_workspace_bytes(int Cin, int Cout, int ksize);
int dcd_conv_stem_wrw(void *stream, const float *input, const float *grad_output, float *grad_weight, int B, int Cin, int H, int W,
                      int Cout, int ksize, void *workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * Depthwise transposed convolution of IDAUp: nn.ConvTranspose2d(C, C, 2f, stride=f, padding=f/2, groups=C, bias=False)
 * (DGDE/model/backbone/dla_dcn.py:416-421; weights from fill_up_weights :386-395, learnable), f in {2,4,8}.
 * x (B,C,H,W) -> y (B,C,H*f,W*f); weight (C,1,2f,2f).  Requires (W*f) % 4 == 0.  Backward overwrites grad_x and grad_weight.
 * ---------------------------------------------------------------------------------------------- */
int dcd_upsample_dw_forward(void *stream, const float *x, const float *weight, float *y, int B, int C, int H, int W, int f);
/* y = up(x) + skip: the sum that feeds IDAUp's node (`layers[i] = node(layers[i] + layers[i-1])`, dla_dcn.py:430-436) leaves the
 * up-sampling kernel directly; skip (B, C, H*f, W*f). */
int dcd_upsample_dw_forward_add(void *stream, const float *x, const float *weight, const float *skip, float *y, int B, int C, int H,
                                int W, int f);

/* 2x2 / stride-2 max pooling of (planes, H, W) maps (H even, W % 4 == 0): the `downsample` of every DLA Tree
 * (`nn.MaxPool2d(stride, stride=stride)`, DGDE/model/backbone/dla_dcn.py:228).  The backward re-derives the arg-max from x
 * (first maximum in scan order, NaN takes over: the stock kernel's rule) instead of keeping an index tensor. */
int dcd_maxpool2x2_forward(void *stream, const float *x, float *y, int64_t planes, int H, int W);
int dcd_maxpool2x2_backward(void *stream, const float *x, const float *grad_y, float *grad_x, int64_t planes, int H, int W);
int dcd_upsample_dw_backward(void *stream, const float *x, const float *weight, const float *grad_y, float *grad_x,
                             float *grad_weight, int B, int C, int H, int W, int f);

/* ------------------------------------------------------------------------------------------------
 * Training-target encoding of a whole batch on the device (csrc/targets.hip).
 * Replaces the numpy work of `KITTIDataset.__getitem__` (DGDE/data/datasets/kitti.py:354-606): box / key-point projection and
 * visibility, truncated-object centres (`approx_proj_center`, kitti_utils.py:1040-1078), Gaussian heat map
 * (`gaussian_radius`, `draw_umich_gaussian`, `draw_umich_gaussian_2D`, DGDE/model/heatmap_coder.py:37-124), multi-bin
 * orientation (`encode_alpha_multibin`, kitti.py:225-244) and the border walk (`get_edge_utils`, kitti.py:165-223).
 *   objs     (B, M, 16) float64: truncation, occlusion, box x1 y1 x2 y2, h, w, l, t x y z, ry, alpha, find_pcl, class id
 *            (the values an `Object3d` holds, kitti_utils.py:61-113; box and t are float32 there and are rounded as such)
 *   kpts3d   (B, M, n_extra, 3) float64  object-frame key points, already shifted by -h/2 (kitti_utils.py:112)
 *   P        (B, 3, 4) float64; img_size (B, 2) int32 (w, h) before padding; n_obj (B) int32 objects per image (<= M)
 *   outputs  26 device pointers, caller-allocated, ALL ZERO-FILLED except ori_mask (which the caller keeps as ones), in this
 *            order: hm (B,n_classes,H/down,W/down) f32 | cls_ids (B,M) i32 | target_centers (B,M,2) i32 | gt_bboxes (B,M,4) f32 |
 *            2d_bboxes (B,M,4) f32 | keypoints (B,M,10,3) f32 | keypoints_depth_mask (B,M,3) f32 | extra_kpts_2d (B,M,K,3) f32 |
 *            extra_kpts_3d (B,M,K,3) f32 | extra_kpts_depth_mask (B,M,K) f32 | Calib_P (B,M,3,4) f32 | find_pcl (B,M) u8 |
 *            dimensions (B,M,3) f32 | locations (B,M,3) f32 | rotys (B,M) f32 | alphas (B,M) f32 | offset_3D (B,M,2) f32 |
 *            occlusions (B,M) f64 | truncations (B,M) f64 | orientations (B,M,8) f32 | reg_mask (B,M) u8 | trunc_mask (B,M) u8 |
 *            reg_weight (B,M) f32 | pad_size (B,2) i64 | edge_indices (B,2(W+H)/down,2) i64 | edge_len (B) i64;  K = n_extra + 10.
 * The configuration is the reference's: INPUT.HEATMAP_CENTER '3D', KEYPOINT_VISIBLE_MODIFY, ADJUST_BOUNDARY_HEATMAP,
 * CONSIDER_OUTSIDE_OBJS with APPROX_3D_CENTER 'intersect', ORIENTATION 'multi-bin' with 4 bins (anything else: bad argument).
 * ---------------------------------------------------------------------------------------------- */
int dcd_encode_targets(void *stream, const double *objs, const double *kpts3d, const double *P, const int32_t *img_size,
                       const int32_t *n_obj, int B, int M, int n_extra, int in_w, int in_h, int down_ratio, double filter_trunc,
                       double filter_size, double edge_heatmap_ratio, int num_bin, int n_classes, void *const *outputs,
                       int n_outputs);

/* ------------------------------------------------------------------------------------------------
 * The image half of the input pipeline on the device (csrc/images.hip): B decoded uint8 frames of different sizes -> the
 * network's input batch, one launch.  Replaces, per sample, the image side of `RandomHorizontallyFlip`
 * (DGDE/data/augmentations/augmentations.py:33-36), `KITTIDataset.pad_image` (DGDE/data/datasets/kitti.py:262-272) and
 * `ToTensor` + `Normalize` with `TO_BGR` (DGDE/data/transforms/transforms.py:14-30, transforms/build.py,
 * INPUT.PIXEL_MEAN / PIXEL_STD / TO_BGR).
 *   src      one device buffer of src_bytes bytes holding the frames: packed uint8 RGB, HWC, rows `pitch` bytes apart
 *   images   (B, 5) int64 on the device, per image: byte offset of its first pixel in src, row pitch in bytes (>= 3 w),
 *            height, width (each <= in_h / in_w), flip (0 / 1: mirror the columns).  An image whose record does not lie inside
 *            [0, src_bytes) or exceeds the canvas is read as empty (all border); nothing outside src is ever read.
 *   table    (3, 256) fp32 on the device: table[k][v] = the normalised value of byte v in SOURCE channel k, built by the caller
 *            with the reference's own operations (`arange(256, dtype=uint8).float().div(255).sub(mean[k]).div(std[k])`), so the
 *            kernel has no arithmetic of its own and the output is bit-equal to the reference's.
 *   out      (B, 3, in_h, in_w) fp32, fully overwritten.  With pad_x = (in_w - w) / 2, pad_y = (in_h - h) / 2 (kitti.py:266-267):
 *            out[b][c][y][x] = table[k][v], k = to_bgr ? 2 - c : c, v = byte k of the source pixel at row y - pad_y, column
 *            x - pad_x (flip: w - 1 - (x - pad_x)), or 0 outside the image -- the reference pads the uint8 canvas before it
 *            normalises and normalises before it permutes the planes.
 * 16-byte stores when in_w % 4 == 0 and out is 16-byte aligned, scalar stores otherwise; same results.  No workspace.
 * ---------------------------------------------------------------------------------------------- */
int dcd_preprocess_images(void *stream, const uint8_t *src, int64_t src_bytes, const int64_t *images, const float *table, int B,
                          int in_h, int in_w, int to_bgr, float *out);

/* ------------------------------------------------------------------------------------------------
 * KITTI average precision on the device (csrc/eval.hip).  Replaces the two slow loops of the
 * reference's evaluator, DGDE/data/datasets/evaluation/kitti_object_eval_python: `calculate_iou_partly` (eval.py:338-412) with
 * its numba.cuda kernel `rotate_iou_kernel_eval` (rotate_iou.py:264-296), and `compute_statistics_jit` (eval.py:155-273) as
 * `eval_class` drives it.  All images of a split travel together as concatenated arrays with per-image offset tables
 * (n_img + 1 entries each, first 0): gt_off / dt_off / dc_off int32 count ground-truth, detection and DontCare boxes, pair_off
 * int64 counts dt_i * gt_i.  G, D, n_dc, P are the totals (the last entries).  Nothing is allocated, copied or synchronised.
 *
 * dcd_eval_overlaps: out (3, P) float64; image i's block out[m][pair_off[i] ...] is laid out [dt, gt], the `overlaps[j, i]` of
 *   compute_statistics_jit.  m = 0: `image_box_overlap` criterion -1 (eval.py:84-111) in float64 on box2d (., 4) x1 y1 x2 y2.
 *   m = 1: `bev_box_overlap`, m = 2: `d3_box_overlap` (eval.py:114-152) on box3d (., 7) float64 x y z l h w ry (location,
 *   dimensions in the l h w order of kitti_common.py:325-327, rotation_y).  The rotated intersection area is computed once, in
 *   float32 on float32-rounded x z l w ry as the reference does (rotate_iou.py:314-315), by clipping the detection against
 *   the ground-truth box in that box's own frame (never more than 8 vertices; coincident boxes give 1, touching boxes 0,
 *   where the reference's vertex collection loses points); height overlap, areas and volumes are float64.  P == 0 is
 *   valid and launches nothing.
 * dcd_eval_match: one wave per (image, combination).  comb (n_comb, 3) int32: metric 0..2, row of the ignore tables, slot of
 *   the similarity output or -1 (read by mode DCD_EVAL_MATCH_COUNTS only); min_overlap (n_comb) float64, >= 0.  ign_gt (n_rows, G) / ign_dt (n_rows, D) int8 are the
 *   0 / 1 / -1 flags of `clean_data` (eval.py:28-81) per (class, difficulty); overlaps is dcd_eval_overlaps' output (or any
 *   (3, P) float64 of that layout); dc_box (n_dc, 4) the DontCare boxes.  max_dt: the largest detection count of one image,
 *   at most 4096.
 *     mode DCD_EVAL_MATCH_SCORES (compute_fp = False, thresh = 0): scores (n_comb, G) float64, fully written: the score of the
 *       detection assigned to each ground-truth box as a true positive, else -1e7.
 *     mode DCD_EVAL_MATCH_COUNTS (compute_fp = True): thresholds (n_comb, T) float64 with n_thresh (n_comb) valid entries per
 *       row, T <= 41.  counts (n_comb, T, 3) int32 tp fp fn, ZEROED BY THE CALLER, summed over images with integer atomics
 *       (the DontCare stage of eval.py:246-260 included, criterion-0 overlap in float64, metric 0 only).  sim_part
 *       (n_img, n_slots, T) float64, written for every combination with a slot: the image's AOS similarity sum
 *       (eval.py:261-270, 0 where the reference returns -1 and past n_thresh).  No floating-point atomics.
 * dcd_eval_sum_similarity: out[k] = sum_i part[i][k] for part (n_img, n), in image order: bit-identical from run to run.
 * Status: DCD_ERR_BAD_ARG for a null pointer that is needed, a negative size, T > 41, n_comb > 65535, max_dt > 4096.
 * ---------------------------------------------------------------------------------------------- */
#define DCD_EVAL_MATCH_SCORES 0
#define DCD_EVAL_MATCH_COUNTS 1
#define DCD_EVAL_MAX_THRESHOLDS 41
typedef struct {
    int mode, n_img, n_comb, n_rows, G, D, n_dc, max_dt, T, n_slots;
    int64_t P;
    const int32_t *gt_off, *dt_off, *dc_off;
    const int64_t *pair_off;
    const double *overlaps;
    const int8_t *ign_gt, *ign_dt;
    const double *dt_score, *gt_alpha, *dt_alpha, *dt_box2d, *dc_box;
    const int32_t *comb;
    const double *min_overlap, *thresholds;
    const int32_t *n_thresh;
    double *scores;
    int32_t *counts;
    double *sim_part;
} dcd_eval_match_args;
int dcd_eval_overlaps(void *stream, int n_img, const int32_t *gt_off, const int32_t *dt_off, const int64_t *pair_off, int G, int D,
                      int64_t P, const double *gt_box2d, const double *dt_box2d, const double *gt_box3d, const double *dt_box3d,
                      double *out);
int dcd_eval_match(void *stream, const dcd_eval_match_args *args);
int dcd_eval_sum_similarity(void *stream, const double *part, int n_img, int n, double *out);

/* ------------------------------------------------------------------------------------------------
 * The optimizer end of the train step (csrc/optim.hip): `torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)` followed by
 * `AdamW.step()` (DGDE/engine/trainer.py:144-147; DGDE/solver/__init__.py:10-62: AdamW, betas (0.9, 0.99), one learning rate per
 * parameter) over LISTS of fp32 tensors.  The host arrays of pointers / element counts are read during the call only (they travel
 * in the kernel arguments); every tensor has fewer than 2^31 elements.
 *
 * dcd_clip_grad_norm_scalars: 2-norm over all listed gradients -> scal[0] = the norm, scal[1] = min(1, max_norm / (norm + 1e-6))
 *   (1 when max_norm <= 0: no clipping), scal[2] = 1 when the norm is not finite else 0; three floats on the device.  The gradients
 *   are not touched here.  workspace: dcd_clip_adamw_workspace_bytes(ntensors, numel) bytes, dead after the call.
 * dcd_adamw_apply: one parameter group.  Unless scal[2] is set (then NOTHING changes: the library's found_inf contract), every
 *   listed step counter (a float on the device each, as the library's capturable AdamW keeps them) += 1 and
 *     g *= scal[1] (written back only when < 1)         p -= lr * weight_decay * p
 *     m = beta1 m + (1 - beta1) g                       v = beta2 v + (1 - beta2) g^2
 *     p -= (lr / (1 - beta1^step)) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 *   in the library's fused kernel's order and types (double hyper-parameters against float operands).  lr: a float on the device. */
size_t dcd_clip_adamw_workspace_bytes(int ntensors, const int64_t *numel);
int dcd_clip_grad_norm_scalars(void *stream, int ntensors, const void *const *grads, const int64_t *numel, float max_norm, void *workspace,
                               size_t workspace_bytes, float *scal);
int dcd_adamw_apply(void *stream, int ntensors, void *const *params, void *const *grads, void *const *exp_avg, void *const *exp_avg_sq,
                    void *const *steps, const int64_t *numel, const float *lr, double beta1, double beta2, double eps, double weight_decay,
                    const float *scal);

/* ------------------------------------------------------------------------------------------------
 * One batch out of tables that stay on the device (csrc/resident.hip; dcd_amd/data/resident.py keeps a decoded KITTI split
 * there: the image kernel's records, the raw label values of `dcd_encode_targets`, one row per (image, flip)).  For every
 * table t < n_tables (1 .. 8) and every b < B (1 .. 65535): row b of dst[t] = row index[b] of src[t], rows of row_bytes[t] bytes,
 * all tables in ONE launch.
 *   src, dst   HOST arrays of n_tables device pointers, each 4-byte aligned; src[t] holds src_rows[t] rows, dst[t] B rows
 *   row_bytes  HOST array, each > 0 and a multiple of 4;  src_rows  HOST array, each >= 0
 *   index      (B) int32 ON THE DEVICE.  An index outside [0, src_rows[t]) gives a zero row in table t: nothing outside src is
 *              ever read, nothing outside dst[t][0 : B * row_bytes[t]] is ever written.
 * The host arrays are read during the call only (they travel in the kernel arguments), so the call needs no copy and may be
 * captured in a graph: a replay follows what `index` holds at that time.  16-byte accesses for a table whose row_bytes is a
 * multiple of 16 and whose two bases are 16-byte aligned, 4-byte accesses otherwise; same results.  No workspace.
 * ---------------------------------------------------------------------------------------------- */
int dcd_gather_rows(void *stream, int n_tables, const void *const *src, void *const *dst, const int64_t *row_bytes,
                    const int64_t *src_rows, const int32_t *index, int B);

/* ------------------------------------------------------------------------------------------------
 * The Sinkhorn forward of the transport layer without the host (csrc/transport.hip; GMW/lib/optimal_transport.py:52-75).
 *   K = exp(-lambda min(M, max_distance));  u = r, previous = 1;
 *   before an iteration: stop when every |u - previous| <= tolerance over the WHOLE batch, or after max_iterations;
 *   an iteration: previous = u, u = r / (K (c / K^T u));   at the end P = diag(u) K diag(c / K^T u).
 * ONE call enqueues everything (2 max_iterations + 4 launches) and reads nothing back: the stop is a flag per iteration on the
 * device, raised with an integer atomic by the kernel that updates u; the launches after the stop return at once.  No kernel
 * waits for another workgroup.  Every sum runs in a fixed order without floating-point atomics: two calls give the same bits, and
 * an object's plan depends on its batch mates through the iteration count only.
 *   M, P        (batch, m, n) fp32, contiguous, distinct (K is built in P's buffer and scaled in place); m, n >= 1, m n < 2^31
 *   r, c        (batch, m) and (batch, n) fp32, positive
 *   iterations  one int ON THE DEVICE (or NULL): the number of updates of u that ran
 *   max_iterations  0 .. 4096;  batch 1 .. 65535
 *   workspace   dcd_sinkhorn_workspace_bytes(batch, m, n) bytes, 16-byte aligned, dead after the call
 * 16-byte accesses when n % 4 == 0 and M and P are 16-byte aligned, 4-byte accesses otherwise; the same bits either way.
 * ---------------------------------------------------------------------------------------------- */
size_t dcd_sinkhorn_workspace_bytes(int batch, int m, int n);
int dcd_sinkhorn(void *stream, const float *M, const float *r, const float *c, float *P, int batch, int m, int n, float lambda,
                 float max_distance, float tolerance, int max_iterations, int *iterations, void *workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * The eval-time decode of a whole batch in ONE launch (csrc/decode.hip, arithmetic in csrc/decode_math.h): everything
 * `PostProcessor._decode` does after the top-K and the POI gather (DGDE/model/head/detector_infer.py:104-213 with the helpers of
 * DGDE/model/anno_encoder.py): 2-D box, dimensions, direct and key-point depths, the inverse-uncertainty fusion, multi-bin
 * orientation, the nk dense key points, the edge-constraint depth as the mean over all nk (nk - 1) / 2 pairs (the per-pair
 * expression of dcd_edge_depth_forward with the clamp [2, 80], minus P[2][3]; the pair tensor is never written), the final
 * location and the KITTI row.  One workgroup per candidate, B * K candidates; ALL of them are decoded: the score threshold is the
 * caller's, nothing is counted, nothing is read back.
 *   vectors      (B K, C) fp32: the regression heads at the top-K cells
 *   scores, classes, ys, xs   (B K) fp32 each, as dcd_heatmap_topk writes them
 *   image_table  (B, 16) fp32: pad_x, pad_y, width, height, P (3 x 4 row-major) of each image
 *   args         the struct below, read during the call only (it travels in the kernel arguments)
 *   rows         (B K, 14): class, alpha, x1, y1, x2, y2, h, w, l, x, y, z, roty, score
 *   aux          (B K, 4): raw score, estimated depth error, confidence 1 - clamp(error, 0.01, 1), arg-max index of 1 / sigma
 *   kpts2d, kpts3d   (B K, nk, 2) K-normalised key points (each row with ITS image's intrinsics) and (B K, nk, 3); written when
 *                args->records is set, may be NULL otherwise
 * The pair mean is a fixed-order sum (per-lane partials in pair order, then a tree) without floating-point atomics: two calls
 * give the same bits.  A candidate's outputs depend on its own inputs only; a non-finite or huge vector gives non-finite
 * outputs for that candidate and touches nothing else.
 * Status: DCD_ERR_BAD_ARG, without a launch, for a null pointer, B < 1, K < 1 or K > 128, nk < 2 or nk > 128, B K > 2^31 - 1,
 * n_bins outside 1 .. 4, num_classes outside 1 .. 8, a channel range outside [0, C), an orientation other
 * than DCD_DECODE_ORI_MULTIBIN (head-axis is not supported: the caller keeps its op-by-op decode) or an unknown mode.
 * ---------------------------------------------------------------------------------------------- */
#define DCD_DECODE_MAX_CLASSES 8
#define DCD_DECODE_ORI_MULTIBIN 0
#define DCD_DECODE_ORI_HEAD_AXIS 1
#define DCD_DECODE_DIM_NONE 0
#define DCD_DECODE_DIM_EXP 1
#define DCD_DECODE_DIM_LINEAR 2
#define DCD_DECODE_DEPTH_INV_SIGMOID 0
#define DCD_DECODE_DEPTH_EXP 1
#define DCD_DECODE_DEPTH_LINEAR 2
typedef struct {
    int B, K, C, nk, n_bins, num_classes;
    /* first channel of each head in a row of `vectors` (key2channel): 2d_dim (4), 3d_offset (2), corner_offset (20),
     * corner_uncertainty (3), 3d_dim (3), ori_cls (2 n_bins), ori_offset (2 n_bins), depth (1), depth_uncertainty (1),
     * extra_kpts_2d (2 nk), extra_kpts_3d (3 nk) */
    int ch_box2d, ch_offset, ch_corner, ch_corner_unc, ch_dims, ch_ori_cls, ch_ori_off, ch_depth, ch_depth_unc, ch_kpts2d, ch_kpts3d;
    int orientation, dim_mode, dim_std_on, depth_mode;       /* DCD_DECODE_* ; dim_std_on: offset * std + mean instead of offset * mean */
    int uncertainty_as_conf, records;
    float down_ratio, depth_lo, depth_hi, eps;
    float depth_ref[2];
    float dim_mean[DCD_DECODE_MAX_CLASSES][3], dim_std[DCD_DECODE_MAX_CLASSES][3];
} dcd_decode_args;
int dcd_decode_detections(void *stream, const float *vectors, const float *scores, const float *classes, const float *ys,
                          const float *xs, const float *image_table, const dcd_decode_args *args, float *rows, float *aux,
                          float *kpts2d, float *kpts3d);

/* ------------------------------------------------------------------------------------------------
 * GMW's training records of a batch, collected on the device (csrc/records.hip, arithmetic in csrc/records_math.h): what
 * `Loss_Computation.prepare_predictions` + `generate_data` compute under TEST.GENERATE_GMW (DGDE/model/head/detector_loss.py:148-173,
 * :217-403), from the regression heads at the objects' centres and the target tables, appended to six tables in device memory.
 * One call enqueues three launches and reads nothing back:
 *   1. prepare, one wave per slot (b, m): the key points in image pixels ((kp + centre + GT offset) * 4 - pad), the 3-D key
 *      points, the TARGET yaw and Calib_P[b, m] in the solver's input layout; an empty slot gets zeros and a unit P;
 *   2. the edge solver of dcd_edge_depth_forward in its training form over all B M slots: top 1 500 pairs (all pairs where nk
 *      has fewer), clamp [2, 80], not normalised, minus P[2][3];
 *   3. finish, one wave per slot: the mean of the slot's kept depths as a fixed-order sum (per-lane partials in rank order, then
 *      a tree: no floating-point atomics, two calls give the same bits), pred_location and gt_location
 *      (decode_location_flatten), pred_rot (multi-bin decode_axes_orientation, wrapped to [-pi, pi]), the key points normalised
 *      with the intrinsics of IMAGE 0 of the batch (the reference's rule), and the row stores.
 * The finish kernel compacts: the record of slot s goes to row cursor + (number of set reg_mask bytes before s), so records
 * appear in ascending (b, m) order behind those of the earlier calls.  A row >= cap is not written; the cursor advances all
 * the same, so the caller sees the overflow when it reads the cursor.  No atomics: every workgroup counts the mask bytes
 * before its slot itself, and the cursor is a pair -- call number `call` reads cursor[call & 1], and one workgroup writes
 * cursor[(call + 1) & 1] = that + this call's count and per_call[call] = this call's count.  Before call 0 the caller sets
 * cursor[0] = 0; calls are numbered 0, 1, 2, ... on one stream.
 *   reg_pois        (B, M, C) fp32: the regression heads at the target centres
 *   reg_mask (B, M) u8, target_centers (B, M, 2) i32, offset_3D (B, M, 2), rotys (B, M), locations (B, M, 3),
 *   calib_P (B, M, 3, 4) fp32, pad_size (B, 2) i64: the target tables;  calib (B, 6) fp32 rows [c_u, c_v, f_u, f_v, b_x, b_y]
 *   image_numbers   (B) i32: what the `image` table receives for the records of image b
 *   kpts_2d (cap, nk, 2), kpts_3d (cap, nk, 3), pred_rot (cap, 1), gt_location (cap, 3), pred_location (cap, 3), image (cap) i32
 *   workspace       dcd_gmw_train_records_workspace_bytes(B, M, nk) bytes (0 for sizes the call refuses), 4-byte aligned,
 *                   dead after the call: B M x (nk x 5 + 13 + 2 x kept pairs) words -- the solver's inputs, its depths and the
 *                   pair indices it writes beside them
 * kpts_3d is a copy of the channels, bit for bit.  Nothing outside the first `cap` rows of the six tables, cursor[(call + 1) & 1],
 * per_call[call] and the workspace is written, and nothing outside the inputs is read, whatever the inputs hold; a non-finite
 * `reg_pois` row gives non-finite values in that record only.
 * Status: DCD_ERR_BAD_ARG, without a launch, for a null pointer, B < 1, M < 1, nk outside 2 .. 128, n_bins outside 1 .. 4,
 * cap < 1, call outside [0, n_calls) or a channel range outside [0, C); DCD_ERR_WORKSPACE for a workspace that is too small.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int B, M, C, nk, n_bins;
    /* first channel of 3d_offset (2), ori_cls (2 n_bins), ori_offset (2 n_bins), extra_kpts_2d (2 nk), extra_kpts_3d (3 nk) */
    int ch_offset, ch_ori_cls, ch_ori_off, ch_kpts2d, ch_kpts3d;
    float down_ratio;
} dcd_records_args;
size_t dcd_gmw_train_records_workspace_bytes(int B, int M, int nk);
int dcd_gmw_train_records(void *stream, const float *reg_pois, const dcd_records_args *args, const uint8_t *reg_mask,
                          const int32_t *target_centers, const float *offset_3D, const float *rotys, const float *locations,
                          const float *calib_P, const int64_t *pad_size, const float *calib, const int32_t *image_numbers, int cap,
                          float *kpts_2d, float *kpts_3d, float *pred_rot, float *gt_location, float *pred_location, int32_t *image,
                          int32_t *cursor, int32_t *per_call, int call, int n_calls, void *workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * The depth report (csrc/depth_report.hip, arithmetic in csrc/depth_report_math.h on top of csrc/decode_math.h): every depth
 * estimate the decode forms on its way to a row, for labelled objects, and the error of each against the label, booked by
 * class and range.
 *
 * dcd_depth_estimates: one launch, one workgroup per object slot, B * M slots (args->B images, args->K = M slots each; the
 * struct is the decode's, `uncertainty_as_conf` and `records` are not read).
 *   vectors      (B M, C) fp32: the regression heads at the objects' centre cells
 *   ys, xs, classes   (B M) fp32: the cell and the class, as dcd_decode_detections takes them
 *   gt_z         (B M) fp32: the label's depth;  valid (B M) u8: 0 = empty slot
 *   image_table  (B, 16) fp32 as for dcd_decode_detections; every object uses its own image's row
 *   est          (B M, 13): valid (1 or 0), class, gt_z, then the 10 methods
 *                  0 direct      the direct depth head             5 hard    the estimate with the smallest sigma
 *                  1 kpt_center  key-point depth, centre line      6 mean    plain mean of 0-3
 *                  2 kpt_02      key-point depth, corners 0/2      7 edges   mean over all nk (nk - 1) / 2 pairs minus P[2][3]:
 *                  3 kpt_13      key-point depth, corners 1/3                the z dcd_decode_detections reports, same bits
 *                  4 soft        inverse-sigma weighted mean       8 oracle  the one of 0-3 closest to gt_z, first on a tie
 *                                                                  9 gmw     NaN: the caller's column
 * An empty slot's row is thirteen zeros and its vector is never read.  A row depends on its own slot only; a non-finite vector
 * gives non-finite estimates in that row and touches no other (method 7 alone can stay finite: the edge solver's clamp drops a
 * NaN, as in the decode).  Fixed-order sums, no atomics: two calls give the same bits.
 * Status: DCD_ERR_BAD_ARG, without a launch, for a null pointer and for everything dcd_decode_detections refuses (M > 128,
 * nk > 128, head-axis orientation, ...).
 *
 * dcd_depth_accumulate: adds the rows of one batch to running tables in device memory, one launch.
 *   est          (n_slots, 13) as above, column 12 filled by the caller or left NaN
 *   edges        n_bins + 1 floats ON THE HOST, read during the call: an object falls in bin i when edges[i] <= gt_z < edges[i + 1]
 *   table        (num_classes, n_bins, 10, 5) fp64, zeroed by the caller before the first call: per cell the count of finite
 *                estimates, sum |e|, sum e, sum e^2 and the count of non-finite estimates, e = d - gt_z in double
 *   outside      (num_classes) i64: objects whose gt_z is below edges[0], at or above edges[n_bins], or not finite; they are
 *                booked nowhere else.  A row whose class is outside [0, num_classes) is booked nowhere at all.
 * One thread per cell walks the rows in slot order and adds its own to its five doubles: no floating-point atomics, no
 * reduction between threads.  A cell's sums are therefore the same sequence of additions whether a split arrives in one call or
 * in many, and two passes agree bit for bit.
 * Status: DCD_ERR_BAD_ARG, without a launch, for a null pointer, n_slots < 0, n_bins outside 1 .. 16, num_classes outside
 * 1 .. 8, or edges that are not finite and strictly increasing.  n_slots = 0 is DCD_OK and does nothing.
 * ---------------------------------------------------------------------------------------------- */
int dcd_depth_estimates(void *stream, const float *vectors, const float *ys, const float *xs, const float *classes,
                        const float *gt_z, const uint8_t *valid, const float *image_table, const dcd_decode_args *args, float *est);
int dcd_depth_accumulate(void *stream, const float *est, int n_slots, const float *edges, int n_bins, int num_classes,
                         double *table, int64_t *outside);

/* ------------------------------------------------------------------------------------------------
 * The disentangled IoU report (csrc/dis_iou.hip, arithmetic in csrc/dis_iou_math.h on top of csrc/decode_math.h,
 * csrc/depth_report_math.h and csrc/nms_math.h): at every labelled object, fifteen boxes in which ONE component is the
 * prediction's and the rest is the label's, and each box's BEV and 3-D overlap with the label -- which head loses the overlap.
 *
 * dcd_dis_iou_estimates: one launch, one workgroup per object slot, B * M slots (args as for dcd_depth_estimates).
 *   vectors, ys, xs, classes, valid, image_table   as for dcd_depth_estimates
 *   gt           (B M, 9) fp32: offset_3D (2), locations (3: the box CENTRE), dimensions (3: l h w), rotys (1)
 *   gmw_z        (B M) fp32: GMW's refined depth of the slot, or null (then NaN)
 *   dis          (B M, 33): valid (1 or 0), class, gt_z, bev[15], iou3d[15]
 *   boxes        (B M, 16, 7) or null: h w l x y z ry (y the bottom: columns 6:13 of a decoded row) of the label, then of the
 *                fifteen variants; null: not written
 * The variants, in the order of their columns (location | dimensions | yaw):
 *    0 full      the row dcd_decode_detections writes at that cell and class, same bits | predicted | predicted roty
 *    1 location  full's centre, the bottom from the label's h | label | label
 *    2 offset    the predicted projected-centre offset, back-projected at the label's z | label | label
 *    3 dims      the label's centre, the bottom from the predicted h | predicted | label
 *    4 orient    label | label | wrap(predicted alpha + atan2(label x, label z))
 *    5-14 depth:<m>, the ten methods of dcd_depth_estimates in their order (gmw from gmw_z): the LABEL's offset_3D
 *                back-projected at depth d[m] | label | label
 * The overlaps are the KITTI evaluator's (nms_math.h: nms_overlap_bev, nms_overlap_3d) with the label in the ground-truth box's
 * role.  When one of a variant's seven numbers is not finite, or an overlap comes out non-finite, both overlaps of that variant
 * are NaN; there is no other special case (a non-positive predicted dimension is booked as the evaluator's arithmetic makes it).
 * An empty slot's row (and boxes) are zeros and its vector is never read.  A row depends on its own slot only.  Fixed-order sums,
 * plain stores, no atomics: two calls give the same bits.
 * Status: DCD_ERR_BAD_ARG, without a launch, for a null pointer (gmw_z and boxes may be null) and for everything
 * dcd_decode_detections refuses.
 *
 * dcd_dis_iou_accumulate: adds the rows of one batch to running tables in device memory, one launch.
 *   dis          (n_slots, 33) as above
 *   edges        n_bins + 1 floats ON THE HOST, read during the call; the bin rule of dcd_depth_accumulate
 *   thresholds   (num_classes, 2, 2) doubles ON THE HOST, read during the call: per class and metric (bev, 3d) the strict and the
 *                loose overlap threshold, each in [0, 1]
 *   table        (num_classes, n_bins, 15, 2, 6) fp64, zeroed by the caller before the first call: per cell the count of finite
 *                overlaps, sum IoU, sum IoU^2, the overlaps > the strict threshold, those > the loose one (the evaluator's
 *                comparison), and the count of non-finite overlaps
 *   outside      (num_classes) i64, as for dcd_depth_accumulate
 * One thread per cell walks the rows in slot order: the tables have the same bits however a split is cut into calls.
 * Status: DCD_ERR_BAD_ARG, without a launch, for a null pointer, everything dcd_depth_accumulate refuses, and a threshold
 * outside [0, 1] or NaN.  n_slots = 0 is DCD_OK and does nothing.
 * ---------------------------------------------------------------------------------------------- */
int dcd_dis_iou_estimates(void *stream, const float *vectors, const float *ys, const float *xs, const float *classes,
                          const float *gt, const uint8_t *valid, const float *image_table, const float *gmw_z,
                          const dcd_decode_args *args, float *dis, float *boxes);
int dcd_dis_iou_accumulate(void *stream, const float *dis, int n_slots, const float *edges, int n_bins, int num_classes,
                           const double *thresholds, double *table, int64_t *outside);

/* ------------------------------------------------------------------------------------------------
 * Box NMS among the decoded candidates of every image of a batch, in ONE launch (csrc/nms.hip, arithmetic in csrc/nms_math.h):
 * TEST.USE_NMS.  The reference names the configuration keys and never reads them, so the rule is this library's:
 *   candidates  of image b: the prefix of its block of K rows whose raw score aux[., 0] is >= det_threshold (the raw scores
 *               leave the top-K descending, so this is every such row; a NaN ends the prefix, as the host's cut does; the
 *               comparison is float32 against det_threshold rounded to float32, as the host's is)
 *   order       descending FINAL score rows[., 13]; a tie goes to the lower rank; a NaN score is visited last
 *   rule        greedy: a candidate is suppressed when its overlap with an already KEPT candidate is > thresh; unless
 *               class_agnostic, only kept candidates of the same class count -- the integer part of rows[., 0], which is how the
 *               result writer names a row (the column carries the top-K's fraction).  A suppressed candidate suppresses nothing.
 *   overlap     KITTI's evaluator's (dcd_eval_overlaps), the kept box in the ground-truth box's role and the visited candidate
 *               in the detection's: DCD_NMS_2D image_box_overlap, criterion -1, float64, on rows[., 2:6]; DCD_NMS_BEV the clipped
 *               rotated area in float32 on (x, z, l, w, ry) over the union; DCD_NMS_3D that area times the height overlap from y
 *               and h over the volume union.  The comparison with thresh is made in float64.
 *   rows (B K, 14), aux (B K, 4), kpts2d (B K, nk, 2), kpts3d (B K, nk, 3): dcd_decode_detections' outputs; the key points may
 *               both be NULL (then so are their outputs, and nk is not read)
 *   rows_out, aux_out, kpts2d_out, kpts3d_out: the same shapes; per image block a permutation of the input rows, bit for bit:
 *               the survivors in their rank order, then the suppressed rows in rank order, then the rows below the threshold
 *               where they were.  The raw score aux_out[., 0] of every suppressed row is -inf, so the prefix `score >= threshold`
 *               of the output block is exactly the survivors.  Outputs must not alias inputs.
 *   overlaps_out (B, K, K) fp32 or NULL: element (i, j) of an image, i != j both candidates, = the overlap of candidates i and j
 *               (input ranks) the decision was taken from, with the one visited first in the kept box's role; symmetric;
 *               every other element 0.  With it every pair is evaluated; without it, class-aware, only pairs of one class.
 * One workgroup per image; no atomics, no workspace, nothing read back: two calls give the same bits.
 * Status: DCD_ERR_BAD_ARG, without a launch, for a null or aliased pointer, B < 1, K outside 1 .. 128, B K > 2^31 - 1, nk outside
 * 1 .. 128 when key points are given, only some of the four key-point pointers given, an unknown mode, thresh outside [0, 1)
 * or NaN, or a NaN det_threshold.
 * ---------------------------------------------------------------------------------------------- */
#define DCD_NMS_2D 1
#define DCD_NMS_BEV 2
#define DCD_NMS_3D 3
int dcd_nms_detections(void *stream, const float *rows, const float *aux, const float *kpts2d, const float *kpts3d, int B, int K,
                       int nk, int mode, double thresh, double det_threshold, int class_agnostic, float *rows_out, float *aux_out,
                       float *kpts2d_out, float *kpts3d_out, float *overlaps_out);

/* ------------------------------------------------------------------------------------------------
 * Mirrored-view test-time augmentation: the detections of a frame (view A) merged with those of the same frame mirrored and
 * decoded with the mirrored P (view M), for every image of a batch in ONE launch (csrc/tta.hip, arithmetic in csrc/tta_math.h;
 * the rule in full is DESIGN.md "Mirrored-view test-time augmentation").
 *   rows (2 B K, 14), aux (2 B K, 4), kpts2d (2 B K, nk, 2), kpts3d (2 B K, nk, 3): dcd_decode_detections' outputs for 2 B
 *               images: blocks 0 .. B - 1 are view A, block B + b is view M of image b.  The key points may both be NULL.
 *   widths (B,) int32: every image's OWN width in pixels (not the padded canvas): a row of M is un-mirrored with it, the
 *               inverse of `flip_sample`: x1' = (W - 1) - x2, x2' = (W - 1) - x1, x' = -x, ry' = (ry < 0 ? -pi - ry : pi - ry)
 *               wrapped into [-pi, pi], alpha' = wrap(ry' - atan2f(x', z)); float32.
 *   candidates  of view A: the prefix with raw score aux[., 0] >= det_threshold, as dcd_nms_detections counts it; they are
 *               visited in its order (descending final score, a tie to the lower rank, NaN last).  Eligible rows of view M: all
 *               K whose raw score is not NaN.
 *   matching    a candidate takes the still-unmatched eligible M row of the same integer class whose overlap with it (mode:
 *               DCD_NMS_2D / _BEV / _3D, dcd_nms_detections' own, the A row as the frame) is > match_thresh in float64 and, rounded
 *               to float32, the largest; a tie goes to the lower M rank.
 *   fusing      a matched pair gives one row by score and inverse-depth-error weights (tta_math.h, tta_fuse); an unmatched
 *               candidate has its final and raw score multiplied by unmatched_scale and keeps every other bit; a row of A below
 *               the cut is copied; an M row without a partner is dropped.  Every output row has an A member.
 *   rows_out (B K, 14), aux_out (B K, 4), kpts2d_out (B K, nk, 2), kpts3d_out (B K, nk, 3): per image the K rows re-ordered by
 *               output raw score, descending, stable on A's rank, NaN last, so `aux_out[., 0] >= det_threshold` is a prefix
 *               again; the key points are those of the row's A member.  Outputs must not alias inputs.
 *   src_out, mate_out (B K,) int32: the A rank an output row came from, and the M rank it was fused with or -1.
 *   overlaps_out (B, K, K) fp32 or NULL: element (a, m) = the overlap of A candidate a with the un-mirrored eligible M row m,
 *               every other element 0.  With it every such pair is evaluated; without it only pairs of one class.
 * One workgroup per image; no atomics, no workspace, nothing read back: two calls give the same bits.
 * Status: DCD_ERR_BAD_ARG, without a launch, for a null or aliased pointer, B < 1, K outside 1 .. 128, 2 B K > 2^31 - 1, nk
 * outside 1 .. 128 when key points are given, only some of the four key-point pointers given, an unknown mode, match_thresh
 * outside [0, 1) or NaN, unmatched_scale outside [0, 1] or NaN, or a NaN det_threshold.
 * ---------------------------------------------------------------------------------------------- */
int dcd_tta_merge_detections(void *stream, const float *rows, const float *aux, const float *kpts2d, const float *kpts3d,
                             const int *widths, int B, int K, int nk, int mode, double match_thresh, double det_threshold,
                             double unmatched_scale, float *rows_out, float *aux_out, float *kpts2d_out, float *kpts3d_out,
                             int *src_out, int *mate_out, float *overlaps_out);

/* ------------------------------------------------------------------------------------------------
 * The detections of a batch drawn on the device (csrc/render.hip; the raster rule is the header of csrc/render_math.h and
 * DESIGN.md 6d): per image the frame with the 2-D boxes, projected 3-D boxes, key points and labels, and beside it a square
 * bird's-eye panel, ground truth under detections, rank 0 on top.  Two launches: the primitive table, then the tiles.
 *   staged      the input pipeline's staged buffer (dcd_preprocess_images): (B, 5) int64 records -- byte offset, row pitch,
 *               height, width, flip -- then the packed uint8 RGB frames; 8-byte aligned, staged_bytes long.  A record that does
 *               not describe a frame inside the buffer and the canvas gives an all-zero picture, never a read outside.
 *               A set flip flag mirrors the frame, as the preprocessing did for the model.
 *   rows (B K, 14), aux (B K, 4), kpts2d (B K, nk, 2) or NULL with nk = 0: dcd_decode_detections' / dcd_nms_detections' outputs.
 *               A row is drawn iff aux[., 0] >= det_threshold and rows[., 13] > vis_threshold, both compared in float32.
 *   image_table (B, 16): the decode's; only P is read.
 *   gt_dims (B, M, 3) (l, h, w), gt_locs (B, M, 3) centres, gt_rotys (B, M), gt_mask (B, M) uint8: the targets' tables; all
 *               NULL with M = 0 for a split without labels.
 *   table (B, S, 12) int32, S = dcd_render_slots(M, K, nk); counts (B) int32; ends (B, S, 4) fp32 or NULL: outputs.  Entry =
 *               panel, kind (-1 none, 0 segment, 1 glyph), x0, y0, x1, y1, thickness, r, g, b, order, glyph; counts[b] = one past
 *               the last drawn entry; ends = the coordinates before truncation.  16-byte aligned table.
 *   canvas (B, in_h, in_w + in_h, 3) uint8, 4-byte aligned: every byte is written.
 * dcd_render_primitives is the second launch alone on a caller's table (B, stride, 12) and counts; an entry that is not a valid
 * primitive (unknown kind or panel, a coordinate of magnitude >= 2^24, thickness outside 1 .. 4, order outside [0, 2^18), glyph
 * outside 0 .. 14) is passed over, and counts are clamped to [0, stride].
 * No global atomics and no dependence on scheduling: two calls give the same bytes.
 * dcd_render_slots: S, or -1 when M, K (1 .. 128), nk (0 .. 128) are out of range or S exceeds 8192 entries.
 * Status: DCD_ERR_BAD_ARG, without a launch, for such a configuration, a null or misaligned pointer, B outside 1 .. 65535,
 * in_h / in_w outside 1 .. 16384, staged_bytes < 40 B, stride outside 1 .. 8192 or a NaN threshold.
 * ---------------------------------------------------------------------------------------------- */
int dcd_render_slots(int M, int K, int nk);
int dcd_render_detections(void *stream, const uint8_t *staged, size_t staged_bytes, const float *rows, const float *aux,
                          const float *kpts2d, const float *image_table, const float *gt_dims, const float *gt_locs,
                          const float *gt_rotys, const uint8_t *gt_mask, int B, int K, int nk, int M, int in_h, int in_w,
                          double det_threshold, double vis_threshold, int *table, int *counts, float *ends, uint8_t *canvas);
int dcd_render_primitives(void *stream, const uint8_t *staged, size_t staged_bytes, const int *table, const int *counts, int B,
                          int stride, int in_h, int in_w, uint8_t *canvas);

#ifdef __cplusplus
}
#endif
#endif /* DCD_HIP_H */
