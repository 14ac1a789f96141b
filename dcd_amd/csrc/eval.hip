// eval.hip -- KITTI average precision on the device: box overlaps and the detection-to-ground-truth assignment.
//
// Replaces the two loops of the reference's evaluator that make it slow (DGDE/data/datasets/evaluation/
// kitti_object_eval_python): `calculate_iou_partly` (eval.py:338-412: `image_box_overlap`, `bev_box_overlap` = the numba.cuda
// kernel `rotate_iou_kernel_eval` of rotate_iou.py:264-296, `d3_box_overlap`) and `compute_statistics_jit` (eval.py:155-273) as
// `eval_class` calls it: once per image with compute_fp = False to collect the matched scores, then once per image and score
// threshold through `fused_compute_statistics` to count tp / fp / fn and the AOS similarity.
//
// All images of a split go through one launch as concatenated arrays with per-image offset tables; only an image's own
// detection x ground-truth block is computed (the reference pads to N x K per 100-image part).
//
// eval_overlaps: one thread per (detection, ground-truth) pair, image found by binary search in the pair-offset table.  The 2-D
// and 3-D arithmetic is float64 as in the reference.  The rotated intersection area is float32 on float32-rounded inputs, as
// in the reference (rotate_iou.py:314-315), and is computed once for the BEV and the 3-D metric -- but not by the reference's
// construction (corners inside the other box + the 16 edge-pair crossings, angular sort, triangle fan; rotate_iou.py:18-262).
// That construction decides "on the boundary" with rounded dot products, so it loses vertices when edges coincide: it returns
// area 0 for a box against ITSELF at yaw 0.3 and half the area at yaw -2.1 (evaluating a label set against itself is a common
// sanity check), and its 16-float vertex array overflows silently when rounding yields a ninth vertex.  Here the detection is
// moved into the ground-truth box's own frame (centre subtracted, relative yaw) and clipped against its four axis-aligned
// sides (Sutherland-Hodgman), then the shoelace sum: coincident boxes give exactly the full area, touching or distant boxes
// exactly 0, a ninth vertex is never written, and the corner coordinates are a few metres instead of up to 50.  Against the
// exact float64 area it is closer than the reference is (tests/test_gpu_eval.py holds it to 4x the reference's own error).
//
// eval_match: one wave per (image, combination); a combination is (class, difficulty, metric, overlap row).  Lanes own the
// image's detections in blocks of 64 (an `assigned` bit per block in a 64-bit lane mask: up to 4096 detections per image);
// ground-truth boxes are visited in order because the assignment is sequential in them.  Re-derived from the `elif` chain of
// eval.py:198-223, whose scan over the unassigned, un-thresholded candidates j with overlap > min_overlap and ignored_det != -1
// keeps:
//   compute_fp = False: the candidate of greatest score (strict `>`, so the lowest j among equals), provided score > -1e7;
//   compute_fp = True:  if any candidate has ignored_det == 0, the one of greatest overlap among THOSE (strict `>` against the
//                       running maximum, lowest j among equals; an ignored_det == 1 pick made earlier in the scan is always
//                       replaced because `assigned_ignored_det` waives the comparison, and none is made later because
//                       valid_detection is then set); otherwise the FIRST candidate with ignored_det == 1.
// so each ground-truth box costs one wave-wide arg-max (plus one wave-wide min for the fallback).  tp / fn and the similarity
// are wave-uniform values accumulated in ground-truth order; the similarity therefore has a fixed summation order inside an
// image, is written as a per-image partial and summed over images in image order by eval_sum_similarity: no floating-point
// atomics, bit-identical from run to run.  The integer counts are summed over images with global integer atomics.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/dcd_hip.h"
#include "nms_math.h"      // rbbox_to_corners, clipped_area: the one copy of the clip, shared with nms.hip

namespace {

constexpr int WAVE = 64;
constexpr int OVL_THREADS = 256;
constexpr int MAX_DT_BLOCKS = 64;               // bits of the per-lane `assigned` mask
constexpr double NO_DETECTION = -10000000.0;    // eval.py:182

// image of pair p: the last i with pair_off[i] <= p
__device__ inline int image_of_pair(const int64_t *__restrict__ pair_off, int n_img, int64_t p)
{
    int lo = 0, hi = n_img - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pair_off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(OVL_THREADS) void eval_overlaps(int n_img, const int32_t *__restrict__ gt_off,
                                                             const int32_t *__restrict__ dt_off, const int64_t *__restrict__ pair_off,
                                                             int G, int D, int64_t P, const double *__restrict__ gt_box2d,
                                                             const double *__restrict__ dt_box2d, const double *__restrict__ gt_box3d,
                                                             const double *__restrict__ dt_box3d, double *__restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * OVL_THREADS + threadIdx.x;
    if (p >= P) return;
    const int img = image_of_pair(pair_off, n_img, p);
    const int ng = gt_off[img + 1] - gt_off[img], nd = dt_off[img + 1] - dt_off[img];
    const int64_t local = p - pair_off[img];
    if (ng <= 0 || nd <= 0 || local < 0 || local >= (int64_t)nd * ng) return;    // inconsistent tables: write nothing
    const int d = dt_off[img] + (int)(local / ng), g = gt_off[img] + (int)(local % ng);   // the block is [dt, gt]
    if (d < 0 || d >= D || g < 0 || g >= G) return;

    // metric 0: image_box_overlap(boxes = dt, query_boxes = gt, criterion -1), eval.py:84-111
    const double *b = dt_box2d + 4 * (int64_t)d, *q = gt_box2d + 4 * (int64_t)g;
    double o2d = 0.0;
    const double iw = fmin(b[2], q[2]) - fmax(b[0], q[0]);
    if (iw > 0) {
        const double ih = fmin(b[3], q[3]) - fmax(b[1], q[1]);
        if (ih > 0) {
            const double qarea = (q[2] - q[0]) * (q[3] - q[1]);
            o2d = iw * ih / ((b[2] - b[0]) * (b[3] - b[1]) + qarea - iw * ih);
        }
    }
    out[p] = o2d;

    // metrics 1 and 2 share the BEV intersection: rbox1 = the ground truth (query), rbox2 = the detection (rotate_iou.py:295)
    const double *B = dt_box3d + 7 * (int64_t)d, *Q = gt_box3d + 7 * (int64_t)g;   // x y z l h w ry
    const float qx = (float)Q[0], qz = (float)Q[2], ql = (float)Q[3], qw = (float)Q[5], qr = (float)Q[6];
    const float bx = (float)B[0], bz = (float)B[2], bl = (float)B[3], bw = (float)B[5], br = (float)B[6];
    // the detection's corners in the ground-truth box's own frame (centre at the origin, sides along the axes):
    // R(qr)^T (R(br) p + cd - cg) = R(br - qr) p + R(qr)^T (cd - cg), with R(a) = [[cos a, sin a], [-sin a, cos a]]
    const float q_cos = cosf(qr), q_sin = sinf(qr), dx = bx - qx, dz = bz - qz;
    float cx[8], cz[8];
    rbbox_to_corners(cx, cz, q_cos * dx - q_sin * dz, q_sin * dx + q_cos * dz, bl, bw, cosf(br - qr), sinf(br - qr));
    const float inter = clipped_area(cx, cz, fabsf(ql) / 2, fabsf(qw) / 2);
    const double area1 = (double)ql * qw, area2 = (double)bl * bw;               // exact products of the float32 inputs
    out[P + p] = (double)inter / (area1 + area2 - (double)inter);

    // d3_box_overlap_kernel(boxes = dt, qboxes = gt), eval.py:119-145
    double o3d = (double)inter;
    if (o3d > 0) {
        const double ih = fmin(B[1], Q[1]) - fmax(B[1] - B[4], Q[1] - Q[4]);
        if (ih > 0) {
            const double v1 = B[3] * B[4] * B[5], v2 = Q[3] * Q[4] * Q[5], inc = ih * o3d;
            o3d = inc / (v1 + v2 - inc);
        } else {
            o3d = 0.0;
        }
    }
    out[2 * P + p] = o3d;
}

// ---- the assignment -------------------------------------------------------------------------------------------------
// greatest v (lowest idx among equals) over the wave; idx == INT_MAX marks "none"
__device__ inline void wave_argmax(double &v, int &idx)
{
#pragma unroll
    for (int s = WAVE / 2; s > 0; s >>= 1) {
        const double ov = __shfl_xor(v, s, WAVE);
        const int oi = __shfl_xor(idx, s, WAVE);
        if (oi != INT_MAX && (idx == INT_MAX || ov > v || (ov == v && oi < idx))) { v = ov; idx = oi; }
    }
}

__device__ inline int wave_min(int v)
{
#pragma unroll
    for (int s = WAVE / 2; s > 0; s >>= 1) v = min(v, __shfl_xor(v, s, WAVE));
    return v;
}

__device__ inline int wave_sum(int v)
{
#pragma unroll
    for (int s = WAVE / 2; s > 0; s >>= 1) v += __shfl_xor(v, s, WAVE);
    return v;
}

struct MatchImage {
    int g0, ng, d0, nd, c0, ndc, metric;
    int64_t p0;
    const int8_t *ign_gt, *ign_dt;      // this combination's flag rows, already offset to the image
    const double *ovl;                  // this metric's overlaps, already offset to the image: [dt, gt]
    double min_overlap;
};

// compute_statistics_jit for one image, by one wave.  FP = compute_fp.  `scores` (mode A) is the image's slice of the output.
template <bool FP>
__device__ void match_image(const dcd_eval_match_args &a, const MatchImage &im, double thresh, bool aos, int lane,
                            double *scores, int &tp_out, int &fp_out, int &fn_out, double &sim_out)
{
    uint64_t assigned = 0;              // bit k: detection lane + 64 k
    int tp = 0, fn = 0;
    double sim = 0.0;
    for (int i = 0; i < im.ng; ++i) {
        const int ig = im.ign_gt[i];
        if (ig == -1) {
            if (!FP && lane == 0) scores[i] = NO_DETECTION;
            continue;
        }
        double best = 0.0;
        int best_j = INT_MAX, first_ignored = INT_MAX;
        for (int k = 0, j = lane; j < im.nd; j += WAVE, ++k) {
            const int idt = im.ign_dt[j];
            if (idt == -1 || ((assigned >> k) & 1)) continue;
            const double score = a.dt_score[im.d0 + j];
            if (FP && score < thresh) continue;
            const double ov = im.ovl[(int64_t)j * im.ng + i];
            if (!(ov > im.min_overlap)) continue;
            if (!FP) {
                if (best_j == INT_MAX ? score > NO_DETECTION : score > best) { best = score; best_j = j; }
            } else if (idt == 0) {
                if (best_j == INT_MAX || ov > best) { best = ov; best_j = j; }
            } else if (first_ignored == INT_MAX) {
                first_ignored = j;
            }
        }
        wave_argmax(best, best_j);
        int det = best_j;
        if (FP && det == INT_MAX) det = wave_min(first_ignored);
        bool is_tp = false;
        if (det == INT_MAX) {
            if (ig == 0) ++fn;
        } else {
            if ((det & (WAVE - 1)) == lane) assigned |= (uint64_t)1 << (det / WAVE);
            if (!(ig == 1 || im.ign_dt[det] == 1)) {
                is_tp = true;
                ++tp;
                if (FP && aos) sim += (1.0 + cos(a.gt_alpha[im.g0 + i] - a.dt_alpha[im.d0 + det])) / 2.0;
            }
        }
        if (!FP && lane == 0) scores[i] = is_tp ? a.dt_score[im.d0 + det] : NO_DETECTION;
    }
    tp_out = tp; fn_out = fn; sim_out = sim;
    if (!FP) return;

    // false positives (eval.py:241-260): what is left unassigned among ignored_det == 0, minus those inside a DontCare box
    int fp = 0;
    for (int k = 0, j = lane; j < im.nd; j += WAVE, ++k) {
        if (im.ign_dt[j] != 0 || ((assigned >> k) & 1) || a.dt_score[im.d0 + j] < thresh) continue;
        ++fp;
        if (im.metric != 0) continue;
        const double *b = a.dt_box2d + 4 * (int64_t)(im.d0 + j);
        const double area = (b[2] - b[0]) * (b[3] - b[1]);
        for (int c = 0; c < im.ndc; ++c) {                           // image_box_overlap(dt, dc, criterion 0)
            const double *q = a.dc_box + 4 * (int64_t)(im.c0 + c);
            const double iw = fmin(b[2], q[2]) - fmax(b[0], q[0]);
            if (!(iw > 0)) continue;
            const double ih = fmin(b[3], q[3]) - fmax(b[1], q[1]);
            if (ih > 0 && iw * ih / area > im.min_overlap) { --fp; break; }
        }
    }
    fp_out = wave_sum(fp);
}

template <bool FP>
__global__ __launch_bounds__(WAVE) void eval_match(dcd_eval_match_args a)
{
    const int img = blockIdx.x, comb = blockIdx.y, lane = threadIdx.x;
    const int metric = a.comb[3 * comb], row = a.comb[3 * comb + 1], slot = a.comb[3 * comb + 2];
    MatchImage im;
    im.g0 = a.gt_off[img]; im.ng = a.gt_off[img + 1] - im.g0;
    im.d0 = a.dt_off[img]; im.nd = a.dt_off[img + 1] - im.d0;
    im.c0 = a.dc_off[img]; im.ndc = a.dc_off[img + 1] - im.c0;
    im.p0 = a.pair_off[img];
    im.metric = metric;
    // tables that do not fit the declared sizes: this wave does nothing
    if (metric < 0 || metric > 2 || row < 0 || row >= a.n_rows || (FP && slot >= a.n_slots)) return;   // mode A has no slots
    if (im.ng < 0 || im.nd < 0 || im.ndc < 0 || im.g0 < 0 || im.d0 < 0 || im.c0 < 0 || im.p0 < 0) return;
    if (im.g0 + im.ng > a.G || im.d0 + im.nd > a.D || im.c0 + im.ndc > a.n_dc || im.nd > WAVE * MAX_DT_BLOCKS) return;
    if (im.p0 + (int64_t)im.nd * im.ng > a.P) return;
    im.ign_gt = a.ign_gt + (int64_t)row * a.G + im.g0;
    im.ign_dt = a.ign_dt + (int64_t)row * a.D + im.d0;
    im.ovl = a.overlaps + (int64_t)metric * a.P + im.p0;
    im.min_overlap = a.min_overlap[comb];

    int tp = 0, fp = 0, fn = 0;
    double sim = 0.0;
    if constexpr (!FP) {
        match_image<false>(a, im, 0.0, false, lane, a.scores + (int64_t)comb * a.G + im.g0, tp, fp, fn, sim);
    } else {
        const int nt = min(max(a.n_thresh[comb], 0), a.T);
        const bool aos = slot >= 0;
        for (int t = 0; t < a.T; ++t) {
            sim = 0.0;
            if (t < nt) {
                match_image<true>(a, im, a.thresholds[(int64_t)comb * a.T + t], aos, lane, nullptr, tp, fp, fn, sim);
                if (lane == 0) {
                    int32_t *c = a.counts + 3 * ((int64_t)comb * a.T + t);
                    if (tp) atomicAdd(c, tp);
                    if (fp) atomicAdd(c + 1, fp);
                    if (fn) atomicAdd(c + 2, fn);
                }
            }
            if (aos && lane == 0) a.sim_part[((int64_t)img * a.n_slots + slot) * a.T + t] = sim;   // zero past the last threshold
        }
    }
}

// out[k] = sum over images, in image order, of part[i][k]
__global__ __launch_bounds__(OVL_THREADS) void eval_sum_similarity(const double *__restrict__ part, int n_img, int n, double *__restrict__ out)
{
    const int k = blockIdx.x * OVL_THREADS + threadIdx.x;
    if (k >= n) return;
    double s = 0.0;
    for (int i = 0; i < n_img; ++i) s += part[(int64_t)i * n + k];
    out[k] = s;
}

}  // namespace

extern "C" {

int dcd_eval_overlaps(void *stream_, int n_img, const int32_t *gt_off, const int32_t *dt_off, const int64_t *pair_off, int G, int D,
                      int64_t P, const double *gt_box2d, const double *dt_box2d, const double *gt_box3d, const double *dt_box3d,
                      double *out)
{
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (n_img <= 0 || G < 0 || D < 0 || P < 0 || P > (int64_t)G * D || !gt_off || !dt_off || !pair_off) return DCD_ERR_BAD_ARG;
    if (P == 0) return DCD_OK;                                        // no image has both kinds of box: nothing to write
    if (!gt_box2d || !dt_box2d || !gt_box3d || !dt_box3d || !out) return DCD_ERR_BAD_ARG;
    const int64_t blocks = (P + OVL_THREADS - 1) / OVL_THREADS;
    if (blocks > INT_MAX) return DCD_ERR_BAD_ARG;
    hipLaunchKernelGGL(eval_overlaps, dim3((unsigned)blocks), dim3(OVL_THREADS), 0, stream, n_img, gt_off, dt_off, pair_off, G, D, P,
                       gt_box2d, dt_box2d, gt_box3d, dt_box3d, out);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}

int dcd_eval_match(void *stream_, const dcd_eval_match_args *a)
{
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (!a || (a->mode != DCD_EVAL_MATCH_SCORES && a->mode != DCD_EVAL_MATCH_COUNTS)) return DCD_ERR_BAD_ARG;
    if (a->n_img <= 0 || a->n_comb <= 0 || a->n_comb > 65535 || a->n_rows <= 0 || a->G < 0 || a->D < 0 || a->n_dc < 0 || a->P < 0)
        return DCD_ERR_BAD_ARG;
    if (a->max_dt < 0 || a->max_dt > WAVE * MAX_DT_BLOCKS) return DCD_ERR_BAD_ARG;
    if (!a->gt_off || !a->dt_off || !a->dc_off || !a->pair_off || !a->comb || !a->min_overlap) return DCD_ERR_BAD_ARG;
    if ((a->P && !a->overlaps) || (a->G && (!a->ign_gt || !a->gt_alpha)) || (a->n_dc && !a->dc_box) ||
        (a->D && (!a->ign_dt || !a->dt_score || !a->dt_alpha || !a->dt_box2d)))
        return DCD_ERR_BAD_ARG;
    const dim3 grid(a->n_img, a->n_comb);
    if (a->mode == DCD_EVAL_MATCH_SCORES) {
        if (a->G == 0) return DCD_OK;
        if (!a->scores) return DCD_ERR_BAD_ARG;
        hipLaunchKernelGGL(eval_match<false>, grid, dim3(WAVE), 0, stream, *a);
    } else {
        if (a->T <= 0 || a->T > DCD_EVAL_MAX_THRESHOLDS || a->n_slots < 0 || !a->thresholds || !a->n_thresh || !a->counts ||
            (a->n_slots && !a->sim_part))
            return DCD_ERR_BAD_ARG;
        hipLaunchKernelGGL(eval_match<true>, grid, dim3(WAVE), 0, stream, *a);
    }
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}

int dcd_eval_sum_similarity(void *stream_, const double *part, int n_img, int n, double *out)
{
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (n_img <= 0 || n < 0) return DCD_ERR_BAD_ARG;
    if (n == 0) return DCD_OK;
    if (!part || !out) return DCD_ERR_BAD_ARG;
    hipLaunchKernelGGL(eval_sum_similarity, dim3((n + OVL_THREADS - 1) / OVL_THREADS), dim3(OVL_THREADS), 0, stream, part, n_img, n, out);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}

}  // extern "C"
