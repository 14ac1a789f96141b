// Arithmetic of the box NMS on decoded detections (include/dcd_hip.h, dcd_nms_detections), and the rotated-rectangle clip it
// shares with KITTI's evaluator (eval.hip).
//
// Written once for two compilations, in the way of decode_math.h and records_math.h: nms.hip runs it with one workgroup per
// image, tests/host/host_nms.cpp runs the same functions in plain loops on the host, so that the decisions can be held against
// a float64 restatement without a GPU.  The host build is test infrastructure; the library has no host path.
//
// The overlaps are the evaluator's own (eval.hip, eval_overlaps), on the (14,) rows of `write_detections`
//   0 class | 1 alpha | 2:6 box x1 y1 x2 y2 | 6:9 h w l | 9:12 x y z | 12 ry | 13 score
// with the KEPT (higher-score) box in the ground-truth box's role -- the frame the other is clipped in -- and the visited
// candidate in the detection's:
//   2d    image_box_overlap, criterion -1, float64
//   bev   the clipped rotated area in float32 on (x, z, l, w, ry), over the union in float64
//   3d    that area times the height overlap from y and h, over the volume union, float64
// This header sets no floating-point contraction mode: eval.hip includes it and must keep the bits it had when the clip lived
// there.  The host build turns contraction off on its command line.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dcd_hip.h"

#ifdef __HIPCC__
#define NM_HD __host__ __device__ inline
#else
#define NM_HD inline
#endif

#define NMS_MAXK 128                    // candidates per image: the fused decode's limit
#define NMS_WORDS (NMS_MAXK / 32)       // 32-bit words of one row of the suppression matrix
#define NMS_ROW 14
#define NMS_AUX 4

// ---- rotated rectangles, float32 -------------------------------------------------------------------------------------
// Corners of a rectangle in the reference's order and rotation sense (rbbox_to_corners, rotate_iou.py:207-230).
NM_HD void rbbox_to_corners(float *x, float *y, float cx, float cy, float xd, float yd, float a_cos, float a_sin)
{
    const float px[4] = {-xd / 2, -xd / 2, xd / 2, xd / 2}, py[4] = {-yd / 2, yd / 2, yd / 2, -yd / 2};
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) {
        x[i] = a_cos * px[i] + a_sin * py[i] + cx;
        y[i] = -a_sin * px[i] + a_cos * py[i] + cy;
    }
}

// Area of the quadrilateral (x, y)[0..3] inside the axis-aligned rectangle |x| <= hx, |y| <= hy: Sutherland-Hodgman against
// the four sides, then the shoelace sum.  A convex polygon gains at most one vertex per side, so 8 slots hold it; the guard
// keeps a ninth from ever being written whatever rounding does.  Points on a side count as inside, and a crossing is put
// exactly on the side, so boxes that touch give a degenerate polygon of area exactly 0 and coincident boxes the full area.
NM_HD float clipped_area(float *x, float *y, float hx, float hy)
{
    float ox[8], oy[8];
    int n = 4;
    for (int side = 0; side < 4; ++side) {
        const bool along_x = side < 2;
        const float sgn = (side & 1) ? -1.f : 1.f, lim = along_x ? hx : hy;       // inside: sgn * coordinate <= lim
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const int k = i + 1 == n ? 0 : i + 1;
            const float pi = sgn * (along_x ? x[i] : y[i]), pk = sgn * (along_x ? x[k] : y[k]);
            const bool in_i = pi <= lim, in_k = pk <= lim;
            if (in_i && m < 8) { ox[m] = x[i]; oy[m] = y[i]; ++m; }
            if (in_i != in_k && m < 8) {
                const float t = (lim - pi) / (pk - pi);
                ox[m] = along_x ? sgn * lim : x[i] + t * (x[k] - x[i]);
                oy[m] = along_x ? y[i] + t * (y[k] - y[i]) : sgn * lim;
                ++m;
            }
        }
        n = m;
        if (n < 3) return 0.f;
        for (int i = 0; i < n; ++i) { x[i] = ox[i]; y[i] = oy[i]; }
    }
    float twice = 0.f;
    for (int i = 0; i < n; ++i) {
        const int k = i + 1 == n ? 0 : i + 1;
        twice += x[i] * y[k] - x[k] * y[i];
    }
    return fabsf(twice) / 2.0f;
}

// ---- the three overlaps of two rows: q = the kept box (the frame), b = the visited candidate --------------------------
// image_box_overlap(boxes = b, query_boxes = q, criterion -1), eval.py:84-111
NM_HD double nms_overlap_2d(const float *q, const float *b)
{
    const double b0 = b[2], b1 = b[3], b2 = b[4], b3 = b[5], q0 = q[2], q1 = q[3], q2 = q[4], q3 = q[5];
    const double iw = fmin(b2, q2) - fmax(b0, q0);
    if (!(iw > 0)) return 0.0;
    const double ih = fmin(b3, q3) - fmax(b1, q1);
    if (!(ih > 0)) return 0.0;
    const double qarea = (q2 - q0) * (q3 - q1);
    return iw * ih / ((b2 - b0) * (b3 - b1) + qarea - iw * ih);
}

// the BEV intersection area: b moved into q's own frame and clipped against q's four sides, as eval_overlaps does it
NM_HD float nms_bev_intersection(const float *q, const float *b)
{
    const float qx = q[9], qz = q[11], ql = q[8], qw = q[7], qr = q[12];
    const float bx = b[9], bz = b[11], bl = b[8], bw = b[7], br = b[12];
    const float q_cos = cosf(qr), q_sin = sinf(qr), dx = bx - qx, dz = bz - qz;
    float cx[8], cz[8];
    rbbox_to_corners(cx, cz, q_cos * dx - q_sin * dz, q_sin * dx + q_cos * dz, bl, bw, cosf(br - qr), sinf(br - qr));
    return clipped_area(cx, cz, fabsf(ql) / 2, fabsf(qw) / 2);
}

NM_HD double nms_overlap_bev(const float *q, const float *b)
{
    const double inter = (double)nms_bev_intersection(q, b);
    const double area1 = (double)q[8] * q[7], area2 = (double)b[8] * b[7];         // exact products of the float32 inputs
    return inter / (area1 + area2 - inter);
}

// d3_box_overlap_kernel(boxes = b, qboxes = q), eval.py:119-145
NM_HD double nms_overlap_3d(const float *q, const float *b)
{
    const double inter = (double)nms_bev_intersection(q, b);
    if (!(inter > 0)) return inter;
    const double by = b[10], bh = b[6], qy = q[10], qh = q[6];
    const double ih = fmin(by, qy) - fmax(by - bh, qy - qh);
    if (!(ih > 0)) return 0.0;
    const double v1 = (double)b[8] * bh * (double)b[7], v2 = (double)q[8] * qh * (double)q[7], inc = ih * inter;
    return inc / (v1 + v2 - inc);
}

NM_HD double nms_overlap(int mode, const float *q, const float *b)
{
    return mode == DCD_NMS_2D ? nms_overlap_2d(q, b) : mode == DCD_NMS_BEV ? nms_overlap_bev(q, b) : nms_overlap_3d(q, b);
}

// ---- order and the greedy rule --------------------------------------------------------------------------------------
// an image's candidates are the prefix of its block whose raw score is >= the threshold (a NaN ends it, as `keep_prefix`).
// The comparison is float32 against the threshold rounded to float32: what numpy makes of `float32 array >= python float` in
// `keep_prefix` and torch of `scores >= threshold` in the op-by-op decode, so the kernel and the host cut at the same row.
NM_HD bool nms_is_candidate(float raw, double det_threshold) { return raw >= (float)det_threshold; }

// is candidate j (final score sj) visited before candidate t (final score st)?  Descending score, a tie to the lower rank,
// a NaN after every number.
NM_HD bool nms_before(float sj, int j, float st, int t)
{
    const bool nan_j = sj != sj, nan_t = st != st;
    if (nan_j) return nan_t && j < t;
    if (nan_t) return true;
    return sj > st || (sj == st && j < t);
}

// A row's class is the integer part of column 0, as `write_detections` names it: the top-K hands the class over as
// index / (H W) in floating point, so the column carries a fraction (the reference's quirk, kept by the decode).  NaN: no class.
NM_HD bool nms_same_class(const float *q, const float *b) { return truncf(q[0]) == truncf(b[0]); }

// does the kept box q take the candidate b out?  (class-aware: only a kept box of the same class counts)
NM_HD bool nms_suppresses(double overlap, double thresh, bool class_agnostic, const float *q, const float *b)
{
    return (class_agnostic || nms_same_class(q, b)) && overlap > thresh;
}

// bits: n rows of NMS_WORDS words in VISIT order, bit c of row r (c > r only) = "r, if kept, suppresses c".  removed
// (NMS_WORDS words) receives the suppressed set: a suppressed candidate's row is never applied, so it suppresses nothing.
NM_HD void nms_greedy(const uint32_t *bits, int n, uint32_t *removed)
{
    for (int w = 0; w < NMS_WORDS; ++w) removed[w] = 0;
    for (int r = 0; r < n; ++r) {
        const uint32_t live = ((removed[r >> 5] >> (r & 31)) & 1u) ? 0u : ~0u;
        for (int w = 0; w < NMS_WORDS; ++w) removed[w] |= bits[r * NMS_WORDS + w] & live;
    }
}

NM_HD bool nms_bit(const uint32_t *words, int i) { return (words[i >> 5] >> (i & 31)) & 1u; }
