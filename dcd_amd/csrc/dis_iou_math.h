// Arithmetic of the disentangled IoU report (include/dcd_hip.h, dcd_dis_iou_estimates and dcd_dis_iou_accumulate): at one
// labelled object, the fifteen boxes in which one component is the prediction's and the rest is the label's, each box's BEV and
// 3-D overlap with the label, and the statistics of one (class, range bin, variant, metric) cell.
//
// Written once for two compilations, as its siblings are: dis_iou.hip runs it on the device and tests/host/host_dis_iou.cpp runs
// the same functions in plain loops on the host.  Nothing here restates a formula: the heads are decode_math.h's (dd_head,
// dd_location, dd_wrap, dd_edge_depth), the ten depths depth_report_math.h's (dr_methods), the clip and the two overlaps
// nms_math.h's, which are the KITTI evaluator's.  This header only says which component of which box comes from where.
//
// nms_math.h is included FIRST: it sets no contraction mode and must be compiled here under the one it is compiled under in
// eval.hip and nms.hip, while decode_math.h turns contraction off from its own first line to the end of the translation unit.
// This header sets none of its own.
#pragma once
#include "nms_math.h"
#include "depth_report_math.h"

#define DIS_NV 15                       // variants: full, location, offset, dims, orient, depth:<the ten methods>
#define DIS_NMETRIC 2                   // bev, 3d
#define DIS_ROW (3 + 2 * DIS_NV)        // floats per row of `dis`: valid, class, gt_z, bev[15], iou3d[15]
#define DIS_STATS 6                     // per cell: count, sum IoU, sum IoU^2, hits strict, hits loose, non-finite
#define DIS_GT 9                        // floats per label: offset_3D (2), locations (3, the centre), dimensions (3: l h w), rotys
#define DIS_BOX 7                       // h w l x y z ry: columns 6:13 of a decoded row, y the BOTTOM of the box
#define DIS_NBOX (1 + DIS_NV)           // boxes per slot of the optional output: the label's, then the variants'

enum { DIS_FULL = 0, DIS_LOCATION, DIS_OFFSET, DIS_DIMS, DIS_ORIENT, DIS_DEPTH0 };

// The label as the (14,) row the overlaps read (nms_math.h: 6:9 h w l, 9:12 x y z with y the bottom, 12 ry); the rest is zero.
DD_HD void dis_label_row(const float *gt, float *q)
{
    for (int i = 0; i < NMS_ROW; ++i) q[i] = 0.f;
    q[6] = gt[6];
    q[7] = gt[7];
    q[8] = gt[5];
    q[9] = gt[2];
    q[10] = gt[3] + gt[6] / 2.f;
    q[11] = gt[4];
    q[12] = gt[8];
}

// Variant v's seven box numbers.  h, z: what dd_head left of the slot's vector; pair_sum: the tree's sum of the lanes' pair
// partials; gmw_z: GMW's depth of the slot (NaN when the caller has none).
//   full      the row dd_finish writes: dd_location at the edge depth, y + predicted h / 2, predicted dimensions, h.roty
//   location  full's centre, the bottom from the label's h; label dimensions and yaw
//   offset    dd_location with the predicted offset at the LABEL's z
//   dims      the label's centre, the bottom from the predicted h; predicted dimensions
//   orient    the label's box with yaw = wrap(alpha + the label's viewing ray)
//   depth:m   dd_location with the LABEL's offset_3D at depth d[m]
DD_HD void dis_variant_box(const dcd_decode_args &a, const DdHead &h, const DdDepths &z, const float *tab, float pair_sum,
                           const float *gt, float gmw_z, int v, float *box)
{
    const float gl = gt[5], gh = gt[6], gw = gt[7], gry = gt[8];
    float loc[3];
    box[0] = gh;
    box[1] = gw;
    box[2] = gl;
    box[3] = gt[2];
    box[4] = gt[3] + gh / 2.f;
    box[5] = gt[4];
    box[6] = gry;
    if (v == DIS_FULL || v == DIS_LOCATION) {
        dd_location(a, h, tab, dd_edge_depth(a, pair_sum), loc);
        const bool full = v == DIS_FULL;
        if (full) {
            box[0] = h.dims[1];
            box[1] = h.dims[2];
            box[2] = h.dims[0];
            box[6] = h.roty;
        }
        box[3] = loc[0];
        box[4] = loc[1] + (full ? h.dims[1] : gh) / 2.f;
        box[5] = loc[2];
    } else if (v == DIS_OFFSET) {
        dd_location(a, h, tab, gt[4], loc);
        box[3] = loc[0];
        box[4] = loc[1] + gh / 2.f;
        box[5] = loc[2];
    } else if (v == DIS_DIMS) {
        box[0] = h.dims[1];
        box[1] = h.dims[2];
        box[2] = h.dims[0];
        box[4] = gt[3] + h.dims[1] / 2.f;
    } else if (v == DIS_ORIENT) {
        box[6] = dd_wrap(h.alpha + atan2f(gt[2], gt[4]));
    } else {
        float d[DR_NM];
        dr_methods(h, z, gt[4], d);
        d[DR_EDGES] = dd_edge_depth(a, pair_sum);
        d[DR_GMW] = gmw_z;
        DdHead g = h;
        g.off_x = gt[0];
        g.off_y = gt[1];
        dd_location(a, g, tab, d[v - DIS_DEPTH0], loc);
        box[3] = loc[0];
        box[4] = loc[1] + gh / 2.f;
        box[5] = loc[2];
    }
}

// The two overlaps of a variant's box with the label's row q, the label in the ground-truth box's role.  Both are NaN when one of
// the seven numbers is not finite, and when an overlap comes out non-finite; there is no other special case.
DD_HD void dis_overlaps(const float *q, const float *box, float *bev, float *iou3d)
{
    const float nan = NAN;
    *bev = nan;
    *iou3d = nan;
    for (int i = 0; i < DIS_BOX; ++i)
        if (!dr_finite(box[i])) return;
    float b[NMS_ROW];
    for (int i = 0; i < 6; ++i) b[i] = 0.f;
    for (int i = 0; i < DIS_BOX; ++i) b[6 + i] = box[i];
    b[13] = 0.f;
    const float o2 = (float)nms_overlap_bev(q, b), o3 = (float)nms_overlap_3d(q, b);
    if (!dr_finite(o2) || !dr_finite(o3)) return;
    *bev = o2;
    *iou3d = o3;
}

// One cell's share of a batch: the rows of class c whose gt_z lies in `bin`, in slot order.  A hit is IoU > threshold, the
// evaluator's comparison (the float32 overlap against the double threshold); a non-finite IoU raises the sixth stat and nothing
// else.
DD_HD void dis_accumulate_cell(const float *dis, int n_slots, const float *edges, int n_bins, int num_classes, int c, int bin, int v,
                               int metric, double strict, double loose, double *cell)
{
    double count = cell[0], sum = cell[1], sq_sum = cell[2], hit_s = cell[3], hit_l = cell[4], bad = cell[5];
    for (int s = 0; s < n_slots; ++s) {
        const float *row = dis + (size_t)s * DIS_ROW;
        if (dr_class(row, num_classes) != c || dr_bin(row[2], edges, n_bins) != bin) continue;
        const float iou = row[3 + metric * DIS_NV + v];
        if (!dr_finite(iou)) {
            bad += 1.0;
            continue;
        }
        const double o = (double)iou;
        count += 1.0;
        sum += o;
        sq_sum += o * o;
        if (o > strict) hit_s += 1.0;
        if (o > loose) hit_l += 1.0;
    }
    cell[0] = count;
    cell[1] = sum;
    cell[2] = sq_sum;
    cell[3] = hit_s;
    cell[4] = hit_l;
    cell[5] = bad;
}

// The objects of class c that fall in no bin (the first three columns of a `dis` row are those of an `est` row).
DD_HD int64_t dis_count_outside(const float *dis, int n_slots, const float *edges, int n_bins, int num_classes, int c)
{
    int64_t n = 0;
    for (int s = 0; s < n_slots; ++s) {
        const float *row = dis + (size_t)s * DIS_ROW;
        if (dr_class(row, num_classes) == c && dr_bin(row[2], edges, n_bins) < 0) ++n;
    }
    return n;
}

// What dcd_dis_iou_accumulate accepts (host code): dr_tables_ok, and num_classes x 2 metrics x 2 thresholds in [0, 1].
inline bool dis_tables_ok(int n_slots, const float *edges, int n_bins, int num_classes, const double *thresholds)
{
    if (!thresholds || !dr_tables_ok(n_slots, edges, n_bins, num_classes)) return false;
    for (int i = 0; i < num_classes * DIS_NMETRIC * 2; ++i)
        if (!(thresholds[i] >= 0.0 && thresholds[i] <= 1.0)) return false;
    return true;
}
