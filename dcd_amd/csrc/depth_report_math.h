// Arithmetic of the depth report (include/dcd_hip.h, dcd_depth_estimates and dcd_depth_accumulate): every depth estimate of one
// labelled object, and the error statistics of one (class, range bin, method) cell.
//
// Written once for two compilations, as decode_math.h is: depth_report.hip runs it on the device and
// tests/host/host_depth_report.cpp runs the same functions in plain loops on the host.  The depths themselves are decode_math.h's
// (dd_head, dd_keypoint, dd_pair_partial, dd_edge_depth): nothing here restates a depth formula, only what is chosen among the
// four estimates and how an error is booked.
#pragma once
#include "decode_math.h"

#define DR_NM 10                  // methods, the order of dcd_depth_estimates' columns
#define DR_ROW (3 + DR_NM)        // floats per row of `est`: valid, class, gt_z, the methods
#define DR_STATS 5                // per cell: count, sum |e|, sum e, sum e^2, non-finite estimates
#define DR_MAX_BINS 16
#define DR_MAX_CLASSES 8

enum { DR_DIRECT = 0, DR_KPT_CENTER, DR_KPT_02, DR_KPT_13, DR_SOFT, DR_HARD, DR_MEAN, DR_EDGES, DR_ORACLE, DR_GMW };

DD_HD bool dr_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }      // false for a NaN and for +-inf

// Methods 0-6 and 8 from what dd_head leaves; d[DR_EDGES] and d[DR_GMW] are the caller's.
//   soft    the inverse-sigma weighted mean the decode locates the viewing ray with (h.fused_depth)
//   hard    the estimate whose sigma is smallest (h.best: the first maximum of 1 / sigma)
//   mean    ((d0 + d1) + d2 + d3) / 4 in float
//   oracle  the one of d0 .. d3 closest to gt_z, |d - gt_z| compared in double, the first on a tie; an estimate whose distance
//           is a NaN is never chosen, and d0 stands when all four are
DD_HD void dr_methods(const DdHead &h, const DdDepths &z, float gt_z, float *d)
{
    for (int i = 0; i < 4; ++i) d[i] = z.depth[i];
    d[DR_SOFT] = h.fused_depth;
    d[DR_HARD] = z.depth[h.best];
    d[DR_MEAN] = (((z.depth[0] + z.depth[1]) + z.depth[2]) + z.depth[3]) / 4.f;
    int pick = -1;
    double nearest = 0.0;
    for (int i = 0; i < 4; ++i) {
        const double e = fabs((double)z.depth[i] - (double)gt_z);
        if (e == e && (pick < 0 || e < nearest)) {
            pick = i;
            nearest = e;
        }
    }
    d[DR_ORACLE] = z.depth[pick < 0 ? 0 : pick];
}

// The range bin of an object: i with edges[i] <= gt_z < edges[i + 1]; -1 below, above or for a non-finite gt_z.
DD_HD int dr_bin(float gt_z, const float *edges, int n_bins)
{
    if (!dr_finite(gt_z)) return -1;
    for (int i = 0; i < n_bins; ++i)
        if (edges[i] <= gt_z && gt_z < edges[i + 1]) return i;
    return -1;
}

// The class of a row, or -1 for an empty slot and for a class outside [0, num_classes): such a row is booked nowhere.
DD_HD int dr_class(const float *row, int num_classes)
{
    if (row[0] == 0.f) return -1;
    const float c = row[1];
    return c >= 0.f && c < (float)num_classes ? (int)c : -1;
}

// One cell's share of a batch: the rows of class c whose gt_z lies in `bin`, in slot order, added to the five running sums in
// double.  e = d - gt_z is formed in double from the two floats; a non-finite estimate raises the fifth stat and nothing else.
DD_HD void dr_accumulate_cell(const float *est, int n_slots, const float *edges, int n_bins, int num_classes, int c, int bin, int m,
                              double *cell)
{
    double count = cell[0], abs_sum = cell[1], sum = cell[2], sq_sum = cell[3], bad = cell[4];
    for (int s = 0; s < n_slots; ++s) {
        const float *row = est + (size_t)s * DR_ROW;
        if (dr_class(row, num_classes) != c || dr_bin(row[2], edges, n_bins) != bin) continue;
        const float d = row[3 + m];
        if (!dr_finite(d)) {
            bad += 1.0;
            continue;
        }
        const double e = (double)d - (double)row[2];
        count += 1.0;
        abs_sum += fabs(e);
        sum += e;
        sq_sum += e * e;
    }
    cell[0] = count;
    cell[1] = abs_sum;
    cell[2] = sum;
    cell[3] = sq_sum;
    cell[4] = bad;
}

// The objects of class c that fall in no bin.
DD_HD int64_t dr_count_outside(const float *est, int n_slots, const float *edges, int n_bins, int num_classes, int c)
{
    int64_t n = 0;
    for (int s = 0; s < n_slots; ++s) {
        const float *row = est + (size_t)s * DR_ROW;
        if (dr_class(row, num_classes) == c && dr_bin(row[2], edges, n_bins) < 0) ++n;
    }
    return n;
}

// What dcd_depth_accumulate accepts (host code).
inline bool dr_tables_ok(int n_slots, const float *edges, int n_bins, int num_classes)
{
    if (n_slots < 0 || !edges || n_bins < 1 || n_bins > DR_MAX_BINS || num_classes < 1 || num_classes > DR_MAX_CLASSES) return false;
    for (int i = 0; i <= n_bins; ++i)
        if (!dr_finite(edges[i]) || (i > 0 && !(edges[i - 1] < edges[i]))) return false;
    return true;
}
