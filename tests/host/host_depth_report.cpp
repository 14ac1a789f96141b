// Host instantiation of csrc/depth_report_math.h: the two kernels of csrc/depth_report.hip in plain loops (a "lane" and a
// "thread" are loop indices, the tree over the lanes' partial sums runs in the kernel's order), so that
// tests/test_depth_report_host.py can hold the estimates against the op-by-op chain and the tables against a numpy restatement on
// a machine without a GPU.  Test infrastructure only -- nothing under dcd_amd/ links or loads this.
#include <math.h>

#include "../../dcd_amd/csrc/depth_report_math.h"

extern "C" int host_depth_estimates(const float *vectors, const float *ys, const float *xs, const float *classes, const float *gt_z,
                                    const uint8_t *valid, const float *table, const dcd_decode_args *args, float *est)
{
    if (!args || !dd_args_ok(*args)) return DCD_ERR_BAD_ARG;
    const dcd_decode_args a = *args;
    const int nk = a.nk;
    for (int n = 0; n < a.B * a.K; ++n) {
        float *row = est + (size_t)n * DR_ROW;
        if (!valid[n]) {
            for (int i = 0; i < DR_ROW; ++i) row[i] = 0.f;
            continue;
        }
        const float *vec = vectors + (size_t)n * a.C;
        const float *tab = table + (size_t)(n / a.K) * DD_TABLE;
        DdDepths z;
        const DdHead h = dd_head(a, vec, 0.f, classes[n], ys[n], xs[n], tab, &z);
        const float sn = sinf(h.roty), cs = cosf(h.roty);
        float vn[DD_LANES], Y[DD_LANES], vC[DD_LANES], part[DD_LANES];
        for (int k = 0; k < nk; ++k) {
            const DdKeypoint p = dd_keypoint(a, vec, h, tab, k, sn, cs);
            vn[k] = p.vn;
            Y[k] = p.Y;
            vC[k] = p.vC;
        }
        for (int t = 0; t < DD_LANES; ++t) part[t] = dd_pair_partial(t, nk, vn, Y, vC, tab[4 + 11]);
        for (int s = DD_LANES / 2; s > 0; s >>= 1)
            for (int t = 0; t < s; ++t) part[t] = DD_ADD(part[t], part[t + s]);
        float d[DR_NM];
        dr_methods(h, z, gt_z[n], d);
        d[DR_EDGES] = dd_edge_depth(a, part[0]);
        d[DR_GMW] = NAN;
        row[0] = 1.f;
        row[1] = classes[n];
        row[2] = gt_z[n];
        for (int m = 0; m < DR_NM; ++m) row[3 + m] = d[m];
    }
    return DCD_OK;
}

extern "C" int host_depth_accumulate(const float *est, int n_slots, const float *edges, int n_bins, int num_classes, double *table,
                                     int64_t *outside)
{
    if (!est || !table || !outside || !dr_tables_ok(n_slots, edges, n_bins, num_classes)) return DCD_ERR_BAD_ARG;
    const int cells = num_classes * n_bins * DR_NM;
    for (int t = 0; t < cells; ++t) {
        const int m = t % DR_NM, bin = (t / DR_NM) % n_bins, c = t / (DR_NM * n_bins);
        dr_accumulate_cell(est, n_slots, edges, n_bins, num_classes, c, bin, m, table + (size_t)t * DR_STATS);
    }
    for (int c = 0; c < num_classes; ++c) outside[c] += dr_count_outside(est, n_slots, edges, n_bins, num_classes, c);
    return DCD_OK;
}
