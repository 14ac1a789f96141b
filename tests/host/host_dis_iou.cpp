// Host instantiation of csrc/dis_iou_math.h: the two kernels of csrc/dis_iou.hip in plain loops (a "lane" and a "thread" are loop
// indices, the tree over the lanes' partial sums runs in the kernel's order), so that tests/test_dis_iou_host.py can hold the
// boxes, the overlaps and the tables against a float64 restatement on a machine without a GPU.  Test infrastructure only --
// nothing under dcd_amd/ links or loads this.
#include <math.h>

#include "../../dcd_amd/csrc/dis_iou_math.h"

extern "C" int host_dis_iou_estimates(const float *vectors, const float *ys, const float *xs, const float *classes, const float *gt,
                                      const uint8_t *valid, const float *table, const float *gmw_z, const dcd_decode_args *args,
                                      float *dis, float *boxes)
{
    if (!args || !vectors || !ys || !xs || !classes || !gt || !valid || !table || !dis || !dd_args_ok(*args)) return DCD_ERR_BAD_ARG;
    const dcd_decode_args a = *args;
    const int nk = a.nk;
    for (int n = 0; n < a.B * a.K; ++n) {
        float *row = dis + (size_t)n * DIS_ROW;
        float *out_boxes = boxes ? boxes + (size_t)n * DIS_NBOX * DIS_BOX : nullptr;
        if (!valid[n]) {
            for (int i = 0; i < DIS_ROW; ++i) row[i] = 0.f;
            if (out_boxes)
                for (int i = 0; i < DIS_NBOX * DIS_BOX; ++i) out_boxes[i] = 0.f;
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
        const float *label = gt + (size_t)n * DIS_GT;
        float q[NMS_ROW];
        dis_label_row(label, q);
        row[0] = 1.f;
        row[1] = classes[n];
        row[2] = label[4];
        if (out_boxes)
            for (int i = 0; i < DIS_BOX; ++i) out_boxes[i] = q[6 + i];
        for (int v = 0; v < DIS_NV; ++v) {
            float box[DIS_BOX], bev, iou3d;
            dis_variant_box(a, h, z, tab, part[0], label, gmw_z ? gmw_z[n] : NAN, v, box);
            dis_overlaps(q, box, &bev, &iou3d);
            row[3 + v] = bev;
            row[3 + DIS_NV + v] = iou3d;
            if (out_boxes)
                for (int i = 0; i < DIS_BOX; ++i) out_boxes[(1 + v) * DIS_BOX + i] = box[i];
        }
    }
    return DCD_OK;
}

extern "C" int host_dis_iou_accumulate(const float *dis, int n_slots, const float *edges, int n_bins, int num_classes,
                                       const double *thresholds, double *table, int64_t *outside)
{
    if (!dis || !table || !outside || !dis_tables_ok(n_slots, edges, n_bins, num_classes, thresholds)) return DCD_ERR_BAD_ARG;
    const int per_bin = DIS_NV * DIS_NMETRIC, cells = num_classes * n_bins * per_bin;
    for (int t = 0; t < cells; ++t) {
        const int metric = t % DIS_NMETRIC, v = (t / DIS_NMETRIC) % DIS_NV, bin = (t / per_bin) % n_bins, c = t / (per_bin * n_bins);
        const double *thr = thresholds + (c * DIS_NMETRIC + metric) * 2;
        dis_accumulate_cell(dis, n_slots, edges, n_bins, num_classes, c, bin, v, metric, thr[0], thr[1], table + (size_t)t * DIS_STATS);
    }
    for (int c = 0; c < num_classes; ++c) outside[c] += dis_count_outside(dis, n_slots, edges, n_bins, num_classes, c);
    return DCD_OK;
}
