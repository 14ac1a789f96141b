// dis_iou.hip -- the disentangled IoU report's two kernels (include/dcd_hip.h, dcd_dis_iou_estimates and dcd_dis_iou_accumulate).
//
// dis_iou_estimates is depth_estimates (depth_report.hip) with a different last stage: one workgroup of DD_LANES threads per
// object slot, the scalar stages evaluated by every lane, lane k takes dense key point k, the lanes share the nk (nk - 1) / 2
// pairs in pair order, a tree through LDS adds the partials in decode.hip's order -- so `full` and `depth:edges` carry the decode's
// bits.  Then lanes 0-14 build one variant's box each and clip it against the label (the rotated clip is the expensive part,
// and the fifteen are independent), and lane 15 writes the leading columns and the label's box.  A slot whose `valid` byte is 0
// never reads its vector and writes zeros.
// dis_iou_accumulate gives every (class, bin, variant, metric) cell one thread, which walks the batch's rows in slot order and
// adds the ones that are its own to its six doubles, as depth_accumulate does: no atomics, no reduction across threads.
// The arithmetic is csrc/dis_iou_math.h.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dcd_hip.h"
#include "dis_iou_math.h"

namespace {

constexpr int ACC_THREADS = 256;

struct AccArgs {
    int n_slots, n_bins, num_classes;
    float edges[DR_MAX_BINS + 1];
    double thresholds[DR_MAX_CLASSES][DIS_NMETRIC][2];
};

__global__ __launch_bounds__(DD_LANES) void dis_iou_estimates(const float *__restrict__ vectors, const float *__restrict__ ys,
                                                              const float *__restrict__ xs, const float *__restrict__ classes,
                                                              const float *__restrict__ gt, const uint8_t *__restrict__ valid,
                                                              const float *__restrict__ table, const float *__restrict__ gmw_z,
                                                              const dcd_decode_args a, float *__restrict__ dis, float *__restrict__ boxes)
{
    __shared__ float s_vn[DD_LANES], s_Y[DD_LANES], s_vC[DD_LANES], s_part[DD_LANES];
    const int n = blockIdx.x, tid = threadIdx.x;
    float *row = dis + (size_t)n * DIS_ROW;
    float *out_boxes = boxes ? boxes + (size_t)n * DIS_NBOX * DIS_BOX : nullptr;
    if (!valid[n]) {                                                  // the whole workgroup: no barrier is skipped by some lanes only
        if (tid < DIS_ROW) row[tid] = 0.f;
        if (out_boxes && tid < DIS_NBOX * DIS_BOX) out_boxes[tid] = 0.f;
        return;
    }
    const int nk = a.nk;
    const float *vec = vectors + (size_t)n * a.C;
    const float *tab = table + (size_t)(n / a.K) * DD_TABLE;

    DdDepths z;
    const DdHead h = dd_head(a, vec, 0.f, classes[n], ys[n], xs[n], tab, &z);
    const float sn = sinf(h.roty), cs = cosf(h.roty);

    if (tid < nk) {
        const DdKeypoint p = dd_keypoint(a, vec, h, tab, tid, sn, cs);
        s_vn[tid] = p.vn;
        s_Y[tid] = p.Y;
        s_vC[tid] = p.vC;
    }
    __syncthreads();

    s_part[tid] = dd_pair_partial(tid, nk, s_vn, s_Y, s_vC, tab[4 + 11]);
    __syncthreads();
    for (int s = DD_LANES / 2; s > 0; s >>= 1) {
        if (tid < s) s_part[tid] = DD_ADD(s_part[tid], s_part[tid + s]);
        __syncthreads();
    }

    if (tid > DIS_NV) return;                                         // (after the last barrier)
    float label[DIS_GT], q[NMS_ROW];
    for (int i = 0; i < DIS_GT; ++i) label[i] = gt[(size_t)n * DIS_GT + i];
    dis_label_row(label, q);
    if (tid == DIS_NV) {
        row[0] = 1.f;
        row[1] = classes[n];
        row[2] = label[4];
        if (out_boxes)
            for (int i = 0; i < DIS_BOX; ++i) out_boxes[i] = q[6 + i];
        return;
    }
    float box[DIS_BOX], bev, iou3d;
    dis_variant_box(a, h, z, tab, s_part[0], label, gmw_z ? gmw_z[n] : __int_as_float(0x7fc00000), tid, box);
    dis_overlaps(q, box, &bev, &iou3d);
    row[3 + tid] = bev;
    row[3 + DIS_NV + tid] = iou3d;
    if (out_boxes)
        for (int i = 0; i < DIS_BOX; ++i) out_boxes[(1 + tid) * DIS_BOX + i] = box[i];
}

__global__ __launch_bounds__(ACC_THREADS) void dis_iou_accumulate(const float *__restrict__ dis, const AccArgs a, double *__restrict__ table,
                                                                  int64_t *__restrict__ outside)
{
    const int t = blockIdx.x * ACC_THREADS + threadIdx.x;
    const int per_bin = DIS_NV * DIS_NMETRIC, cells = a.num_classes * a.n_bins * per_bin;
    if (t < cells) {
        const int metric = t % DIS_NMETRIC, v = (t / DIS_NMETRIC) % DIS_NV, bin = (t / per_bin) % a.n_bins, c = t / (per_bin * a.n_bins);
        dis_accumulate_cell(dis, a.n_slots, a.edges, a.n_bins, a.num_classes, c, bin, v, metric, a.thresholds[c][metric][0],
                            a.thresholds[c][metric][1], table + (size_t)t * DIS_STATS);
    } else if (t < cells + a.num_classes) {
        const int c = t - cells;
        outside[c] += dis_count_outside(dis, a.n_slots, a.edges, a.n_bins, a.num_classes, c);
    }
}

}  // namespace

extern "C" int dcd_dis_iou_estimates(void *stream_, const float *vectors, const float *ys, const float *xs, const float *classes,
                                     const float *gt, const uint8_t *valid, const float *image_table, const float *gmw_z,
                                     const dcd_decode_args *args, float *dis, float *boxes)
{
    if (!args) return DCD_ERR_BAD_ARG;
    const dcd_decode_args a = *args;
    if (!vectors || !ys || !xs || !classes || !gt || !valid || !image_table || !dis) return DCD_ERR_BAD_ARG;
    if (!dd_args_ok(a)) return DCD_ERR_BAD_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(dis_iou_estimates, dim3((unsigned)(a.B * a.K)), dim3(DD_LANES), 0, stream, vectors, ys, xs, classes, gt, valid,
                       image_table, gmw_z, a, dis, boxes);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}

extern "C" int dcd_dis_iou_accumulate(void *stream_, const float *dis, int n_slots, const float *edges, int n_bins, int num_classes,
                                      const double *thresholds, double *table, int64_t *outside)
{
    if (!dis || !table || !outside) return DCD_ERR_BAD_ARG;
    if (!dis_tables_ok(n_slots, edges, n_bins, num_classes, thresholds)) return DCD_ERR_BAD_ARG;
    if (n_slots == 0) return DCD_OK;
    AccArgs a;
    a.n_slots = n_slots;
    a.n_bins = n_bins;
    a.num_classes = num_classes;
    for (int i = 0; i <= DR_MAX_BINS; ++i) a.edges[i] = i <= n_bins ? edges[i] : 0.f;
    for (int c = 0; c < DR_MAX_CLASSES; ++c)
        for (int m = 0; m < DIS_NMETRIC; ++m)
            for (int k = 0; k < 2; ++k) a.thresholds[c][m][k] = c < num_classes ? thresholds[(c * DIS_NMETRIC + m) * 2 + k] : 0.0;
    const int threads = num_classes * n_bins * DIS_NV * DIS_NMETRIC + num_classes;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(dis_iou_accumulate, dim3((unsigned)((threads + ACC_THREADS - 1) / ACC_THREADS)), dim3(ACC_THREADS), 0, stream, dis,
                       a, table, outside);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}
