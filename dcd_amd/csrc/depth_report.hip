// depth_report.hip -- every depth estimate of a batch of labelled objects in one launch, and their errors booked into running
// tables in a second (include/dcd_hip.h, dcd_depth_estimates and dcd_depth_accumulate).
//
// depth_estimates is decode.hip's kernel cut down to the depths: one workgroup of DD_LANES threads per object slot, the scalar
// stages evaluated by every lane, lane k takes dense key point k, the lanes share the nk (nk - 1) / 2 pairs in pair order, a tree
// through LDS adds the partials in decode.hip's order, lane 0 writes the row.  A slot whose `valid` byte is 0 never reads its
// vector and writes zeros.
// depth_accumulate gives every (class, bin, method) cell one thread, which walks the batch's rows in slot order and adds the
// ones that are its own to its five doubles: no atomics, no reduction across threads, so a cell's sums are one fixed sequence of
// additions over the objects of the split however the split is cut into calls.  It is as slow as that sounds (a few hundred
// rows, read by 1 280 threads from L2) and is meant to be: the pass behind it runs a backbone per batch.
// The arithmetic is csrc/depth_report_math.h.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dcd_hip.h"
#include "depth_report_math.h"

namespace {

constexpr int ACC_THREADS = 256;

struct AccArgs {
    int n_slots, n_bins, num_classes;
    float edges[DR_MAX_BINS + 1];
};

__global__ __launch_bounds__(DD_LANES) void depth_estimates(const float *__restrict__ vectors, const float *__restrict__ ys,
                                                            const float *__restrict__ xs, const float *__restrict__ classes,
                                                            const float *__restrict__ gt_z, const uint8_t *__restrict__ valid,
                                                            const float *__restrict__ table, const dcd_decode_args a,
                                                            float *__restrict__ est)
{
    __shared__ float s_vn[DD_LANES], s_Y[DD_LANES], s_vC[DD_LANES], s_part[DD_LANES];
    const int n = blockIdx.x, tid = threadIdx.x;
    float *row = est + (size_t)n * DR_ROW;
    if (!valid[n]) {                                                  // the whole workgroup: no barrier is skipped by some lanes only
        if (tid < DR_ROW) row[tid] = 0.f;
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

    if (tid == 0) {
        const float gz = gt_z[n];
        float d[DR_NM];
        dr_methods(h, z, gz, d);
        d[DR_EDGES] = dd_edge_depth(a, s_part[0]);
        d[DR_GMW] = __int_as_float(0x7fc00000);                       // the caller's column: NaN until it is filled
        row[0] = 1.f;
        row[1] = classes[n];
        row[2] = gz;
        for (int m = 0; m < DR_NM; ++m) row[3 + m] = d[m];
    }
}

__global__ __launch_bounds__(ACC_THREADS) void depth_accumulate(const float *__restrict__ est, const AccArgs a, double *__restrict__ table,
                                                                int64_t *__restrict__ outside)
{
    const int t = blockIdx.x * ACC_THREADS + threadIdx.x;
    const int cells = a.num_classes * a.n_bins * DR_NM;
    if (t < cells) {
        const int m = t % DR_NM, bin = (t / DR_NM) % a.n_bins, c = t / (DR_NM * a.n_bins);
        dr_accumulate_cell(est, a.n_slots, a.edges, a.n_bins, a.num_classes, c, bin, m, table + (size_t)t * DR_STATS);
    } else if (t < cells + a.num_classes) {
        const int c = t - cells;
        outside[c] += dr_count_outside(est, a.n_slots, a.edges, a.n_bins, a.num_classes, c);
    }
}

}  // namespace

extern "C" int dcd_depth_estimates(void *stream_, const float *vectors, const float *ys, const float *xs, const float *classes,
                                   const float *gt_z, const uint8_t *valid, const float *image_table, const dcd_decode_args *args,
                                   float *est)
{
    if (!args) return DCD_ERR_BAD_ARG;
    const dcd_decode_args a = *args;
    if (!vectors || !ys || !xs || !classes || !gt_z || !valid || !image_table || !est) return DCD_ERR_BAD_ARG;
    if (!dd_args_ok(a)) return DCD_ERR_BAD_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(depth_estimates, dim3((unsigned)(a.B * a.K)), dim3(DD_LANES), 0, stream, vectors, ys, xs, classes, gt_z, valid,
                       image_table, a, est);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}

extern "C" int dcd_depth_accumulate(void *stream_, const float *est, int n_slots, const float *edges, int n_bins, int num_classes,
                                    double *table, int64_t *outside)
{
    if (!est || !table || !outside) return DCD_ERR_BAD_ARG;
    if (!dr_tables_ok(n_slots, edges, n_bins, num_classes)) return DCD_ERR_BAD_ARG;
    if (n_slots == 0) return DCD_OK;
    AccArgs a;
    a.n_slots = n_slots;
    a.n_bins = n_bins;
    a.num_classes = num_classes;
    for (int i = 0; i <= DR_MAX_BINS; ++i) a.edges[i] = i <= n_bins ? edges[i] : 0.f;
    const int threads = num_classes * n_bins * DR_NM + num_classes;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(depth_accumulate, dim3((unsigned)((threads + ACC_THREADS - 1) / ACC_THREADS)), dim3(ACC_THREADS), 0, stream, est,
                       a, table, outside);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}
