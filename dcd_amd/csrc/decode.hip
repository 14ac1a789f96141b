// decode.hip -- the eval-time decode of a whole batch of detections in one launch (include/dcd_hip.h, dcd_decode_detections).
//
// One workgroup of DD_LANES threads (two waves) per candidate.  The scalar stages (box, dimensions, depths, fusion,
// orientation: a few dozen operations on ~40 head outputs) are evaluated by every lane from the same addresses -- cheaper
// than one lane computing and a broadcast through LDS -- then lane k takes dense key point k, the lanes share the
// nk (nk - 1) / 2 pairs in pair order, a tree through LDS adds the DD_LANES partials in a fixed order, and lane 0 writes the row.
// LDS per workgroup: 3 nk floats of key points + DD_LANES partials.  The arithmetic is csrc/decode_math.h.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dcd_hip.h"
#include "decode_math.h"

namespace {

constexpr int DECODE_MAXK = DD_LANES;      // K and nk: the sizes dd_args_ok lets through

__global__ __launch_bounds__(DD_LANES) void decode_detections(const float *__restrict__ vectors, const float *__restrict__ scores,
                                                              const float *__restrict__ classes, const float *__restrict__ ys,
                                                              const float *__restrict__ xs, const float *__restrict__ table,
                                                              const dcd_decode_args a, float *__restrict__ rows,
                                                              float *__restrict__ aux, float *__restrict__ kpts2d,
                                                              float *__restrict__ kpts3d)
{
    __shared__ float s_vn[DECODE_MAXK], s_Y[DECODE_MAXK], s_vC[DECODE_MAXK], s_part[DD_LANES];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int nk = a.nk;
    const float *vec = vectors + (size_t)n * a.C;
    const float *tab = table + (size_t)(n / a.K) * DD_TABLE;

    const DdHead h = dd_head(a, vec, scores[n], classes[n], ys[n], xs[n], tab);
    const float sn = sinf(h.roty), cs = cosf(h.roty);

    if (tid < nk) {
        const DdKeypoint p = dd_keypoint(a, vec, h, tab, tid, sn, cs);
        s_vn[tid] = p.vn;
        s_Y[tid] = p.Y;
        s_vC[tid] = p.vC;
        if (a.records) {
            const float *P = tab + 4;
            float *k2 = kpts2d + ((size_t)n * nk + tid) * 2, *k3 = kpts3d + ((size_t)n * nk + tid) * 3;
            k2[0] = (p.u - P[2]) / P[0];
            k2[1] = (p.v - P[6]) / P[5];
            k3[0] = p.X;
            k3[1] = p.Y;
            k3[2] = p.Z;
        }
    }
    __syncthreads();

    s_part[tid] = dd_pair_partial(tid, nk, s_vn, s_Y, s_vC, tab[4 + 11]);
    __syncthreads();
    for (int s = DD_LANES / 2; s > 0; s >>= 1) {
        if (tid < s) s_part[tid] = DD_ADD(s_part[tid], s_part[tid + s]);
        __syncthreads();
    }

    if (tid == 0) dd_finish(a, h, tab, s_part[0], rows + (size_t)n * 14, aux + (size_t)n * 4);
}

}  // namespace

extern "C" int dcd_decode_detections(void *stream_, const float *vectors, const float *scores, const float *classes, const float *ys,
                                     const float *xs, const float *image_table, const dcd_decode_args *args, float *rows, float *aux,
                                     float *kpts2d, float *kpts3d)
{
    if (!args) return DCD_ERR_BAD_ARG;
    const dcd_decode_args a = *args;
    if (!vectors || !scores || !classes || !ys || !xs || !image_table || !rows || !aux) return DCD_ERR_BAD_ARG;
    if (a.records && (!kpts2d || !kpts3d)) return DCD_ERR_BAD_ARG;
    if (!dd_args_ok(a)) return DCD_ERR_BAD_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(decode_detections, dim3((unsigned)(a.B * a.K)), dim3(DD_LANES), 0, stream, vectors, scores, classes, ys, xs,
                       image_table, a, rows, aux, kpts2d, kpts3d);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}
