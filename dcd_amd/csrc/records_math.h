// Arithmetic of one object slot of GMW's training records (include/dcd_hip.h, dcd_gmw_train_records).
//
// Written once for two compilations, in the way of decode_math.h: records.hip runs it with one wave per object slot, and
// tests/host/host_records.cpp runs the same functions in plain loops on the host, so that the formulas can be held against the
// reference's own `Loss_Computation.gen_data` fixture without a GPU.  The host build is test infrastructure; the library has
// no host path.
//
// What it restates is the part of `Loss_Computation.prepare_predictions` / `generate_data` that GMW's records are a function
// of (DGDE/model/head/detector_loss.py:148-173, :217-403), for a slot (b, m) with reg_mask[b, m] != 0:
//   kps_img        decode_kpts_2d_img (anno_encoder.py:392-393) with the TARGET offset          -> rm_kpt_img
//   edge depths    decode_pairs_kpts_depth in its training form (anno_encoder.py:326-390): the per-pair expression of
//                  heads.hip's edge_depth_fwd, the 1 500 pairs of largest |v'_i - v'_j|           -> rm_pair (host selection)
//   pred_depth     their mean (detector_loss.py:390) as a fixed-order sum                        -> rm_lane_partial + tree
//   locations      decode_location_flatten (anno_encoder.py:147-161) from the (B, 6) table       -> rm_location
//   pred_rot       decode_axes_orientation, multi-bin (anno_encoder.py:254-304)                   -> rm_roty
//   kpts_2d        (kps_img - (K[0,2], K[1,2])) / (K[0,0], K[1,1]) with image 0's K (:150-153)    -> rm_normalise
// Nothing here is contracted into a fused multiply-add (the pragma below; -ffp-contract=off on the host build).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dcd_hip.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

#ifdef __HIPCC__
#define RM_HD __host__ __device__ __forceinline__
#else
#define RM_HD inline
#endif

// the explicitly rounded operations of the edge solver (heads.hip, edge_depth_fwd); plain operators on the host
#if defined(__HIP_DEVICE_COMPILE__)
#define RM_ADD(a, b) __fadd_rn((a), (b))
#define RM_SUB(a, b) __fsub_rn((a), (b))
#define RM_MUL(a, b) __fmul_rn((a), (b))
#define RM_DIV(a, b) __fdiv_rn((a), (b))
#else
#define RM_ADD(a, b) ((a) + (b))
#define RM_SUB(a, b) ((a) - (b))
#define RM_MUL(a, b) ((a) * (b))
#define RM_DIV(a, b) ((a) / (b))
#endif

#define RM_PI 3.14159265358979323846f
#define RM_LANES 64        // lanes of the fixed-order mean: one wave of records.hip, a plain loop on the host
#define RM_TOPK 1500       // pairs the training form of the solver keeps (anno_encoder.py:326 num_k)
#define RM_ZMIN 2.0f
#define RM_ZMAX 80.0f
#define RM_MAXK 128

// pairs the solver keeps for nk key points: 1 500, or all of them where there are fewer
RM_HD int rm_topk(int nk)
{
    const int npairs = nk * (nk - 1) / 2;
    return npairs < RM_TOPK ? npairs : RM_TOPK;
}

RM_HD float rm_wrap(float a)
{
    a = a > RM_PI ? a - 2.f * RM_PI : a;
    return a < -RM_PI ? a + 2.f * RM_PI : a;
}

// The target side of a slot, as the target tables hold it.
struct RmSlot {
    float cx, cy;           // target_centers (int32 in the table)
    float off_x, off_y;     // offset_3D: the GT offset
    float pad_x, pad_y;     // pad_size[b] (int64 in the table)
};

RM_HD RmSlot rm_slot(const int32_t *centers, const float *offset_3D, const int64_t *pad_size, int b, int slot)
{
    RmSlot s;
    s.cx = (float)centers[(size_t)slot * 2];
    s.cy = (float)centers[(size_t)slot * 2 + 1];
    s.off_x = offset_3D[(size_t)slot * 2];
    s.off_y = offset_3D[(size_t)slot * 2 + 1];
    s.pad_x = (float)pad_size[(size_t)b * 2];
    s.pad_y = (float)pad_size[(size_t)b * 2 + 1];
    return s;
}

// key point k in image pixels: (kp + (centre + GT offset)) * 4 - pad (decode_kpts_2d_img; the 4 is the reference's literal)
RM_HD void rm_kpt_img(const dcd_records_args &a, const float *vec, const RmSlot &s, int k, float *uv)
{
    uv[0] = (vec[a.ch_kpts2d + 2 * k] + (s.cx + s.off_x)) * 4.f - s.pad_x;
    uv[1] = (vec[a.ch_kpts2d + 2 * k + 1] + (s.cy + s.off_y)) * 4.f - s.pad_y;
}

// What the solver keeps of a key point (edge_depth_fwd): v' = (v - c_v) / f_v, Y, v' (X sin - Z cos), P = Calib_P[b, m].
RM_HD void rm_solver_point(float v, const float *xyz, const float *P, float sn, float cs, float *vn, float *Y, float *vC)
{
    *vn = RM_DIV(RM_SUB(v, P[6]), P[5]);
    *Y = xyz[1];
    *vC = RM_MUL(*vn, RM_SUB(RM_MUL(xyz[0], sn), RM_MUL(xyz[2], cs)));
}

// Pair (i, j): its depth clamped to [2, 80] (before P[2][3] is subtracted) and |v'_i - v'_j|, the quantity the top-k orders by.
RM_HD float rm_pair(int i, int j, const float *vn, const float *Y, const float *vC, float *dv)
{
    const float hm = RM_ADD(RM_SUB(Y[i], Y[j]), RM_SUB(vC[i], vC[j]));
    *dv = fabsf(RM_SUB(vn[i], vn[j]));
    const float z = RM_DIV(fabsf(hm), fmaxf(*dv, 1e-10f));
    return fminf(fmaxf(z, RM_ZMIN), RM_ZMAX);
}

// One lane's share of the mean over the kept depths: ranks lane, lane + RM_LANES, ... in rank order.  The lanes' partials are
// then added as a tree (part[t] += part[t + s], s = RM_LANES / 2 .. 1) and divided by the count.
RM_HD float rm_lane_partial(int lane, int topk, const float *depths)
{
    float acc = 0.f;
    for (int r = lane; r < topk; r += RM_LANES) acc = RM_ADD(acc, depths[r]);
    return acc;
}

// (centre + offset) * down_ratio - pad, back-projected at `depth` with a row [c_u, c_v, f_u, f_v, b_x, b_y] of the
// calibration table (decode_location_flatten in this project's table form: ((u - c) * z) / f + b)
RM_HD void rm_location(const dcd_records_args &a, const RmSlot &s, float off_x, float off_y, float depth, const float *tab, float *loc)
{
    const float u = (s.cx + off_x) * a.down_ratio - s.pad_x;
    const float v = (s.cy + off_y) * a.down_ratio - s.pad_y;
    loc[0] = ((u - tab[0]) * depth) / tab[2] + tab[4];
    loc[1] = ((v - tab[1]) * depth) / tab[3] + tab[5];
    loc[2] = depth;
}

// multi-bin orientation: the bin whose softmax value is largest (the first of equal ones), atan2 of its offsets plus the
// bin's centre, plus the viewing ray of `loc`, wrapped to [-pi, pi]
RM_HD float rm_roty(const dcd_records_args &a, const float *vec, const float *loc)
{
    const float *c = vec + a.ch_ori_cls, *o = vec + a.ch_ori_off;
    int best = 0;
    float best_p = 0.f, o0 = o[0], o1 = o[1];
    for (int b = 0; b < a.n_bins; ++b) {
        const float m = c[2 * b] > c[2 * b + 1] ? c[2 * b] : c[2 * b + 1];
        const float e0 = expf(c[2 * b] - m), e1 = expf(c[2 * b + 1] - m);
        const float p = e1 / (e0 + e1);
        if (b == 0 || p > best_p) {
            best = b;
            best_p = p;
            o0 = o[2 * b];
            o1 = o[2 * b + 1];
        }
    }
    // alpha_centers = [0, pi / 2, pi, -pi / 2]
    const float centre = best == 0 ? 0.f : (best == 1 ? RM_PI / 2.f : (best == 2 ? RM_PI : -RM_PI / 2.f));
    const float ori = atan2f(o0, o1) + centre;
    const float ray = atan2f(loc[0], loc[2]);
    return rm_wrap(ori + ray);
}

// K-normalised key point with the intrinsics of image 0 of the batch: tab0 = row 0 of the calibration table
RM_HD void rm_normalise(const float *uv, const float *tab0, float *out)
{
    out[0] = (uv[0] - tab0[0]) / tab0[2];
    out[1] = (uv[1] - tab0[1]) / tab0[3];
}

// Workspace of a call, in floats per slot: key points in pixels (nk x 2), 3-D key points (nk x 3), yaw, P (12), the kept
// depths and their pair indices (the solver's second output, which nothing here reads).
RM_HD size_t rm_workspace_floats(int slots, int nk)
{
    return (size_t)slots * ((size_t)nk * 5 + 13 + 2 * (size_t)rm_topk(nk));
}

struct RmWorkspace {
    float *kps, *kps3d, *rot, *P, *depth;
    int32_t *pair_idx;
};

RM_HD RmWorkspace rm_workspace(void *base, int slots, int nk)
{
    RmWorkspace w;
    w.kps = (float *)base;
    w.kps3d = w.kps + (size_t)slots * nk * 2;
    w.rot = w.kps3d + (size_t)slots * nk * 3;
    w.P = w.rot + slots;
    w.depth = w.P + (size_t)slots * 12;
    w.pair_idx = (int32_t *)(w.depth + (size_t)slots * rm_topk(nk));
    return w;
}

// Argument check shared by both builds: DCD_ERR_BAD_ARG for B < 1, M < 1, nk outside 2 .. 128, n_bins outside 1 .. 4 or a
// channel range outside [0, C).
RM_HD int rm_args_ok(const dcd_records_args &a)
{
    if (a.B < 1 || a.M < 1 || a.C < 1 || a.nk < 2 || a.nk > RM_MAXK || a.n_bins < 1 || a.n_bins > 4) return 0;
    if ((int64_t)a.B * a.M > 0x7fffffffLL / 2) return 0;
    const int start[5] = {a.ch_offset, a.ch_ori_cls, a.ch_ori_off, a.ch_kpts2d, a.ch_kpts3d};
    const int width[5] = {2, 2 * a.n_bins, 2 * a.n_bins, 2 * a.nk, 3 * a.nk};
    for (int i = 0; i < 5; ++i)
        if (start[i] < 0 || start[i] > a.C - width[i]) return 0;
    return 1;
}
