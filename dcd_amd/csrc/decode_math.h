// Arithmetic of one detection candidate of the eval-time decode (include/dcd_hip.h, dcd_decode_detections).
//
// Written once for two compilations: decode.hip runs it with one workgroup per candidate, and tests/host/host_decode.cpp
// runs the same functions in plain loops on the host, so that the formulas can be held against the reference's own
// `PostProcessor` fixture without a GPU.  The host build is test infrastructure; the library has no host path.
//
// Follows DGDE/model/head/detector_infer.py:86-243 in its order, with the helpers of DGDE/model/anno_encoder.py cited per
// block.  Every stage is the chain's expression in the chain's order of operations; nothing here is contracted into a
// fused multiply-add (the pragma below), so the device build, the host build and the op-by-op chain differ by the
// rounding of exp / atan2 / sin / cos and the order of two sums only.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dcd_hip.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

#ifdef __HIPCC__
#define DD_HD __host__ __device__ __forceinline__
#else
#define DD_HD inline
#endif

// the explicitly rounded operations of the edge solver (heads.hip, edge_depth_fwd): the same on the host, where nothing
// contracts them (tests/host/host_decode.cpp is built without FMA contraction)
#if defined(__HIP_DEVICE_COMPILE__)
#define DD_ADD(a, b) __fadd_rn((a), (b))
#define DD_SUB(a, b) __fsub_rn((a), (b))
#define DD_MUL(a, b) __fmul_rn((a), (b))
#define DD_DIV(a, b) __fdiv_rn((a), (b))
#else
#define DD_ADD(a, b) ((a) + (b))
#define DD_SUB(a, b) ((a) - (b))
#define DD_MUL(a, b) ((a) * (b))
#define DD_DIV(a, b) ((a) / (b))
#endif

#define DD_PI 3.14159265358979323846f
#define DD_LANES 128      // lanes of the fixed-order pair sum: the workgroup of decode.hip, a plain loop on the host
#define DD_TABLE 16       // floats per image: pad_x, pad_y, width, height, P (3 x 4, row-major)

// clamp / relu that pass a NaN on, as torch.clamp / F.relu do
DD_HD float dd_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
DD_HD float dd_relu(float x) { return x < 0.f ? 0.f : x; }
DD_HD float dd_wrap(float a)
{
    a = a > DD_PI ? a - 2.f * DD_PI : a;
    return a < -DD_PI ? a + 2.f * DD_PI : a;
}

// What stages 1-8 leave for the rest: everything of a candidate that does not need the dense key points.
struct DdHead {
    float cls, score;
    float cx, cy, off_x, off_y;     // heat-map cell and the 3d_offset head
    float box[4];
    float dims[3];                  // (l, h, w)
    float fused_depth, depth_error;
    int best;                       // arg-max of 1 / sigma: 0 direct depth, 1 centre line, 2 / 3 the corner groups
    float roty, alpha;
};

// The four depth estimates of stages 3-4 and their sigmas of stage 5, in the fusion's order: 0 direct depth, 1 centre line,
// 2 / 3 the corner groups.  The decode keeps them to itself; the depth report (depth_report_math.h) asks for them.
struct DdDepths {
    float depth[4], sigma[4];
};

// (centre + offset) * down_ratio - pad, back-projected at `depth` (decode_location_flatten, anno_encoder.py:147-161)
DD_HD void dd_location(const dcd_decode_args &a, const DdHead &h, const float *tab, float depth, float *loc)
{
    const float *P = tab + 4;
    const float cu = P[2], cv = P[6], fu = P[0], fv = P[5];
    const float bx = P[3] / (-fu), by = P[7] / (-fv);
    const float u = (h.cx + h.off_x) * a.down_ratio - tab[0];
    const float v = (h.cy + h.off_y) * a.down_ratio - tab[1];
    loc[0] = ((u - cu) * depth) / fu + bx;
    loc[1] = ((v - cv) * depth) / fv + by;
    loc[2] = depth;
}

// Stages 1-8 (detector_infer.py:104-180).  vec: the candidate's C head outputs; tab: its image's row of the table.
// est: where the four depths and sigmas go as well, or null.
DD_HD DdHead dd_head(const dcd_decode_args &a, const float *vec, float score, float cls, float y, float x, const float *tab,
                     DdDepths *est = nullptr)
{
    DdHead h;
    h.cls = cls;
    h.score = score;
    h.cx = x;
    h.cy = y;
    h.off_x = vec[a.ch_offset];
    h.off_y = vec[a.ch_offset + 1];

    // 1. the 2-D box: FCOS distances, relu'd, un-padded, clamped to the image (decode_box2d_fcos, anno_encoder.py:75-91)
    {
        const float *o = vec + a.ch_box2d;
        const float raw[4] = {x - dd_relu(o[0]), y - dd_relu(o[1]), x + dd_relu(o[2]), y + dd_relu(o[3])};
        for (int i = 0; i < 4; ++i) {
            float b = raw[i] * a.down_ratio - tab[i & 1];
            b = b < 0.f ? 0.f : b;                                  // clamp(min=0): a NaN passes
            const float lim = tab[2 + (i & 1)] - 1.f;
            h.box[i] = lim < b ? lim : b;                           // torch.min(box, lim)
        }
    }

    // 2. dimensions (decode_dimension, anno_encoder.py:226-252): (l, h, w)
    int ci = (int)cls;
    ci = ci < 0 ? 0 : (ci >= a.num_classes ? a.num_classes - 1 : ci);
    for (int i = 0; i < 3; ++i) {
        float d = vec[a.ch_dims + i];
        if (a.dim_mode == DCD_DECODE_DIM_EXP) d = expf(d);
        if (a.dim_mode != DCD_DECODE_DIM_NONE) d = a.dim_std_on ? d * a.dim_std[ci][i] + a.dim_mean[ci][i] : d * a.dim_mean[ci][i];
        h.dims[i] = d;
    }

    // 3. direct depth (decode_depth, anno_encoder.py:130-145)
    DdDepths four;
    float *depths = four.depth, *sigma = four.sigma;
    {
        const float d = vec[a.ch_depth];
        float z;
        if (a.depth_mode == DCD_DECODE_DEPTH_EXP) z = expf(d);
        else if (a.depth_mode == DCD_DECODE_DEPTH_LINEAR) z = d * a.depth_ref[1] + a.depth_ref[0];
        else z = 1.f / (1.f / (1.f + expf(-d))) - 1.f;
        depths[0] = dd_clamp(z, a.depth_lo, a.depth_hi);
    }

    // 4. depths from the projected heights of the centre line and the two corner groups
    //    (decode_depth_from_keypoints_batch, anno_encoder.py:193-224): key points 8-9 | 0-4, 2-6 | 1-5, 3-7
    {
        const float *ky = vec + a.ch_corner + 1;                    // y of key point k at ky[2 k]
        const int top[5] = {8, 0, 2, 1, 3}, bottom[5] = {9, 4, 6, 5, 7};
        const float fh = tab[4] * h.dims[1];
        float d[5];
        for (int i = 0; i < 5; ++i) d[i] = fh / (dd_relu(ky[2 * top[i]] - ky[2 * bottom[i]]) * a.down_ratio + a.eps);
        depths[1] = dd_clamp(d[0], a.depth_lo, a.depth_hi);
        depths[2] = dd_clamp((d[1] + d[2]) / 2.f, a.depth_lo, a.depth_hi);
        depths[3] = dd_clamp((d[3] + d[4]) / 2.f, a.depth_lo, a.depth_hi);
    }

    // 5. sigma = exp(log sigma)
    sigma[0] = expf(vec[a.ch_depth_unc]);
    for (int i = 0; i < 3; ++i) sigma[1 + i] = expf(vec[a.ch_corner_unc + i]);

    // 6. inverse-uncertainty weights (detector_infer.py:150-170); the arg-max compares 1 / sigma, the first maximum wins
    {
        float w[4], total = 0.f;
        h.best = 0;
        for (int i = 0; i < 4; ++i) {
            w[i] = 1.f / sigma[i];
            if (w[i] > w[h.best]) h.best = i;
            total += w[i];
        }
        float depth = 0.f, err = 0.f;
        for (int i = 0; i < 4; ++i) {
            const float wn = w[i] / total;
            depth += depths[i] * wn;
            err += wn * sigma[i];
        }
        h.fused_depth = depth;
        h.depth_error = err;
    }

    // 7. the coarse location, for the viewing ray only
    float coarse[3];
    dd_location(a, h, tab, h.fused_depth, coarse);

    // 8. multi-bin orientation (decode_axes_orientation, anno_encoder.py:254-304): the bin whose softmax value is largest
    {
        const float *c = vec + a.ch_ori_cls, *o = vec + a.ch_ori_off;
        const float centers[4] = {0.f, DD_PI / 2.f, DD_PI, -DD_PI / 2.f};
        int best = 0;
        float best_p = 0.f;
        for (int b = 0; b < a.n_bins; ++b) {
            const float m = c[2 * b] > c[2 * b + 1] ? c[2 * b] : c[2 * b + 1];
            const float e0 = expf(c[2 * b] - m), e1 = expf(c[2 * b + 1] - m);
            const float p = e1 / (e0 + e1);
            if (b == 0 || p > best_p) {
                best = b;
                best_p = p;
            }
        }
        const float ori = atan2f(o[2 * best], o[2 * best + 1]) + centers[best];
        const float ray = atan2f(coarse[0], coarse[2]);
        h.roty = dd_wrap(ori + ray);
        h.alpha = dd_wrap(ori);
    }
    if (est) *est = four;
    return h;
}

// 9. dense key point k: image pixels (u, v) = (kp + centre + offset) * 4 - pad (decode_kpts_2d_img, anno_encoder.py:392-393)
//    and its 3-D point.  sn, cs = sin, cos of the candidate's yaw.  Returns what the edge solver keeps of the key point:
//    v' = (v - c_v) / f_v, Y and v' (X sin - Z cos).
struct DdKeypoint {
    float u, v, X, Y, Z;
    float vn, vC;
};

DD_HD DdKeypoint dd_keypoint(const dcd_decode_args &a, const float *vec, const DdHead &h, const float *tab, int k, float sn, float cs)
{
    DdKeypoint p;
    p.u = (vec[a.ch_kpts2d + 2 * k] + (h.cx + h.off_x)) * 4.f - tab[0];
    p.v = (vec[a.ch_kpts2d + 2 * k + 1] + (h.cy + h.off_y)) * 4.f - tab[1];
    p.X = vec[a.ch_kpts3d + 3 * k];
    p.Y = vec[a.ch_kpts3d + 3 * k + 1];
    p.Z = vec[a.ch_kpts3d + 3 * k + 2];
    p.vn = DD_DIV(DD_SUB(p.v, tab[4 + 6]), tab[4 + 5]);
    p.vC = DD_MUL(p.vn, DD_SUB(DD_MUL(p.X, sn), DD_MUL(p.Z, cs)));
    return p;
}

// 10. one lane's share of the edge-constraint depths (decode_pairs_kpts_depth, anno_encoder.py:326-390; the per-pair
//     expression of heads.hip's edge_depth_fwd with the clamp [2, 80], minus P[2][3]): pairs lane, lane + DD_LANES, ... of
//     the row-major upper triangle, added in that order.
DD_HD float dd_pair_partial(int lane, int K, const float *vn, const float *Y, const float *vC, float b3)
{
    float acc = 0.f;
    int i = 0, j = 1 + lane;
    for (;;) {
        while (j >= K && i < K - 1) {
            j -= K;
            ++i;
            j += i + 1;
        }
        if (i >= K - 1) break;
        const float hm = DD_ADD(DD_SUB(Y[i], Y[j]), DD_SUB(vC[i], vC[j]));
        const float dv = fabsf(DD_SUB(vn[i], vn[j]));
        float z = DD_DIV(fabsf(hm), fmaxf(dv, 1e-10f));
        z = fminf(fmaxf(z, 2.f), 80.f);
        acc = DD_ADD(acc, DD_SUB(z, b3));
        j += DD_LANES;
    }
    return acc;
}

// the edge depth inference reports: the mean over all nk (nk - 1) / 2 pairs of the tree's sum of the lanes' partials
DD_HD float dd_edge_depth(const dcd_decode_args &a, float pair_sum)
{
    const int npairs = a.nk * (a.nk - 1) / 2;
    return pair_sum / (float)npairs;
}

// 11-14. the final location at the edge depth (the mean over all pairs), the (h, w, l) dimensions, the confidence and
//        the 14-float row [cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, roty, score]; aux = raw score, depth error,
//        confidence, arg-max index.
DD_HD void dd_finish(const dcd_decode_args &a, const DdHead &h, const float *tab, float pair_sum, float *row, float *aux)
{
    const float edge_depth = dd_edge_depth(a, pair_sum);
    float loc[3];
    dd_location(a, h, tab, edge_depth, loc);
    loc[1] += h.dims[1] / 2.f;
    const float conf = 1.f - dd_clamp(h.depth_error, 0.01f, 1.f);
    float score = h.score;
    if (a.uncertainty_as_conf) {
        score = score * conf;
        if (score != score) score = 0.f;                            // nan_to_num(nan=0, posinf=inf, neginf=-inf)
    }
    row[0] = h.cls;
    row[1] = h.alpha;
    for (int i = 0; i < 4; ++i) row[2 + i] = h.box[i];
    row[6] = h.dims[1];
    row[7] = h.dims[2];
    row[8] = h.dims[0];
    for (int i = 0; i < 3; ++i) row[9 + i] = loc[i];
    row[12] = h.roty;
    row[13] = score;
    aux[0] = h.score;
    aux[1] = h.depth_error;
    aux[2] = conf;
    aux[3] = (float)h.best;
}

// What the launchers of decode.hip and depth_report.hip accept of a `dcd_decode_args` (host code): the sizes the kernels' LDS
// arrays hold, the modes the header implements, every head inside a row of C channels.
inline bool dd_args_ok(const dcd_decode_args &a)
{
    if (a.B < 1 || a.K < 1 || a.K > DD_LANES || a.nk < 2 || a.nk > DD_LANES || a.C < 1) return false;
    if ((int64_t)a.B * a.K > 0x7fffffffLL) return false;
    if (a.n_bins < 1 || a.n_bins > 4 || a.num_classes < 1 || a.num_classes > DCD_DECODE_MAX_CLASSES) return false;
    if (a.orientation != DCD_DECODE_ORI_MULTIBIN) return false;
    if (a.dim_mode < DCD_DECODE_DIM_NONE || a.dim_mode > DCD_DECODE_DIM_LINEAR) return false;
    if (a.depth_mode < DCD_DECODE_DEPTH_INV_SIGMOID || a.depth_mode > DCD_DECODE_DEPTH_LINEAR) return false;
    const int start[11] = {a.ch_box2d, a.ch_offset, a.ch_corner, a.ch_corner_unc, a.ch_dims, a.ch_ori_cls, a.ch_ori_off, a.ch_depth,
                           a.ch_depth_unc, a.ch_kpts2d, a.ch_kpts3d};
    const int width[11] = {4, 2, 20, 3, 3, 2 * a.n_bins, 2 * a.n_bins, 1, 1, 2 * a.nk, 3 * a.nk};
    for (int i = 0; i < 11; ++i)
        if (start[i] < 0 || start[i] > a.C - width[i]) return false;
    return true;
}
