// Arithmetic of the mirrored-view merge (include/dcd_hip.h, dcd_tta_merge_detections; the rule is DESIGN.md "Mirrored-view
// test-time augmentation").
//
// Written once for two compilations, in the way of nms_math.h and decode_math.h: tta.hip runs it with one workgroup per image,
// tests/host/host_tta.cpp runs the same functions in plain loops on the host, so that the decisions and the fused floats can be
// held against a float64 restatement without a GPU.  The host build is test infrastructure; the library has no host path.
//
// Per image two blocks of K decoded rows (`write_detections`' 14 floats, nms_math.h) with their aux rows [raw score, depth
// error, confidence, arg-max]: view A, the frame as it is, and view M, the frame mirrored and decoded with the mirrored P of
// `flip_sample`.  Everything here is plain float32; the overlaps are nms_math.h's own (float64 ratios of float32 areas).
// The host build turns contraction off on its command line; this header sets no mode.
#pragma once
#include "nms_math.h"

#define TTA_MAXK NMS_MAXK
#define TTA_PI 3.14159265358979323846f
#define TTA_NO_MATCH (-1.0f)            // what the match table holds for a pair that may not match (overlaps are >= 0)

// An angle into [-pi, pi], one turn at a time as `convertRot2Alpha` does; four turns at most each way, so that an infinite
// angle ends the loop as a NaN does (the decode's angles lie within two turns).
NM_HD float tta_wrap(float a)
{
    for (int i = 0; i < 4 && a > TTA_PI; ++i) a -= 2 * TTA_PI;
    for (int i = 0; i < 4 && a < -TTA_PI; ++i) a += 2 * TTA_PI;
    return a;
}

// A row of view M back in view A's frame: the inverse of data/augment.py:flip_sample for an image `width` pixels wide.
NM_HD void tta_unmirror(const float *m, int width, float *out)
{
    for (int i = 0; i < NMS_ROW; ++i) out[i] = m[i];
    const float edge = (float)(width - 1);
    out[2] = edge - m[4];
    out[4] = edge - m[2];
    out[9] = -m[9];
    const float ry = m[12];
    out[12] = tta_wrap(ry < 0 ? -TTA_PI - ry : TTA_PI - ry);
    out[1] = tta_wrap(out[12] - atan2f(out[9], out[11]));
}

// May row m of view M be matched at all?  Every row whose raw score is a number.
NM_HD bool tta_eligible(float raw_m) { return raw_m == raw_m; }

// What the match table holds for (A candidate a, un-mirrored M row m): the overlap rounded to float32 when the pair may match
// -- m eligible, the same integer class, the overlap above the threshold in float64 as the NMS compares -- else TTA_NO_MATCH.
NM_HD float tta_match_value(double overlap, double match_thresh, bool eligible, const float *a, const float *m)
{
    return (eligible && nms_same_class(a, m) && overlap > match_thresh) ? (float)overlap : TTA_NO_MATCH;
}

// is (value v of M row i) a better partner than (value w of M row j)?  The larger overlap, a tie to the lower M rank.
NM_HD bool tta_better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

NM_HD bool tta_finite(float v) { return v - v == 0.f; }

// The fused row of a matched pair: a, aux_a of view A; m (already un-mirrored), aux_m of view M.
NM_HD void tta_fuse(const float *a, const float *aux_a, const float *m, const float *aux_m, float *row, float *aux)
{
    const float sa = a[13], sm = m[13], s = sa + sm;
    const float wa = (s > 0 && tta_finite(s)) ? sa / s : 0.5f, wm = 1.f - wa;
    row[0] = a[0];
    for (int i = 2; i < 9; ++i) row[i] = wa * a[i] + wm * m[i];
    const float ea = aux_a[1], em = aux_m[1];
    const bool sigma = tta_finite(ea) && ea > 0 && tta_finite(em) && em > 0;
    const float ua = sigma ? 1.f / ea : wa, um = sigma ? 1.f / em : wm;
    const float za = a[11], zm = m[11];
    const float z = (ua * za + um * zm) / (ua + um);
    row[9] = z * (wa * a[9] / za + wm * m[9] / zm);
    row[10] = z * (wa * a[10] / za + wm * m[10] / zm);
    row[11] = z;
    const float d = tta_wrap(m[12] - a[12]);
    row[12] = fabsf(d) > TTA_PI / 2 ? (sm > sa ? m[12] : a[12]) : tta_wrap(a[12] + wm * d);
    row[1] = tta_wrap(row[12] - atan2f(row[9], z));
    row[13] = 0.5f * (sa + sm);
    aux[0] = 0.5f * (aux_a[0] + aux_m[0]);
    aux[1] = (ua * ea + um * em) / (ua + um);
    aux[2] = aux_a[2];
    aux[3] = aux_a[3];
}
