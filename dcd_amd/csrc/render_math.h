// The raster rule of the detection renderer (include/dcd_hip.h, dcd_render_detections; DESIGN.md 6d "Rendering").
//
// Written once for two compilations: render.hip runs it on the device, tests/host/host_render.cpp runs the same functions in
// plain loops on the host (test infrastructure; the library has no host path).  All geometry is fp32 and nothing is contracted
// into a fused multiply-add (the pragma below; the host build adds -ffp-contract=off), so the two builds differ by the rounding
// of sinf / cosf and of the division only.  Everything after the truncation to pixels is integer arithmetic and exact.
//
// THE RULE.  The picture of image b (frame w x h) is canvas[b, :h, :w + h]: panel 0, columns [0, w), is the frame; panel 1,
// columns [w, w + h), is the bird's-eye square on background 230; every other byte of the canvas is 0.  A primitive belongs
// to one panel, its coordinates are relative to that panel's left edge, and it writes only inside the panel.
//   float -> pixel   truncation toward zero; a primitive with a non-finite coordinate or one of magnitude >= 2^24 is skipped whole
//   segment          ends ordered so that the major coordinate (larger of |dx|, |dy|; x on a tie) increases; for every major
//                    step t in [0, D] the minor coordinate is m0 + floor((2 t dm + D) / (2 D)) (a true floor, 64-bit); a point
//                    is one step; thickness T in 1 .. 4 stamps T x T pixels with offsets -(T - 1) / 2 .. T / 2 at every step
//   glyph            5 x 7 bits from RD_FONT at a top-left corner
//   order            the primitive with the greatest `order` wins a pixel (then the later table entry); no blending
// The table of an image has a FIXED layout (rd_slots): a primitive that is not drawn leaves its slot with kind -1.
//   ground truth slot m:       17 m + [0, 12) box edges T1 | [12, 16) bird's-eye footprint T2 | 16 heading edge 0-1 T4
//   detection drawn j-th (rank K - 1 - j, so rank 0 is last and on top), at 17 M + j (28 + nk):
//                              [0, 4) 2-D box T1 | [4, 18) 12 edges + diagonals 0-5, 1-4 T1 | nk key points T3 |
//                              4 footprint T2 | heading T4 | 5 glyphs "C0.87"
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __clang__
#pragma clang fp contract(off)
#endif

#ifdef __HIPCC__
#define RD_HD __host__ __device__ __forceinline__
#else
#define RD_HD inline
#endif

#define RD_ENTRY 12        // int32 per table entry: panel, kind, x0, y0, x1, y1, T, r, g, b, order, glyph
#define RD_MAX_ENTRIES 8192
#define RD_MAX_ORDER (1 << 18)
#define RD_GT_SLOTS 17
#define RD_DET_SLOTS 28    // + nk key points
#define RD_NEAR 0.125f
#define RD_LIMIT 16777216.f
#define RD_BACKGROUND 230
#define RD_KIND_NONE (-1)
#define RD_KIND_SEGMENT 0
#define RD_KIND_GLYPH 1

// glyphs 0-9, '.', 'C', 'P', 'Y', '?': seven rows of five bits, the left pixel in bit 4
#define RD_GLYPHS 15
#define RD_FONT_ROWS                                                                                                              \
    {                                                                                                                             \
        {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E},                                   \
            {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F}, {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E},                               \
            {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},                               \
            {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08},                               \
            {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E}, {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C},                               \
            {0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C}, {0x0E, 0x11, 0x10, 0x10, 0x10, 0x11, 0x0E},                               \
            {0x1E, 0x11, 0x11, 0x1E, 0x10, 0x10, 0x10}, {0x11, 0x11, 0x11, 0x0A, 0x04, 0x04, 0x04},                               \
            {0x0E, 0x11, 0x01, 0x02, 0x04, 0x00, 0x04},                                                                           \
    }

RD_HD int rd_glyph_row(int glyph, int row)
{
    const unsigned char font[RD_GLYPHS][7] = RD_FONT_ROWS;
    return font[glyph][row];
}

// the reference's keypoint_colors (DGDE/engine/visualize_infer.py:18-21)
RD_HD void rd_keypoint_color(int k, int *rgb)
{
    const unsigned char c[16][3] = {{128, 64, 128}, {244, 35, 232}, {70, 70, 70},   {102, 102, 156}, {190, 153, 153}, {153, 153, 153},
                                    {250, 170, 30}, {220, 220, 0},  {107, 142, 35}, {255, 0, 0},     {0, 0, 142},     {0, 0, 70},
                                    {152, 251, 152}, {0, 130, 180}, {220, 20, 60},  {0, 60, 100}};
    for (int i = 0; i < 3; ++i) rgb[i] = c[k % 16][i];
}

struct RdArgs {
    int B, K, nk, M;                    // nk = 0: no key points; M = 0: no ground truth
    float det_threshold, vis_threshold;
    const float *rows, *aux, *k2, *table;
    const float *gt_dims, *gt_locs, *gt_rotys;
    const uint8_t *gt_mask;
    const int64_t *recs;                // (B, 5): byte offset, row pitch, height, width, flip -- the head of the staged buffer
    uint64_t staged_bytes;
    int in_h, in_w;
};

RD_HD int rd_slots(int M, int K, int nk) { return RD_GT_SLOTS * M + K * (RD_DET_SLOTS + nk); }

// The frame of image b as the raster may read it: false (an all-zero picture) when the record does not describe w x h pixels
// inside the staged buffer and the canvas.
RD_HD bool rd_frame(const int64_t *recs, uint64_t staged_bytes, int b, int in_h, int in_w, int *w, int *h, int64_t *off,
                    int64_t *pitch, int *flip)
{
    const int64_t *r = recs + (int64_t)b * 5;
    *w = *h = 0;
    *off = *pitch = 0;
    *flip = 0;
    if (r[2] < 1 || r[2] > in_h || r[3] < 1 || r[3] > in_w || r[0] < 0 || r[1] < 3 * r[3] || r[1] > (int64_t)1 << 32) return false;
    if ((uint64_t)r[0] > staged_bytes || (uint64_t)(r[1] * (r[2] - 1) + 3 * r[3]) > staged_bytes - (uint64_t)r[0]) return false;
    *off = r[0];
    *pitch = r[1];
    *h = (int)r[2];
    *w = (int)r[3];
    *flip = r[4] != 0;
    return true;
}

RD_HD void rd_none(int *e, float *f)
{
    for (int i = 0; i < RD_ENTRY; ++i) e[i] = 0;
    e[1] = RD_KIND_NONE;
    if (f) f[0] = f[1] = f[2] = f[3] = 0.f;
}

RD_HD bool rd_pixel(float v, int *out)
{
    if (!(fabsf(v) < RD_LIMIT)) return false;                          // (a NaN fails the comparison)
    *out = (int)v;
    return true;
}

RD_HD void rd_segment(int *e, float *f, int order, int panel, float x0, float y0, float x1, float y1, int T, const int *rgb)
{
    rd_none(e, f);
    if (f) {
        f[0] = x0;
        f[1] = y0;
        f[2] = x1;
        f[3] = y1;
    }
    int p[4];
    if (!rd_pixel(x0, p) || !rd_pixel(y0, p + 1) || !rd_pixel(x1, p + 2) || !rd_pixel(y1, p + 3)) return;
    e[0] = panel;
    e[1] = RD_KIND_SEGMENT;
    for (int i = 0; i < 4; ++i) e[2 + i] = p[i];
    e[6] = T;
    for (int i = 0; i < 3; ++i) e[7 + i] = rgb[i];
    e[10] = order;
}

// box3d_to_corners (visualize_infer.py:56-72): bottom centre `loc`, yaw `ry`; corner i at c[3 i]
RD_HD void rd_corners(float h, float w, float l, const float *loc, float ry, float *c)
{
    const float xs[8] = {l / 2.f, l / 2.f, -l / 2.f, -l / 2.f, l / 2.f, l / 2.f, -l / 2.f, -l / 2.f};
    const float ys[8] = {0.f, 0.f, 0.f, 0.f, -h, -h, -h, -h};
    const float zs[8] = {w / 2.f, -w / 2.f, -w / 2.f, w / 2.f, w / 2.f, -w / 2.f, -w / 2.f, w / 2.f};
    const float cs = cosf(ry), sn = sinf(ry);
    for (int i = 0; i < 8; ++i) {
        c[3 * i] = (cs * xs[i] + sn * zs[i]) + loc[0];
        c[3 * i + 1] = ys[i] + loc[1];
        c[3 * i + 2] = (-sn * xs[i] + cs * zs[i]) + loc[2];
    }
}

// one 3-D edge, clipped against z = RD_NEAR and projected with P (3 x 4, row-major), to an image-panel segment
RD_HD void rd_edge(int *e, float *f, int order, const float *A, const float *B, const float *P, const int *rgb)
{
    float a[3] = {A[0], A[1], A[2]}, b[3] = {B[0], B[1], B[2]};
    const bool near_a = a[2] < RD_NEAR, near_b = b[2] < RD_NEAR;
    if (near_a && near_b) {
        rd_none(e, f);
        return;
    }
    if (near_a || near_b) {
        float *in = near_a ? a : b;
        const float *out = near_a ? b : a;
        const float t = (RD_NEAR - in[2]) / (out[2] - in[2]);
        in[0] = in[0] + t * (out[0] - in[0]);
        in[1] = in[1] + t * (out[1] - in[1]);
        in[2] = RD_NEAR;
    }
    const float ua = ((P[0] * a[0] + P[2] * a[2]) + P[3]) / (a[2] + P[11]), va = ((P[5] * a[1] + P[6] * a[2]) + P[7]) / (a[2] + P[11]);
    const float ub = ((P[0] * b[0] + P[2] * b[2]) + P[3]) / (b[2] + P[11]), vb = ((P[5] * b[1] + P[6] * b[2]) + P[7]) / (b[2] + P[11]);
    rd_segment(e, f, order, 0, ua, va, ub, vb, 1, rgb);
}

// draw_bev_box3d (kitti_utils.py:872-897) with world_size 64 and out_size h: footprint 0-1-2-3 T2, heading 0-1 T4
RD_HD void rd_bev(int *e, float *f, int order, const float *c, float hf, const int *rgb)
{
    float bx[4], by[4];
    for (int i = 0; i < 4; ++i) {
        bx[i] = (c[3 * i] + 32.f) * hf / 64.f;
        by[i] = (64.f - c[3 * i + 2]) * hf / 64.f;
    }
    for (int i = 0; i < 4; ++i) {
        const int j = (i + 1) % 4;
        rd_segment(e + i * RD_ENTRY, f ? f + 4 * i : nullptr, order + i, 1, bx[i], by[i], bx[j], by[j], 2, rgb);
    }
    rd_segment(e + 4 * RD_ENTRY, f ? f + 16 : nullptr, order + 4, 1, bx[0], by[0], bx[1], by[1], 4, rgb);
}

// the 12 edges in draw_projected_box3d's order (kitti_utils.py:782-792), then the front-face diagonals
RD_HD void rd_box_edge(int i, int *p, int *q)
{
    if (i >= 12) {
        *p = i - 12;
        *q = 17 - i;
        return;
    }
    const int k = i / 3, r = i % 3;
    *p = r == 1 ? k + 4 : k;
    *q = r == 0 ? (k + 1) % 4 : (r == 1 ? (k + 1) % 4 + 4 : k + 4);
}

// Object `obj` of image b: obj < M a ground-truth slot, else the detection drawn (obj - M)-th.  ent / ends: the image's table
// (rd_slots entries) and float ends (4 per entry, or null).  w, h: the frame.  Returns one past the last slot it drew, or 0.
RD_HD int rd_object(const RdArgs &a, int b, int obj, int h, int *ent, float *ends)
{
    const float *P = a.table + (int64_t)b * 16 + 4;
    const float hf = (float)h;
    float c[24];
    int last = 0;
    if (obj < a.M) {
        const int base = RD_GT_SLOTS * obj;
        const int64_t g = (int64_t)b * a.M + obj;
        int *e = ent + (int64_t)base * RD_ENTRY;
        float *f = ends ? ends + (int64_t)base * 4 : nullptr;
        if (!a.gt_mask[g]) {
            for (int i = 0; i < RD_GT_SLOTS; ++i) rd_none(e + i * RD_ENTRY, f ? f + 4 * i : nullptr);
            return 0;
        }
        const int rgb[3] = {244, 96, 108};
        const float *d = a.gt_dims + g * 3, *t = a.gt_locs + g * 3;          // (l, h, w), the centre
        const float loc[3] = {t[0], t[1] + d[1] / 2.f, t[2]};
        rd_corners(d[1], d[2], d[0], loc, a.gt_rotys[g], c);
        for (int i = 0; i < 12; ++i) {
            int p, q;
            rd_box_edge(i, &p, &q);
            rd_edge(e + i * RD_ENTRY, f ? f + 4 * i : nullptr, base + i, c + 3 * p, c + 3 * q, P, rgb);
        }
        rd_bev(e + 12 * RD_ENTRY, f ? f + 48 : nullptr, base + 12, c, hf, rgb);
        for (int i = 0; i < RD_GT_SLOTS; ++i)
            if (e[i * RD_ENTRY + 1] != RD_KIND_NONE) last = base + i + 1;
        return last;
    }
    const int j = obj - a.M, per = RD_DET_SLOTS + a.nk, base = RD_GT_SLOTS * a.M + j * per;
    const int64_t n = (int64_t)b * a.K + (a.K - 1 - j);
    int *e = ent + (int64_t)base * RD_ENTRY;
    float *f = ends ? ends + (int64_t)base * 4 : nullptr;
    const float *row = a.rows + n * 14;
    if (!(a.aux[n * 4] >= a.det_threshold) || !(row[13] > a.vis_threshold)) {
        for (int i = 0; i < per; ++i) rd_none(e + i * RD_ENTRY, f ? f + 4 * i : nullptr);
        return 0;
    }
    const int green[3] = {0, 255, 0}, pred[3] = {25, 202, 173};
    const float x0 = row[2], y0 = row[3], x1 = row[4], y1 = row[5];
    const float rect[4][4] = {{x0, y0, x1, y0}, {x1, y0, x1, y1}, {x1, y1, x0, y1}, {x0, y1, x0, y0}};
    for (int i = 0; i < 4; ++i)
        rd_segment(e + i * RD_ENTRY, f ? f + 4 * i : nullptr, base + i, 0, rect[i][0], rect[i][1], rect[i][2], rect[i][3], 1, green);
    rd_corners(row[6], row[7], row[8], row + 9, row[12], c);
    for (int i = 0; i < 14; ++i) {
        int p, q;
        rd_box_edge(i, &p, &q);
        rd_edge(e + (4 + i) * RD_ENTRY, f ? f + 4 * (4 + i) : nullptr, base + 4 + i, c + 3 * p, c + 3 * q, P, pred);
    }
    for (int k = 0; k < a.nk; ++k) {                                      // the decode's normalisation undone: u = x' f_u + c_u
        const float *kp = a.k2 + (n * a.nk + k) * 2;
        const float u = kp[0] * P[0] + P[2], v = kp[1] * P[5] + P[6];
        int rgb[3];
        rd_keypoint_color(k, rgb);
        rd_segment(e + (18 + k) * RD_ENTRY, f ? f + 4 * (18 + k) : nullptr, base + 18 + k, 0, u, v, u, v, 3, rgb);
    }
    const int s = 18 + a.nk;
    rd_bev(e + s * RD_ENTRY, f ? f + 4 * s : nullptr, base + s, c, hf, pred);
    {                                                                     // the label "C0.87" above the 2-D box
        const float sc = row[13];
        int cents = 0, lx, ly;
        if (sc >= 1.f && sc < INFINITY) cents = 99;                       // (every score from 0.995 up prints 0.99)
        else if (sc >= 0.f && sc < 1.f) cents = (int)(sc * 100.f + 0.5f);
        cents = cents > 99 ? 99 : cents;
        const bool known = row[0] >= 0.f && row[0] < 3.f;                 // the class is the integer part of column 0
        const int letter = known ? 11 + (int)row[0] : 14;
        const int glyphs[5] = {letter, 0, 10, cents / 10, cents % 10};
        const bool ok = rd_pixel(x0, &lx) && rd_pixel(y0, &ly);
        for (int i = 0; i < 5; ++i) {
            int *g = e + (s + 5 + i) * RD_ENTRY;
            float *gf = f ? f + 4 * (s + 5 + i) : nullptr;
            rd_none(g, gf);
            if (gf) {
                gf[0] = x0;
                gf[1] = y0;
            }
            if (!ok) continue;
            g[0] = 0;
            g[1] = RD_KIND_GLYPH;
            g[2] = lx + 6 * i;
            g[3] = ly - 8;
            g[4] = g[2] + 4;
            g[5] = g[3] + 6;
            g[6] = 1;
            for (int q = 0; q < 3; ++q) g[7 + q] = green[q];
            g[10] = base + s + 5 + i;
            g[11] = glyphs[i];
        }
    }
    for (int i = 0; i < per; ++i)
        if (e[i * RD_ENTRY + 1] != RD_KIND_NONE) last = base + i + 1;
    return last;
}

// ---- the raster ------------------------------------------------------------------------------------------------------------
// an entry the raster draws: anything else (a caller's table may hold anything) is passed over
RD_HD bool rd_entry_ok(const int *e)
{
    if (e[1] != RD_KIND_SEGMENT && e[1] != RD_KIND_GLYPH) return false;
    if (e[0] != 0 && e[0] != 1) return false;
    for (int i = 2; i < 6; ++i)
        if (e[i] <= -(1 << 24) || e[i] >= (1 << 24)) return false;
    if (e[10] < 0 || e[10] >= RD_MAX_ORDER) return false;
    if (e[1] == RD_KIND_SEGMENT) return e[6] >= 1 && e[6] <= 4;
    return e[11] >= 0 && e[11] < RD_GLYPHS;
}

RD_HD int64_t rd_floordiv(int64_t a, int64_t b)                          // b > 0
{
    int64_t q = a / b;
    if (a % b < 0) --q;
    return q;
}

// Every pixel of entry e (rd_entry_ok) inside the region [rx0, rx1] x [ry0, ry1] of its panel (inclusive, panel coordinates):
// plot(x, y).  The range of steps is cut to the region in closed form, so a far end costs nothing.
template <class Plot>
RD_HD void rd_raster(const int *e, int rx0, int ry0, int rx1, int ry1, Plot plot)
{
    if (rx0 > rx1 || ry0 > ry1) return;
    if (e[1] == RD_KIND_GLYPH) {
        if (e[2] > rx1 || e[2] + 4 < rx0 || e[3] > ry1 || e[3] + 6 < ry0) return;
        for (int gy = 0; gy < 7; ++gy) {
            const int y = e[3] + gy, bits = rd_glyph_row(e[11], gy);
            if (y < ry0 || y > ry1) continue;
            for (int gx = 0; gx < 5; ++gx) {
                const int x = e[2] + gx;
                if (((bits >> (4 - gx)) & 1) && x >= rx0 && x <= rx1) plot(x, y);
            }
        }
        return;
    }
    const int dx = e[4] - e[2], dy = e[5] - e[3];
    const bool xmajor = (dx < 0 ? -dx : dx) >= (dy < 0 ? -dy : dy);
    int M0 = xmajor ? e[2] : e[3], m0 = xmajor ? e[3] : e[2], M1 = xmajor ? e[4] : e[5], m1 = xmajor ? e[5] : e[4];
    if (M1 < M0) {
        int t = M0;
        M0 = M1;
        M1 = t;
        t = m0;
        m0 = m1;
        m1 = t;
    }
    const int T = e[6], omin = -((T - 1) / 2), omax = T / 2;
    const int RA = xmajor ? rx0 : ry0, RB = xmajor ? rx1 : ry1, SA = xmajor ? ry0 : rx0, SB = xmajor ? ry1 : rx1;
    const int lo = m0 < m1 ? m0 : m1, hi = m0 < m1 ? m1 : m0;
    if (lo + omin > SB || hi + omax < SA) return;
    const int64_t D = (int64_t)M1 - M0, dm = (int64_t)m1 - m0;
    int64_t t0 = (int64_t)RA - omax - M0, t1 = (int64_t)RB - omin - M0;
    t0 = t0 < 0 ? 0 : t0;
    t1 = t1 > D ? D : t1;
    for (int64_t t = t0; t <= t1; ++t) {
        const int Mj = M0 + (int)t;
        const int m = D ? m0 + (int)rd_floordiv(2 * t * dm + D, 2 * D) : m0;
        if (m + omin > SB || m + omax < SA) continue;
        for (int oa = omin; oa <= omax; ++oa) {
            const int pM = Mj + oa;
            if (pM < RA || pM > RB) continue;
            for (int ob = omin; ob <= omax; ++ob) {
                const int pm = m + ob;
                if (pm < SA || pm > SB) continue;
                if (xmajor) plot(pM, pm);
                else plot(pm, pM);
            }
        }
    }
}

// the key the raster keeps per pixel: the greatest wins; 0 is "nothing drawn"
RD_HD uint32_t rd_key(const int *e, int index) { return ((uint32_t)(e[10] + 1) << 13) | (uint32_t)index; }
