// Host side of the deformable convolution's workspace: the geometry, the shape rules that choose a route, the plans that size a
// route's buffers, and ONE map of the caller's workspace -- byte offset and length of every region any DCN kernel is handed.
// dcd_dcn_v2_workspace_bytes is the end of the map's last region; dcd_dcn_v2_forward / _backward (dcn_v2.hip) and the column-buffer
// path (dcn_dense.inc) take every pointer from it.  Host-only, and plain C++17 without hipcc (tests/host/dcn_workspace_host.cpp
// checks bounds, alignment and overlaps on the CPU).  Offsets are relative to the workspace's start, which include/dcd_hip.h asks
// to be 256-byte aligned.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "sgemm_tile.h"
#include "tuning_env.h"

#ifndef __HIPCC__
#define __host__
#endif

namespace {

struct Geom {
    int B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg;
    int Ho, Wo, HoWo, KK, cpg, cpgp, Kp, Cop;  // cpgp: channels/group padded to 32; Kp = dg*KK*cpgp; Cop: Co padded to 32
};

__host__ inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

__host__ inline bool make_geom(Geom &g, int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph,
                               int pw, int dh, int dw, int dg)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || Co <= 0 || kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || ph < 0 ||
        pw < 0 || dh <= 0 || dw <= 0 || dg <= 0 || C % dg)
        return false;
    g.B = B; g.C = C; g.H = H; g.W = W; g.Co = Co; g.kh = kh; g.kw = kw; g.sh = sh; g.sw = sw;
    g.ph = ph; g.pw = pw; g.dh = dh; g.dw = dw; g.dg = dg;
    g.Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) / sh + 1;
    g.Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) / sw + 1;
    if (g.Ho <= 0 || g.Wo <= 0) return false;
    g.HoWo = g.Ho * g.Wo;
    g.KK = kh * kw;
    g.cpg = C / dg;
    g.cpgp = round_up(g.cpg, 32);
    g.Kp = dg * g.KK * g.cpgp;
    g.Cop = round_up(Co, 32);
    // 32-bit index safety for per-image planes
    if ((int64_t)C * H * W >= (1ll << 31) || (int64_t)Co * g.HoWo >= (1ll << 31) ||
        (int64_t)g.Kp * g.Cop >= (1ll << 31) || (int64_t)dg * 2 * g.KK * g.HoWo >= (1ll << 31))
        return false;
    return true;
}

// ---- sizes of the kernels' tiles that the layout depends on (the kernels read the same constants) --------------------------------
constexpr int TL_CH = 8;                    // forward tile kernel: channels per chunk
constexpr int TL_OB = 64;                   // output channels per workgroup (two 32-wide MFMA blocks)
constexpr int TL_W_FLOATS = 9 * TL_OB * TL_CH;            // 4608: [tap][o][h][4 steps]
constexpr int TB_CH = 16;                   // the same in the split-bf16 forward tile kernel
constexpr int TB_W_FLOATS = 9 * 2 * 2 * 64 * 4;          // 9216 dwords (18 432 bf16) per (slice, chunk)
constexpr int INV_CAP = 10;     // list capacity per (cell, tap): offsets below 1 px give at most 9, typically 4
constexpr int DW_CB = 32;                             // tiled grad_weight kernel: channels per block
constexpr int SW_PX = 16;                         // one-pass backward: output pixels per row step
constexpr int SW_CH = 16;                         // channels per wave
constexpr int SW_W_FLOATS = 9 * 16 * 64;          // prepared weights of one 16-channel chunk and one block of 64 outputs
constexpr int SW_DW_FLOATS = 9 * 64 * SW_CH;      // grad_weight partial of one wave: [tap][o][c]
constexpr int SW_PART_FLOATS = SW_DW_FLOATS + 64; // + the wave's grad_bias partial [o] (chunk 0 only)
constexpr int SW_GEMM_T = 128, SW_GEMM_K = 16;    // sgemm_f32.inc's tile edge and k step (checked where the product is launched)

// The DLA-34 shape every workgroup-tiled kernel and the one-pass backward are written for: 3x3, stride 1, pad 1, dilation 1, one
// deformable group, rows of whole float4s, a map of at least 8 x 32.
__host__ inline bool dla_shape(const Geom &g)
{
    return g.kh == 3 && g.kw == 3 && g.sh == 1 && g.sw == 1 && g.ph == 1 && g.pw == 1 && g.dh == 1 && g.dw == 1 && g.dg == 1 &&
           (g.W & 3) == 0 && g.H >= 8 && g.W >= 32;
}

// ---- column-buffer path (dcn_dense.inc) ---------------------------------------------------------------------------------------
// DCD_DCN_DENSE: unset = wide inputs only (Cin >= 256); 0 = never; 1 = every geometry the alignment rules allow (tests).
__host__ inline int dense_mode()
{
    const char *e = dcd_env("DCD_DCN_DENSE");                  // read per call: the tests switch it inside one process
    return !e ? 2 : (atoi(e) == 1 ? 1 : (atoi(e) == 0 ? 0 : 2));
}

// column buffer [B][C*KK][HoWo]; the backward's Tt [B][HoWo][Kp] (Kp >= C*KK: channels padded to 32 per group) shares it
__host__ inline size_t dense_col_floats(const Geom &g) { return (size_t)g.B * g.Kp * g.HoWo; }

// backward = true: the gradient pass; it pays off earlier than the forward (the fused backward needs three kernels with the
// product inside, the dense one shares T between grad_input and the coordinate gradients): measured on 128->128 @ 48x160
// forward 0.35 (dense) vs 0.22 ms (fused), backward 1.20 vs 1.45 ms.
__host__ inline bool dense_ok(const Geom &g, bool backward)
{
    const int mode = dense_mode();
    if (mode == 0) return false;
    const int64_t K9 = (int64_t)g.C * g.KK;
    if ((g.HoWo & 3) || (K9 & 3) || (g.cpg % 16) || g.W < 2 || (int64_t)g.Kp * g.HoWo >= (1ll << 30) ||
        (int64_t)g.Co * g.Kp >= (1ll << 31))
        return false;
    if (dense_col_floats(g) * sizeof(float) > ((size_t)1 << 30)) return false;
    if (mode == 1 || g.C >= 256) return true;
    return backward && g.C >= 128 && g.Co >= 128;
}

struct DensePlan { int fwd_split, fwd_kchunk, dw_split, dw_kchunk; size_t part_floats; };

__host__ inline DensePlan dense_plan(const Geom &g)
{
    DensePlan p;
    const int K9 = g.C * g.KK;
    const int mt = (g.Co + SG_T - 1) / SG_T;
    auto pick = [](int tiles, int K, int min_chunk) {
        int s = (512 + tiles - 1) / tiles;
        const int smax = K / min_chunk > 1 ? K / min_chunk : 1;
        if (s > smax) s = smax;
        if (s < 1) s = 1;
        return s;
    };
    const int ft = mt * ((g.HoWo + SG_T - 1) / SG_T) * g.B;
    p.fwd_split = pick(ft, K9, 512);
    p.fwd_kchunk = ((K9 + p.fwd_split - 1) / p.fwd_split + SG_K - 1) / SG_K * SG_K;
    p.fwd_split = (K9 + p.fwd_kchunk - 1) / p.fwd_kchunk;
    const int wt = mt * ((K9 + SG_T - 1) / SG_T) * g.B;
    p.dw_split = pick(wt, g.HoWo, 256);
    p.dw_kchunk = ((g.HoWo + p.dw_split - 1) / p.dw_split + SG_K - 1) / SG_K * SG_K;
    p.dw_split = (g.HoWo + p.dw_kchunk - 1) / p.dw_kchunk;
    const size_t fp = p.fwd_split > 1 ? (size_t)g.B * p.fwd_split * g.Co * g.HoWo : 0;
    const size_t wp = (size_t)g.B * p.dw_split * g.Co * K9;
    p.part_floats = fp > wp ? fp : wp;
    return p;
}

// ---- one-pass backward (dcn_bwd_sweep.inc) --------------------------------------------------------------------------------------
struct SweepPlan {
    int nck, nstrip, nseg, seg_rows, nv;
    int nslot;                                    // persistent waves of the launch
    int nob;                                      // blocks of 64 outputs (1, 2 or 4); > 1: grad_weight as one product from the col buffer
    int dw_split, dw_kchunk;                      // nob > 1: pixel chunks of that product (per image), summed in a fixed order
    size_t wp_floats, cpart_floats, dw_floats, col_floats;
};

__host__ inline SweepPlan sweep_plan(const Geom &g)
{
    SweepPlan p;
    p.nck = (g.C + SW_CH - 1) / SW_CH;
    p.nstrip = (g.W + SW_PX - 1) / SW_PX;
    // segments: a unit (one wave's sweep over its rows of a strip) pays ~5 rows' worth of ring warm-up and row retirement on top
    // of its rows, and the launch runs ceil(units / 1024 resident waves) units deep: the segment count with the least
    // (depth x (rows + 5)).  Rounds 3-4 kept segments at >= 8 rows, which left the one-image step's <= 48x160 layers at a
    // quarter to a half of the wave slots (one image, 128->64 @ 48x160: 0.155 -> 0.120 ms; 256->128 @ 24x80 0.162 -> 0.111).
    const int64_t base = (int64_t)g.B * p.nstrip * p.nck;
    static const int min_rows = dcd_env("DCD_SWEEP_MIN_ROWS") && atoi(dcd_env("DCD_SWEEP_MIN_ROWS")) > 0 ? atoi(dcd_env("DCD_SWEEP_MIN_ROWS")) : 3;
    int best = 1;
    int64_t best_cost = -1;
    for (int ns = 1; ns <= g.H; ++ns) {
        const int rows = (g.H + ns - 1) / ns;
        if (rows < min_rows && ns > 1) break;
        const int real_ns = (g.H + rows - 1) / rows;
        const int64_t total = base * real_ns;
        const int64_t cost = ((total + 1023) / 1024) * (rows + 5);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = real_ns; }
    }
    p.seg_rows = (g.H + best - 1) / best;
    p.nseg = (g.H + p.seg_rows - 1) / p.seg_rows;
    p.nv = g.B * p.nstrip * p.nseg;
    // persistent waves: about one round of the 1024 wave slots (4 per CU), in whole groups of 8 * nck (a wave keeps its chunk);
    // SW_WAVES divides 8, so whole workgroups too
    const int64_t units = (int64_t)((p.nv + 7) / 8) * 8 * p.nck;
    const int grp = 8 * p.nck;
    int64_t slots = units < 1024 ? units : (1024 / grp) * (int64_t)grp;
    if (slots < grp) slots = grp;
    if (const char *e = dcd_env("DCD_SWEEP_SLOTS")) {             // A/B: 0 = one unit per wave
        const int64_t v_ = atoll(e);
        slots = v_ <= 0 ? units : (v_ / grp > 0 ? v_ / grp : 1) * grp;
    }
    if (slots > units) slots = units;
    p.nslot = (int)slots;
    p.nob = g.Co <= 64 ? 1 : (g.Co <= 128 ? 2 : 4);
    p.wp_floats = (size_t)p.nck * SW_W_FLOATS * p.nob;
    p.cpart_floats = (size_t)p.nck * g.B * 27 * g.HoWo;
    p.dw_split = 1;
    p.dw_kchunk = 0;
    if (p.nob == 1) {
        p.dw_floats = (size_t)p.nslot * SW_PART_FLOATS;
        p.col_floats = 0;
    } else {
        // grad_weight[o][c * 9 + t] = sum_b sum_p dY[b][o][p] col[b][c * 9 + t][p]: per image Co x 9C tiles of 128 x 128, the pixel
        // axis cut so that the launch has ~512 workgroups (chunks of at least 256 pixels)
        const int K9 = g.C * 9;
        const int tiles = ((g.Co + SW_GEMM_T - 1) / SW_GEMM_T) * ((K9 + SW_GEMM_T - 1) / SW_GEMM_T) * g.B;
        int sp = (512 + tiles - 1) / tiles;
        const int smax = g.HoWo / 256 > 1 ? g.HoWo / 256 : 1;
        if (sp > smax) sp = smax;
        if (sp < 1) sp = 1;
        p.dw_kchunk = ((g.HoWo + sp - 1) / sp + SW_GEMM_K - 1) / SW_GEMM_K * SW_GEMM_K;
        p.dw_split = (g.HoWo + p.dw_kchunk - 1) / p.dw_kchunk;
        p.col_floats = (size_t)g.B * K9 * g.HoWo;
        p.dw_floats = (size_t)g.B * p.dw_split * g.Co * K9;
    }
    return p;
}

// DCD_BWD_SWEEP (read per call: the tests switch it inside one process): 0 restores the three-pass backward, 2 leaves the
// layers the dense path takes (Cin >= 256) to it
__host__ inline int sweep_mode()
{
    const char *e = dcd_env("DCD_BWD_SWEEP");
    return !e ? 1 : (atoi(e) == 0 ? 0 : (atoi(e) == 2 ? 2 : 1));
}

__host__ inline bool sweep_ok(const Geom &g)
{
    return sweep_mode() != 0 && dla_shape(g) && g.Co <= 256 && ((int64_t)g.HoWo * 27 & 3) == 0 &&
           (g.Co <= 64 || (((int64_t)g.C * 9 * g.HoWo < (1ll << 29)) && (int64_t)g.B * g.C * 9 * g.HoWo * 4 <= (1ll << 31)));
}

// ---- forward tile route -------------------------------------------------------------------------------------------------------
// DCD_TILE_ROWS=4: forward regions of 4 rows always (read once per process)
__host__ inline int fwd_tile_rows()
{
    static int tile_rows = 0;
    if (tile_rows == 0) {
        const char *e = dcd_env("DCD_TILE_ROWS");
        tile_rows = (e && atoi(e) == 4) ? 4 : 8;
    }
    return tile_rows;
}

struct FwdTilePlan {
    int nz, nchunk;               // slices of 64 outputs, channel chunks
    int tiles_x, rows, regions;   // 32-pixel columns, rows per region (8 when that fills the chip, else 4), regions per image
    int nflag_words;              // region flags (one byte each, whole words) + the far-coordinate counter, zeroed together
    size_t nwl;                   // floats of the tile kernel's weight layout
};

__host__ inline FwdTilePlan fwd_tile_plan(const Geom &g, bool split)
{
    FwdTilePlan t;
    t.nz = (g.Co + TL_OB - 1) / TL_OB;
    t.nchunk = split ? (g.C + TB_CH - 1) / TB_CH : (g.C + TL_CH - 1) / TL_CH;
    t.nwl = (size_t)t.nz * t.nchunk * (split ? TB_W_FLOATS : TL_W_FLOATS);
    t.tiles_x = (g.Wo + 31) / 32;
    const bool rows8 = fwd_tile_rows() == 8 && (int64_t)t.tiles_x * ((g.Ho + 7) / 8) * g.B * t.nz >= 512;
    t.rows = rows8 ? 8 : 4;
    t.regions = t.tiles_x * ((g.Ho + t.rows - 1) / t.rows);
    t.nflag_words = (g.B * t.regions + 3) / 4 + 1;
    return t;
}

// ---- the map ------------------------------------------------------------------------------------------------------------------
// partial grad_weight blocks of the tiled kernel: (channel blocks x output slices x pixel splits) x [64 o][32 c][9]
__host__ inline size_t dw_partial_floats(int Cin, int Cout)
{
    const size_t nb = (size_t)((Cin + DW_CB - 1) / DW_CB) * ((Cout + TL_OB - 1) / TL_OB);
    return (nb > 512 ? nb : 512) * (size_t)(2 * 32 * DW_CB * 9);
}

// tile flags of the tiled grad_input kernel: per (image, 4 x 32 tile of input cells) one byte
__host__ inline size_t tileflag_bytes(const Geom &g) { return ((size_t)g.B * ((g.H + 3) / 4) * ((g.W + 31) / 32) + 255) / 256 * 256; }

// block maxima: per (image, tap segment, 8x8 block of output pixels) one byte
__host__ inline size_t blockmax_bytes(const Geom &g)
{
    return ((size_t)g.B * g.dg * g.KK * ((g.Ho + 7) / 8) * ((g.Wo + 7) / 8) + 255) / 256 * 256;
}

struct Region {
    size_t off = 0, bytes = 0;
    size_t end() const { return off + bytes; }
    template <typename T> T *in(void *workspace) const { return (T *)((char *)workspace + off); }
};

// Backward (and what the forward shares with it), in address order:
//   [Wf | Wb | scalars (256 B) | inverse lists: cnt, idx, w | far-tile flags | far-tile list | grad_weight partials | 256 B unused |
//    block maxima | tile flags] [column buffer (Tt shares it) | split-K partials | 256 B unused]
//   [one-pass backward: prepared weights | grad_offset / grad_mask partial planes | grad_weight partials | col | pad + 256 B unused]
// The second bracket exists when dense_ok(g, true), the third when sweep_ok(g): both depend on per-call environment switches, so
// the map does too.  Forward overlays (the backward's areas are dead then): Wl over [Wf | Wb], or [Wl | Wf9] over them with the
// region flags and the far counter behind the weights; the plain 3x3 route keeps its weights (w9) where Wf is.
struct DcnWorkspace {
    Region wf, wb, scalars, inv_cnt, inv_idx, inv_w, far_flag, far_list, dw_part, blockmax, tileflag;
    Region dense_col, dense_part;
    Region sw_wp, sw_cpart, sw_dwpart, sw_col;
    Region fwd_wl, fwd_wf9, fwd_flags, fwd_far_count, fwd_w9;
    size_t base_end = 0, dense_end = 0, total = 0;     // ends of the three brackets; total is what the caller must provide
    bool has_dense = false, has_sweep = false, has_tile = false;
    DensePlan dense;
    SweepPlan sweep;
    FwdTilePlan tile;
};

struct RegionCursor {
    size_t at = 0;
    void take(Region &r, size_t bytes) { r.off = at; r.bytes = bytes; at += bytes; }
    void align256() { at = (at + 255) / 256 * 256; }
};

// first bracket + column-buffer bracket (needed by both passes)
__host__ inline void map_shared(DcnWorkspace &m, const Geom &g, RegionCursor &c)
{
    const size_t nw = (size_t)g.Kp * g.Cop;
    const size_t cells = (size_t)g.B * g.dg * g.KK * g.H * g.W;
    const size_t ntile = (size_t)g.B * ((g.HoWo + 31) / 32);
    c.take(m.wf, nw * sizeof(float));
    c.take(m.wb, nw * sizeof(float));
    c.take(m.scalars, 256);
    c.take(m.inv_cnt, (cells + 255) / 256 * 256);
    c.take(m.inv_idx, cells * INV_CAP * sizeof(int));
    c.take(m.inv_w, cells * INV_CAP * sizeof(float));
    c.align256();
    c.take(m.far_flag, (ntile + 255) / 256 * 256);
    c.take(m.far_list, (ntile + 63) / 64 * 64 * sizeof(int));
    c.take(m.dw_part, dw_partial_floats(g.C, g.Co) * sizeof(float));
    c.at += 256;                  // the size formula's allowance for the round-up above, which the round-up has taken already
    c.take(m.blockmax, blockmax_bytes(g));
    c.take(m.tileflag, tileflag_bytes(g));
    m.base_end = c.at;
    m.has_dense = dense_ok(g, true);
    if (m.has_dense) {
        m.dense = dense_plan(g);
        c.take(m.dense_col, dense_col_floats(g) * sizeof(float));
        c.take(m.dense_part, m.dense.part_floats * sizeof(float));
        c.at += 256;
    }
    m.dense_end = c.at;
}

__host__ inline DcnWorkspace dcn_workspace_backward(const Geom &g)
{
    DcnWorkspace m;
    RegionCursor c;
    map_shared(m, g, c);
    m.has_sweep = sweep_ok(g);
    if (m.has_sweep) {
        m.sweep = sweep_plan(g);
        c.take(m.sw_wp, m.sweep.wp_floats * sizeof(float));
        c.take(m.sw_cpart, m.sweep.cpart_floats * sizeof(float));
        c.take(m.sw_dwpart, m.sweep.dw_floats * sizeof(float));
        c.take(m.sw_col, m.sweep.col_floats * sizeof(float));
        c.at = m.dense_end + (c.at - m.dense_end + 255) / 256 * 256 + 256;
    }
    m.total = c.at;
    return m;
}

// split: the tile kernel's weights in its split-bf16 layout (DCD_PREC_BF16X3 / DCD_PREC_BF16)
__host__ inline DcnWorkspace dcn_workspace_forward(const Geom &g, bool split)
{
    DcnWorkspace m;
    RegionCursor c;
    map_shared(m, g, c);
    m.total = c.at;               // (of the forward's own needs; the caller allocates dcd_dcn_v2_workspace_bytes for both passes)
    const size_t n9 = (size_t)g.C * 9 * g.Cop;
    m.fwd_w9.bytes = n9 * sizeof(float);
    m.has_tile = dla_shape(g) && dcd_env("DCD_NO_TILE") == nullptr;
    if (m.has_tile) {
        m.tile = fwd_tile_plan(g, split);
        m.fwd_wl.bytes = m.tile.nwl * sizeof(float);
        m.fwd_wf9.off = m.wb.off;
        m.fwd_wf9.bytes = n9 * sizeof(float);
        m.fwd_flags.off = m.wb.end();
        m.fwd_flags.bytes = (size_t)(m.tile.nflag_words - 1) * 4;
        m.fwd_far_count.off = m.fwd_flags.end();
        m.fwd_far_count.bytes = 4;
    }
    return m;
}

}  // namespace
