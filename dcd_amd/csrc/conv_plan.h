// Host side of the convolutions in conv.hip, as far as it is arithmetic on shapes: the chunk widths the kernels share with it, the
// direction of a call, the plans of the three 3x3 / stride 1 forms, the shape rule of each family and the partitions of the
// weight-gradient kernels.  Every workspace size is a member here (ConvPlan::part_bytes, *Partition::bytes) that both the
// *_workspace_bytes function and the run function read.  Host-only, plain C++17 without hipcc: tests/host/conv_plan_host.cpp
// checks on the CPU that what a run needs never exceeds what is advertised.  The CU count is a parameter (conv.hip asks the device).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "tuning_env.h"

namespace {

// contraction channels per chunk (the kernels stage one chunk per barrier)
constexpr int WN_CH = 8;                          // fp32 Winograd form
constexpr int WS_CH = 16;                         // split-bf16 Winograd form
constexpr int DC_CH = 16;                         // direct one-product form (conv_direct_bf16.inc)

// ---- the direction of a call -------------------------------------------------------------------------------------------------
// Forward contracts over Cin and produces Cout; backward-data the other way round.  A workgroup produces nb blocks of 32 channels
// (ks = 32 nb of them): 2, or 1 for layers of at most 32 outputs (DCN's 27-channel offset convs).
struct ConvDir {
    int Cc, Kk;                                   // contraction channels, produced channels
    int nb, ks, nchunk, nz;                       // nchunk chunks of `ch` contraction channels, nz output slices of ks channels
    // the transformed weights of this direction: the kernels' weight slab per (output slice, chunk)
    size_t wino_floats() const { return (size_t)nchunk * nz * 16 * ks * WN_CH; }           // fp32 form (ch = WN_CH)
    size_t split_dwords() const { return (size_t)nchunk * nz * 16 * nb * 2 * 256; }        // split-bf16 form (ch = WS_CH)
};

inline ConvDir conv_dir(int Cin, int Cout, int backward_data, int ch)
{
    const int Cc = backward_data ? Cout : Cin, Kk = backward_data ? Cin : Cout;
    const int nb = Kk <= 32 ? 1 : 2, ks = 32 * nb;
    return {Cc, Kk, nb, ks, (Cc + ch - 1) / ch, (Kk + ks - 1) / ks};
}

// dcd_conv3x3 transforms the weights into the head of its workspace; the advertised size does not know the direction, so it
// reserves the larger channel count both ways at 64 outputs per slice (never less than either direction's wino_floats()).
inline size_t wino_floats_bound(int Cin, int Cout)
{
    const int cmax = Cin > Cout ? Cin : Cout;
    return (size_t)((cmax + WN_CH - 1) / WN_CH) * ((cmax + 63) / 64) * 16 * 64 * WN_CH;
}

inline bool conv_sizes_ok(int B, int Cin, int H, int W, int Cout) { return B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0; }

// ---- 3x3 / stride 1: the three forms -----------------------------------------------------------------------------------------
enum ConvForm { CONV_F32, CONV_SPLIT, CONV_DIRECT };

// Region geometry and contraction split of one call.
struct ConvPlan {
    ConvForm form;
    int geom;          // CONV_F32: 0 = 8 x 32 px regions, 1 = 12 x 20 px.  CONV_DIRECT: rows per wave P | region width in 32 px << 4
    int nb;            // 32-channel output blocks per workgroup
    int tiles_x, tiles_y, nchunk, nz, ksplit;
    size_t img;        // floats of the produced image (B, Kk, H, W)
    // splits 1 .. ksplit-1 write partial images that wino_sum_partials adds to the output
    size_t part_bytes() const { return (size_t)(ksplit - 1) * img * sizeof(float); }
};

inline void conv_region(ConvForm form, int geom, int &rows, int &cols)
{
    if (form == CONV_DIRECT) { rows = 4 * (geom & 15); cols = 32 * (geom >> 4); }
    else if (form == CONV_F32 && geom == 1) { rows = 12; cols = 20; }
    else { rows = 8; cols = 32; }
}

inline ConvPlan with_geom(ConvPlan p, int g, int H, int W)
{
    int rows, cols;
    conv_region(p.form, g, rows, cols);
    p.geom = g;
    p.tiles_x = (W + cols - 1) / cols;
    p.tiles_y = (H + rows - 1) / rows;
    return p;
}

// the unsplit plan of a form at region shape g, and the workgroups it launches
inline ConvPlan conv_plan_unsplit(ConvForm form, int g, int ch, int B, int Cc, int H, int W, int Kk)
{
    const ConvDir d = conv_dir(Cc, Kk, 0, ch);
    ConvPlan p{};
    p.form = form;
    p.nb = d.nb; p.nchunk = d.nchunk; p.nz = d.nz;
    p.ksplit = 1;
    p.img = (size_t)B * Kk * H * W;
    return with_geom(p, g, H, W);
}

inline int64_t conv_workgroups(const ConvPlan &p, int B) { return (int64_t)p.tiles_x * p.tiles_y * B * p.nz; }

// fp32 form.  The workgroup holds 103 KB of LDS and 8 waves with 128 accumulator registers each, so exactly one sits on a CU:
// time ~ rounds of `cus` workgroups x chunks per workgroup.
inline ConvPlan conv_plan(int cus, int B, int Cc, int H, int W, int Kk)
{
    // split the contraction while the launch leaves CUs idle and a split keeps at least 4 chunks (its output transform
    // and the partial image it writes are not free; 4 vs 8: one image per GPU, 256 -> 256 @ 24x80 39 -> 32 us)
    static const int min_chunks = dcd_env("DCD_CONV_MINCHUNK") ? atoi(dcd_env("DCD_CONV_MINCHUNK")) : 4;
    ConvPlan best{};
    int64_t best_cost = -1;
    for (int g = 0; g < 2; ++g) {
        ConvPlan p = conv_plan_unsplit(CONV_F32, g, WN_CH, B, Cc, H, W, Kk);
        const int64_t wgs = conv_workgroups(p, B);
        int ks = 1;
        while (ks < 8 && wgs * (ks * 2) <= cus && p.nchunk / (ks * 2) >= min_chunks) ks *= 2;
        p.ksplit = ks;
        const int64_t rounds = (wgs * ks + cus - 1) / cus;
        const int64_t cost = rounds * ((p.nchunk + ks - 1) / ks + 2) * (g == 0 ? 16 : 17);     // 12x20: 30 of 32 lanes, more halo
        if (best_cost < 0 || cost < best_cost) {
            best_cost = cost;
            best = p;
        }
    }
    return best;
}

// split-bf16 form: 8 x 32 px regions, chunks of 16 channels; the contraction is split while CUs would idle and a split keeps two chunks
inline ConvPlan conv_plan_split(int cus, int B, int Cc, int H, int W, int Kk)
{
    ConvPlan p = conv_plan_unsplit(CONV_SPLIT, 0, WS_CH, B, Cc, H, W, Kk);
    const int64_t wgs = conv_workgroups(p, B);
    while (p.ksplit < 8 && wgs * (p.ksplit * 2) <= cus && p.nchunk / (p.ksplit * 2) >= 2) p.ksplit *= 2;
    return p;
}

// direct one-product form (conv_direct_bf16.inc): rows per wave P = 2, i.e. 8 x 32 px regions; DCD_CONV_DIRECT_P=4 pins 16 x 32 px
// (one workgroup per CU), DCD_CONV_DIRECT_WX=2 pins 8 x 64 px (eight waves; a third less L2 traffic for the column halo).
inline ConvPlan conv_plan_direct(int cus, int B, int Cc, int H, int W, int Kk)
{
    static const int P = dcd_env("DCD_CONV_DIRECT_P") && atoi(dcd_env("DCD_CONV_DIRECT_P")) == 4 ? 4 : 2;
    static const int wx = P == 2 && dcd_env("DCD_CONV_DIRECT_WX") && atoi(dcd_env("DCD_CONV_DIRECT_WX")) == 2 ? 2 : 1;
    // Three workgroups share a CU.  A long contraction is split while slots would stay empty and a split keeps 16 chunks
    // (256 -> 256 @ 24x80 x 8: 46.5 us split in two or not, and the split pays a wino_sum_partials launch); a launch of less
    // than 1.5 workgroups per CU (one or two images per GPU) is split down to two chunks -- there a workgroup's chunks are a
    // serial chain of load latencies (256 -> 256 @ 24x80 x 1: 27.7 us unsplit against the Winograd form's 14.5).
    static const int min_chunks = dcd_env("DCD_CONV_DIRECT_MINCHUNK") ? atoi(dcd_env("DCD_CONV_DIRECT_MINCHUNK")) : 16;
    ConvPlan p = conv_plan_unsplit(CONV_DIRECT, P | (wx << 4), DC_CH, B, Cc, H, W, Kk);
    const int64_t wgs = conv_workgroups(p, B);
    while (p.ksplit < 8) {
        const int64_t next = wgs * p.ksplit * 2;
        const int left = p.nchunk / (p.ksplit * 2);
        const bool fill = next <= 3 * cus && left >= min_chunks;
        const bool small = 2 * next <= 3 * cus && left >= 2;
        if (!fill && !small) break;
        p.ksplit *= 2;
    }
    return p;
}

inline ConvPlan conv_plan_of(ConvForm form, int cus, int B, int Cc, int H, int W, int Kk)
{
    return form == CONV_F32 ? conv_plan(cus, B, Cc, H, W, Kk)
         : form == CONV_SPLIT ? conv_plan_split(cus, B, Cc, H, W, Kk) : conv_plan_direct(cus, B, Cc, H, W, Kk);
}

// the partial images of a split contraction, whichever direction the call takes
inline size_t conv_part_bytes_either(ConvForm form, int cus, int B, int Cin, int H, int W, int Cout)
{
    const size_t pf = conv_plan_of(form, cus, B, Cin, H, W, Cout).part_bytes(), pd = conv_plan_of(form, cus, B, Cout, H, W, Cin).part_bytes();
    return pf > pd ? pf : pd;
}

// The shape rule of the three forms' run functions (and of dcd_conv3x3_wrw, which takes CONV_F32's).  The forms differ in two
// places, kept as they were:
//                       fp32 / split-bf16 (Winograd)                  direct
//   rows                H even.  wino_wrw3x3_f32 needs it (it reads     any H: conv3x3_direct_bf16 tests every output row
//                       both dY rows of a strip untested); the         (orow >= H)
//                       forward kernels test each row of a 2 x 2
//                       tile (orow0 + 1 < H), so for them it only
//                       keeps forward and weight gradient in step
//   32-bit offsets      max(Cin, Cout) H W < 2^31, whichever the        (Cc + 16) H W < 2^29: the loads' whole byte offset
//                       direction (the kernels' own int offsets        sits in a 32-bit buffer-load VGPR.  Kk H W < 2^31:
//                       span one chunk of one image, the stores'       a margin too (the stores' offsets are size_t)
//                       are size_t: a wide margin)
// Common to all: positive sizes, and W a multiple of 4 (float4 groups in the window staging and in wino_sum_partials).
inline bool conv3x3_shape_ok(ConvForm form, int B, int Cin, int H, int W, int Cout, int backward_data)
{
    if (!conv_sizes_ok(B, Cin, H, W, Cout) || (W & 3)) return false;
    const int64_t HW = (int64_t)H * W;
    if (form != CONV_DIRECT) return !(H & 1) && (Cin > Cout ? Cin : Cout) * HW < (1ll << 31);
    const ConvDir d = conv_dir(Cin, Cout, backward_data, DC_CH);
    return (d.Cc + DC_CH) * HW < (1ll << 29) && d.Kk * HW < (1ll << 31);
}

// 3x3 / stride 2 / pad 1 (conv_s2_f32.inc)
inline bool s2_args_ok(int B, int Cin, int H, int W, int Cout)
{
    return conv_sizes_ok(B, Cin, H, W, Cout) && (H & 1) == 0 && (W & 7) == 0 && (Cin & 15) == 0 &&
           (int64_t)Cin * H * W < (1ll << 29) && (int64_t)Cout * (H / 2) * (W / 2) < (1ll << 29);
}

// ---- weight-gradient partitions: S pixel splits per block of the weight matrix, one partial per split ------------------------
// 1x1: blocks of 64 outputs x group_width inputs (128 in the one-product form, 64 in fp32)
struct PwWrwPartition {
    int nog, ncg, S, group_width;
    size_t bytes() const { return (size_t)nog * ncg * S * 64 * group_width * sizeof(float); }
};

inline PwWrwPartition pw_wrw_partition(int cus, int B, int O, int C, long long HW, int group_width)
{
    PwWrwPartition p;
    p.group_width = group_width;
    p.nog = (O + 63) / 64;
    p.ncg = (C + group_width - 1) / group_width;
    const int64_t T = (int64_t)B * ((HW + 63) / 64);
    int64_t s = 2 * (int64_t)cus / (p.nog * p.ncg);           // two workgroups per CU
    if (s > T / 4) s = T / 4;
    if (s < 1) s = 1;
    p.S = (int)s;
    return p;
}

// 3x3 / stride 2: blocks of 32 x 32 channels, each split writes all nine taps
struct S2WrwSplits {
    int S, Cin, Cout;
    size_t bytes() const { return (size_t)S * 9 * Cout * Cin * sizeof(float); }
};

inline S2WrwSplits s2_wrw_splits(int cus, int B, int Cin, int H, int W, int Cout)
{
    const int nblk = ((Cout + 31) / 32) * ((Cin + 31) / 32);
    const int64_t groups = (int64_t)B * (H / 2) * (W / 2) / 8;
    int64_t S = (8 * (int64_t)cus + nblk - 1) / nblk;                 // two waves per SIMD over the chip
    if (S > groups / 8) S = groups / 8;                               // at least eight iterations per wave
    if (S < 1) S = 1;
    return {(int)S, Cin, Cout};
}

// 3x3 / stride 1 (Winograd and direct-bf16 weight gradient): blocks of KO outputs x 64 inputs, twelve planes per partial
struct WrwPartition {
    int nog, ncg, S, strips_x, KO;
    int nblk() const { return nog * ncg; }
    size_t bytes() const { return (size_t)nblk() * S * 12 * KO * 64 * sizeof(float); }
};

inline WrwPartition wrw_partition(int B, int Cin, int H, int W, int Cout)
{
    WrwPartition p;
    p.KO = Cout <= 32 ? 32 : 64;
    p.nog = (Cout + p.KO - 1) / p.KO;
    p.ncg = (Cin + 63) / 64;
    p.strips_x = (W + 31) / 32;
    const int T = B * (H / 2) * p.strips_x;
    // about one workgroup per CU.  The 256 is a literal, NOT the device's CU count (every other partition asks for that):
    // replacing it would change workspace sizes and launch grids on other parts.
    int S = 256 / p.nblk();
    // ... but at least four strips per workgroup: every split writes a 16 x 64 x 64 partial (67 MB for 256 of them) that the
    // reduce kernel reads back, which at one image per GPU cost more than the product itself (29 + 17 us at 64 -> 64 @ 96x320)
    if (S > T / 4) S = T / 4;
    if (S >= 8) S &= ~7;
    if (S < 1) S = 1;
    if (S > T) S = T;
    p.S = S;
    return p;
}

}  // namespace
