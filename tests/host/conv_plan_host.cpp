// csrc/conv_plan.h compiled for the HOST (plain g++, no HIP): the sizes the dcd_conv* entry points advertise and the plan of a
// 3x3 / stride 1 call at a given CU count, for tests/test_conv_plan_host.py.  With -DCONV_PLAN_MAIN it is a stand-alone program
// that walks a list of geometries (one per line: B Cin H W Cout) at 64, 256 and 304 CUs -- built with
// -fsanitize=address,undefined it checks the header's own arithmetic.
#include <stdio.h>

#include "../../dcd_amd/csrc/conv_plan.h"

extern "C" {

// The *_bytes entry points of csrc/conv.hip, each as the one expression it is there, in the order of SIZE_NAMES in
// tests/golden/make_golden_conv_plans.py -- except dcd_conv3x3_bf16_weights_bytes (dc_weight_slots is device code's too and stays in
// conv_direct_bf16.inc).  q = B, Cin, H, W, Cout; the 1x1 sizes take O = Cout, C = Cin, HW = H W.
int conv_plan_size_count() { return 11; }

void conv_plan_sizes(int cus, const int *q, unsigned long long *out)
{
    const int B = q[0], Cin = q[1], H = q[2], W = q[3], Cout = q[4];
    for (int i = 0; i < conv_plan_size_count(); ++i) out[i] = 0;
    if (Cin > 0 && Cout > 0)
        for (int bwd = 0; bwd < 2; ++bwd) {
            out[1 + bwd] = conv_dir(Cin, Cout, bwd, WN_CH).wino_floats() * sizeof(float);
            out[3 + bwd] = conv_dir(Cin, Cout, bwd, WS_CH).split_dwords() * sizeof(unsigned);
        }
    if (s2_args_ok(B, Cin, H, W, Cout)) out[8] = s2_wrw_splits(cus, B, Cin, H, W, Cout).bytes();
    if (!conv_sizes_ok(B, Cin, H, W, Cout)) return;
    out[0] = wino_floats_bound(Cin, Cout) * sizeof(float) + conv_part_bytes_either(CONV_F32, cus, B, Cin, H, W, Cout);
    out[5] = conv_part_bytes_either(CONV_SPLIT, cus, B, Cin, H, W, Cout) + 16;
    out[6] = conv_part_bytes_either(CONV_DIRECT, cus, B, Cin, H, W, Cout) + 16;
    out[7] = wrw_partition(B, Cin, H, W, Cout).bytes();
    out[9] = pw_wrw_partition(cus, B, Cout, Cin, (long long)H * W, 128).bytes();
    out[10] = pw_wrw_partition(cus, B, Cout, Cin, (long long)H * W, 64).bytes();
}

// One call of form 0 (fp32) / 1 (split-bf16) / 2 (direct) as conv3x3_run plans it.  out: the shape rule's verdict, bytes the run
// needs with prepared weights, with raw weights (fp32 form; else the same), bytes advertised, ksplit, nz, nb, Kk, tiles_x, tiles_y,
// region rows, region columns.  Returns 0 when a size is not positive.
int conv_plan_query(int form_, int cus, const int *q, int backward_data, unsigned long long *out)
{
    const int B = q[0], Cin = q[1], H = q[2], W = q[3], Cout = q[4];
    if (!conv_sizes_ok(B, Cin, H, W, Cout)) return 0;
    const ConvForm form = (ConvForm)form_;
    const ConvDir d = conv_dir(Cin, Cout, backward_data, WN_CH);
    const ConvPlan pl = conv_plan_of(form, cus, B, d.Cc, H, W, d.Kk);
    int rows, cols;
    conv_region(form, pl.geom, rows, cols);
    unsigned long long sizes[11];
    conv_plan_sizes(cus, q, sizes);
    out[0] = conv3x3_shape_ok(form, B, Cin, H, W, Cout, backward_data);
    out[1] = pl.part_bytes();
    out[2] = pl.part_bytes() + (form == CONV_F32 ? d.wino_floats() * sizeof(float) : 0);
    out[3] = form == CONV_F32 ? sizes[0] : form == CONV_SPLIT ? sizes[5] : sizes[6];
    out[4] = pl.ksplit; out[5] = pl.nz; out[6] = pl.nb; out[7] = d.Kk;
    out[8] = pl.tiles_x; out[9] = pl.tiles_y; out[10] = rows; out[11] = cols;
    return 1;
}

}  // extern "C"

#ifdef CONV_PLAN_MAIN
int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    int q[5], n = 0, plans = 0, bad = 0;
    unsigned long long sum = 0, o[12], sizes[11];
    while (fscanf(f, "%d %d %d %d %d", q, q + 1, q + 2, q + 3, q + 4) == 5) {
        const int counts[] = {64, 256, 304};
        for (int cus : counts) {
            conv_plan_sizes(cus, q, sizes);
            for (int i = 0; i < conv_plan_size_count(); ++i) sum += sizes[i];
            for (int form = 0; form < 3; ++form)
                for (int bwd = 0; bwd < 2; ++bwd) {
                    if (!conv_plan_query(form, cus, q, bwd, o)) continue;
                    ++plans;
                    const bool covers = o[8] * o[11] >= (unsigned long long)q[3] && o[9] * o[10] >= (unsigned long long)q[2];
                    if (o[1] > o[3] || o[2] > o[3] || o[5] * 32 * o[6] < o[7] || !covers) ++bad;
                }
        }
        ++n;
    }
    fclose(f);
    printf("%d geometries, %d plans, %llu bytes in all, %d plans that break a property\n", n, plans, sum, bad);
    return bad ? 1 : 0;
}
#endif
