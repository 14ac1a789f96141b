// csrc/dcn_workspace.h compiled for the HOST (plain g++, no HIP): the workspace map of the deformable convolution as a table of
// (offset, bytes) per region, for tests/test_dcn_workspace_host.py.  With -DDCN_WORKSPACE_MAIN it is a stand-alone program that
// walks a list of geometries (one per line: B C H W Co kh kw sh sw ph pw dh dw dg) -- built with -fsanitize=address,undefined
// it checks the map's own arithmetic.
#include <stdio.h>

#include "../../dcd_amd/csrc/dcn_workspace.h"

namespace {

struct Named { const char *name; Region DcnWorkspace::*r; };
const Named REGIONS[] = {
    {"wf", &DcnWorkspace::wf}, {"wb", &DcnWorkspace::wb}, {"scalars", &DcnWorkspace::scalars}, {"inv_cnt", &DcnWorkspace::inv_cnt},
    {"inv_idx", &DcnWorkspace::inv_idx}, {"inv_w", &DcnWorkspace::inv_w}, {"far_flag", &DcnWorkspace::far_flag},
    {"far_list", &DcnWorkspace::far_list}, {"dw_part", &DcnWorkspace::dw_part}, {"blockmax", &DcnWorkspace::blockmax},
    {"tileflag", &DcnWorkspace::tileflag}, {"dense_col", &DcnWorkspace::dense_col}, {"dense_part", &DcnWorkspace::dense_part},
    {"sw_wp", &DcnWorkspace::sw_wp}, {"sw_cpart", &DcnWorkspace::sw_cpart}, {"sw_dwpart", &DcnWorkspace::sw_dwpart},
    {"sw_col", &DcnWorkspace::sw_col}, {"fwd_wl", &DcnWorkspace::fwd_wl}, {"fwd_wf9", &DcnWorkspace::fwd_wf9},
    {"fwd_flags", &DcnWorkspace::fwd_flags}, {"fwd_far_count", &DcnWorkspace::fwd_far_count}, {"fwd_w9", &DcnWorkspace::fwd_w9},
};
constexpr int NREG = sizeof(REGIONS) / sizeof(REGIONS[0]);

}  // namespace

extern "C" {

int dcn_ws_region_count() { return NREG; }
const char *dcn_ws_region_name(int i) { return REGIONS[i].name; }

// which: 0 backward, 1 forward fp32, 2 forward split-bf16.  regions: NREG x (offset, bytes).  info: total, base_end, dense_end,
// has_dense, has_sweep, has_tile, forward takes the column-buffer route.  Returns 0 for an invalid geometry.
int dcn_ws_map(const int *q, int which, unsigned long long *regions, unsigned long long *info)
{
    Geom g;
    if (!make_geom(g, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11], q[12], q[13])) return 0;
    const DcnWorkspace m = which == 0 ? dcn_workspace_backward(g) : dcn_workspace_forward(g, which == 2);
    for (int i = 0; i < NREG; ++i) {
        regions[2 * i] = (m.*REGIONS[i].r).off;
        regions[2 * i + 1] = (m.*REGIONS[i].r).bytes;
    }
    info[0] = m.total; info[1] = m.base_end; info[2] = m.dense_end;
    info[3] = m.has_dense; info[4] = m.has_sweep; info[5] = m.has_tile; info[6] = which != 0 && dense_ok(g, false);
    return 1;
}

}  // extern "C"

#ifdef DCN_WORKSPACE_MAIN
int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    int q[14], n = 0, bad = 0;
    unsigned long long sum = 0, regions[2 * NREG], info[7];
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d", q, q + 1, q + 2, q + 3, q + 4, q + 5, q + 6, q + 7, q + 8, q + 9, q + 10,
                  q + 11, q + 12, q + 13) == 14) {
        for (int which = 0; which < 3; ++which) {
            if (!dcn_ws_map(q, which, regions, info)) continue;
            for (int i = 0; i < NREG; ++i)
                if (which == 0 && regions[2 * i] + regions[2 * i + 1] > info[0]) ++bad;
            sum += info[0];
        }
        ++n;
    }
    fclose(f);
    printf("%d geometries, %llu bytes in all, %d regions past the end\n", n, sum, bad);
    return bad ? 1 : 0;
}
#endif
