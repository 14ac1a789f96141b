// Host instantiation of csrc/decode_math.h: the candidate loop of csrc/decode.hip in plain loops (a "lane" is a loop index,
// the tree over the lanes' partial sums runs in the kernel's order), so that tests/test_decode_host.py can hold the decode
// arithmetic against the reference's PostProcessor fixture on a machine without a GPU.  Test infrastructure only --
// nothing under dcd_amd/ links or loads this.
#include "../../dcd_amd/csrc/decode_math.h"

extern "C" int host_decode_detections(const float *vectors, const float *scores, const float *classes, const float *ys, const float *xs,
                                      const float *table, const dcd_decode_args *args, float *rows, float *aux, float *kpts2d,
                                      float *kpts3d)
{
    const dcd_decode_args a = *args;
    if (a.nk < 2 || a.nk > 128 || a.K < 1 || a.K > 128 || a.orientation != DCD_DECODE_ORI_MULTIBIN) return DCD_ERR_BAD_ARG;
    const int nk = a.nk;
    for (int n = 0; n < a.B * a.K; ++n) {
        const float *vec = vectors + (size_t)n * a.C;
        const float *tab = table + (size_t)(n / a.K) * DD_TABLE;
        const DdHead h = dd_head(a, vec, scores[n], classes[n], ys[n], xs[n], tab);
        const float sn = sinf(h.roty), cs = cosf(h.roty);
        float vn[128], Y[128], vC[128], part[DD_LANES];
        for (int k = 0; k < nk; ++k) {
            const DdKeypoint p = dd_keypoint(a, vec, h, tab, k, sn, cs);
            vn[k] = p.vn;
            Y[k] = p.Y;
            vC[k] = p.vC;
            if (a.records) {
                const float *P = tab + 4;
                float *k2 = kpts2d + ((size_t)n * nk + k) * 2, *k3 = kpts3d + ((size_t)n * nk + k) * 3;
                k2[0] = (p.u - P[2]) / P[0];
                k2[1] = (p.v - P[6]) / P[5];
                k3[0] = p.X;
                k3[1] = p.Y;
                k3[2] = p.Z;
            }
        }
        for (int t = 0; t < DD_LANES; ++t) part[t] = dd_pair_partial(t, nk, vn, Y, vC, tab[4 + 11]);
        for (int s = DD_LANES / 2; s > 0; s >>= 1)
            for (int t = 0; t < s; ++t) part[t] = DD_ADD(part[t], part[t + s]);
        dd_finish(a, h, tab, part[0], rows + (size_t)n * 14, aux + (size_t)n * 4);
    }
    return DCD_OK;
}
