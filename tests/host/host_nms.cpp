// Host instantiation of csrc/nms_math.h: the image loop of csrc/nms.hip in plain loops (a "lane" is a loop index, a ballot is
// a loop that sets bits), so that tests/test_nms_host.py can hold the overlaps, the visit order, the greedy rule and the output
// order against tests/nms_refs.py on a machine without a GPU.  Test infrastructure only -- nothing under dcd_amd/ links or
// loads this.
#include "../../dcd_amd/csrc/nms_math.h"

extern "C" int host_nms_detections(const float *rows, const float *aux, const float *kpts2d, const float *kpts3d, int B, int K, int nk,
                                   int mode, double thresh, double det_threshold, int class_agnostic, float *rows_out, float *aux_out,
                                   float *kpts2d_out, float *kpts3d_out, float *overlaps_out)
{
    if (!rows || !aux || !rows_out || !aux_out || B < 1 || K < 1 || K > NMS_MAXK) return DCD_ERR_BAD_ARG;
    if (mode != DCD_NMS_2D && mode != DCD_NMS_BEV && mode != DCD_NMS_3D) return DCD_ERR_BAD_ARG;
    if (!(thresh >= 0.0 && thresh < 1.0) || det_threshold != det_threshold) return DCD_ERR_BAD_ARG;
    const bool kpts = kpts2d != nullptr;
    if (kpts && (!kpts3d || !kpts2d_out || !kpts3d_out || nk < 1 || nk > 128)) return DCD_ERR_BAD_ARG;
    for (int img = 0; img < B; ++img) {
        const size_t row0 = (size_t)img * K;
        const float *row = rows + row0 * NMS_ROW;
        int n = 0;
        while (n < K && nms_is_candidate(aux[(row0 + n) * NMS_AUX], det_threshold)) ++n;
        int order[NMS_MAXK], rank[NMS_MAXK];
        for (int t = 0; t < n; ++t) {
            int r = 0;
            for (int j = 0; j < n; ++j) r += nms_before(row[j * NMS_ROW + 13], j, row[t * NMS_ROW + 13], t) ? 1 : 0;
            rank[t] = r;
            order[r] = t;
        }
        uint32_t bits[NMS_MAXK * NMS_WORDS] = {0};
        float *ovl = overlaps_out ? overlaps_out + (size_t)img * K * K : nullptr;
        if (ovl)
            for (int i = 0; i < K * K; ++i) ovl[i] = 0.f;
        for (int r = 0; r + 1 < n; ++r) {
            const float *q = row + order[r] * NMS_ROW;
            for (int c = r + 1; c < n; ++c) {
                const float *b = row + order[c] * NMS_ROW;
                if (!(ovl || class_agnostic || nms_same_class(q, b))) continue;
                const double o = nms_overlap(mode, q, b);
                if (nms_suppresses(o, thresh, class_agnostic != 0, q, b)) bits[r * NMS_WORDS + (c >> 5)] |= 1u << (c & 31);
                if (ovl) ovl[order[r] * K + order[c]] = ovl[order[c] * K + order[r]] = (float)o;
            }
        }
        uint32_t removed[NMS_WORDS];
        nms_greedy(bits, n, removed);
        int n_keep = 0;
        for (int t = 0; t < n; ++t) n_keep += nms_bit(removed, rank[t]) ? 0 : 1;
        int next_s = 0, next_p = n_keep;
        for (int t = 0; t < K; ++t) {
            const bool suppressed = t < n && nms_bit(removed, rank[t]);
            const size_t src = row0 + t, dst = row0 + (t >= n ? t : suppressed ? next_p++ : next_s++);
            for (int i = 0; i < NMS_ROW; ++i) rows_out[dst * NMS_ROW + i] = rows[src * NMS_ROW + i];
            for (int i = 0; i < NMS_AUX; ++i) aux_out[dst * NMS_AUX + i] = aux[src * NMS_AUX + i];
            if (suppressed) aux_out[dst * NMS_AUX] = -INFINITY;
            if (kpts) {
                for (int i = 0; i < 2 * nk; ++i) kpts2d_out[dst * 2 * nk + i] = kpts2d[src * 2 * nk + i];
                for (int i = 0; i < 3 * nk; ++i) kpts3d_out[dst * 3 * nk + i] = kpts3d[src * 3 * nk + i];
            }
        }
    }
    return DCD_OK;
}
