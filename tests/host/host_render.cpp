// TEST INFRASTRUCTURE: csrc/render_math.h compiled for the host, the two kernels of csrc/render.hip as plain loops.
// Built by tests/test_render_host.py with -ffp-contract=off; the library has no host path.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../dcd_amd/csrc/render_math.h"

static void raster(const uint8_t *staged, uint64_t staged_bytes, const int *table, const int *counts, int B, int stride, int in_h,
                   int in_w, uint8_t *canvas)
{
    const int CW = in_w + in_h;
    memset(canvas, 0, (size_t)B * in_h * CW * 3);
    std::vector<uint32_t> key((size_t)in_h * CW);
    for (int b = 0; b < B; ++b) {
        int w, h, flip;
        int64_t off, pitch;
        rd_frame((const int64_t *)staged, staged_bytes, b, in_h, in_w, &w, &h, &off, &pitch, &flip);
        const int *ent = table + (int64_t)b * stride * RD_ENTRY;
        std::fill(key.begin(), key.end(), 0u);
        int count = counts[b];
        count = count < 0 ? 0 : (count > stride ? stride : count);
        for (int i = 0; i < count; ++i) {
            const int *e = ent + (int64_t)i * RD_ENTRY;
            if (!rd_entry_ok(e)) continue;
            const int left = e[0] ? w : 0, pw = e[0] ? h : w;
            const uint32_t k = rd_key(e, i);
            rd_raster(e, 0, 0, pw - 1, h - 1, [&](int x, int y) {
                uint32_t &at = key[(size_t)y * CW + x + left];
                at = k > at ? k : at;
            });
        }
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w + h; ++x) {
                uint8_t *px = canvas + (((size_t)b * in_h + y) * CW + x) * 3;
                const uint32_t k = key[(size_t)y * CW + x];
                if (k) {
                    const int *e = ent + (int64_t)(k & (RD_MAX_ENTRIES - 1)) * RD_ENTRY;
                    for (int c = 0; c < 3; ++c) px[c] = (uint8_t)e[7 + c];
                } else if (x < w) {
                    const uint8_t *src = staged + off + (int64_t)y * pitch + 3 * (int64_t)(flip ? w - 1 - x : x);
                    for (int c = 0; c < 3; ++c) px[c] = src[c];
                } else {
                    px[0] = px[1] = px[2] = RD_BACKGROUND;
                }
            }
    }
}

extern "C" int host_render_slots(int M, int K, int nk) { return rd_slots(M, K, nk); }

extern "C" int host_render_detections(const uint8_t *staged, uint64_t staged_bytes, const float *rows, const float *aux, const float *k2,
                                      const float *image_table, const float *gt_dims, const float *gt_locs, const float *gt_rotys,
                                      const uint8_t *gt_mask, int B, int K, int nk, int M, int in_h, int in_w, double det_threshold,
                                      double vis_threshold, int *table, int *counts, float *ends, uint8_t *canvas)
{
    const int slots = rd_slots(M, K, nk);
    if (slots < 1 || slots > RD_MAX_ENTRIES) return 1;
    RdArgs a;
    a.B = B, a.K = K, a.nk = nk, a.M = M;
    a.det_threshold = (float)det_threshold, a.vis_threshold = (float)vis_threshold;
    a.rows = rows, a.aux = aux, a.k2 = k2, a.table = image_table;
    a.gt_dims = gt_dims, a.gt_locs = gt_locs, a.gt_rotys = gt_rotys, a.gt_mask = gt_mask;
    a.recs = (const int64_t *)staged, a.staged_bytes = staged_bytes;
    a.in_h = in_h, a.in_w = in_w;
    for (int b = 0; b < B; ++b) {
        int w, h, flip;
        int64_t off, pitch;
        rd_frame(a.recs, staged_bytes, b, in_h, in_w, &w, &h, &off, &pitch, &flip);
        int last = 0;
        for (int obj = 0; obj < M + K; ++obj) {
            const int l = rd_object(a, b, obj, h, table + (int64_t)b * slots * RD_ENTRY, ends ? ends + (int64_t)b * slots * 4 : nullptr);
            last = l > last ? l : last;
        }
        counts[b] = last;
    }
    raster(staged, staged_bytes, table, counts, B, slots, in_h, in_w, canvas);
    return 0;
}

extern "C" int host_render_primitives(const uint8_t *staged, uint64_t staged_bytes, const int *table, const int *counts, int B,
                                      int stride, int in_h, int in_w, uint8_t *canvas)
{
    if (stride < 1 || stride > RD_MAX_ENTRIES) return 1;
    raster(staged, staged_bytes, table, counts, B, stride, in_h, in_w, canvas);
    return 0;
}
