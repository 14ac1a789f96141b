// Host instantiation of csrc/records_math.h: the three launches of csrc/records.hip in plain loops (a "lane" is a loop index,
// the tree over the lanes' partial sums runs in the kernel's order; the 1 500 pairs are selected with a sort under the solver's
// rule: largest |v'_i - v'_j| first, ties by lower pair index), so that tests/test_records_host.py can hold the arithmetic and
// the compaction rules against the reference's `Loss_Computation.gen_data` fixture on a machine without a GPU.  The signature
// is dcd_gmw_train_records' (the stream is ignored), the workspace is used as the kernels use it.  Test infrastructure only --
// nothing under dcd_amd/ links or loads this.
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../dcd_amd/csrc/records_math.h"

extern "C" size_t host_gmw_train_records_workspace_bytes(int B, int M, int nk)
{
    if (B < 1 || M < 1 || nk < 2 || nk > RM_MAXK || (int64_t)B * M > 0x7fffffffLL / 2) return 0;
    return sizeof(float) * rm_workspace_floats(B * M, nk);
}

extern "C" int host_gmw_train_records(void *, const float *reg_pois, const dcd_records_args *args, const uint8_t *reg_mask,
                                      const int32_t *target_centers, const float *offset_3D, const float *rotys,
                                      const float *locations, const float *calib_P, const int64_t *pad_size, const float *calib,
                                      const int32_t *image_numbers, int cap, float *kpts_2d, float *kpts_3d, float *pred_rot,
                                      float *gt_location, float *pred_location, int32_t *image, int32_t *cursor, int32_t *per_call,
                                      int call, int n_calls, void *workspace, size_t workspace_bytes)
{
    if (!args) return DCD_ERR_BAD_ARG;
    const dcd_records_args a = *args;
    if (!reg_pois || !reg_mask || !target_centers || !offset_3D || !rotys || !locations || !calib_P || !pad_size || !calib ||
        !image_numbers || !kpts_2d || !kpts_3d || !pred_rot || !gt_location || !pred_location || !image || !cursor || !per_call ||
        !workspace)
        return DCD_ERR_BAD_ARG;
    if (!rm_args_ok(a) || cap < 1 || call < 0 || call >= n_calls) return DCD_ERR_BAD_ARG;
    const int slots = a.B * a.M, nk = a.nk, topk = rm_topk(nk), npairs = nk * (nk - 1) / 2;
    if (workspace_bytes < sizeof(float) * rm_workspace_floats(slots, nk)) return DCD_ERR_WORKSPACE;
    const RmWorkspace w = rm_workspace(workspace, slots, nk);

    // 1. prepare
    for (int slot = 0; slot < slots; ++slot) {
        const int b = slot / a.M;
        const bool set = reg_mask[slot] != 0;
        const float *vec = reg_pois + (size_t)slot * a.C;
        float *kps = w.kps + (size_t)slot * nk * 2, *k3 = w.kps3d + (size_t)slot * nk * 3;
        if (set) {
            const RmSlot s = rm_slot(target_centers, offset_3D, pad_size, b, slot);
            for (int k = 0; k < nk; ++k) rm_kpt_img(a, vec, s, k, kps + 2 * k);
            memcpy(k3, vec + a.ch_kpts3d, sizeof(float) * 3 * nk);
        } else {
            memset(kps, 0, sizeof(float) * 2 * nk);
            memset(k3, 0, sizeof(float) * 3 * nk);
        }
        for (int i = 0; i < 12; ++i) w.P[(size_t)slot * 12 + i] = set ? calib_P[(size_t)slot * 12 + i] : ((i % 5 == 0) ? 1.f : 0.f);
        w.rot[slot] = set ? rotys[slot] : 0.f;
    }

    // 2. the solver, training form: depth - P[2][3] of the topk pairs, ordered by (|dv| descending, pair index ascending)
    std::vector<float> z(npairs);
    std::vector<uint64_t> key(npairs);
    for (int slot = 0; slot < slots; ++slot) {
        const float *P = w.P + (size_t)slot * 12;
        const float sn = sinf(w.rot[slot]), cs = cosf(w.rot[slot]);
        float vn[RM_MAXK], Y[RM_MAXK], vC[RM_MAXK];
        for (int k = 0; k < nk; ++k)
            rm_solver_point(w.kps[((size_t)slot * nk + k) * 2 + 1], w.kps3d + ((size_t)slot * nk + k) * 3, P, sn, cs, vn + k, Y + k, vC + k);
        int q = 0;
        for (int i = 0; i < nk - 1; ++i)
            for (int j = i + 1; j < nk; ++j, ++q) {
                float dv;
                z[q] = rm_pair(i, j, vn, Y, vC, &dv);
                uint32_t bits;
                memcpy(&bits, &dv, 4);
                key[q] = ((uint64_t)bits << 32) | (uint32_t)(~(uint32_t)q);
            }
        std::sort(key.begin(), key.end(), [](uint64_t x, uint64_t y) { return x > y; });
        for (int r = 0; r < topk; ++r) {
            const uint32_t p = ~(uint32_t)(key[r] & 0xffffffffull);
            w.depth[(size_t)slot * topk + r] = z[p] - P[11];
            w.pair_idx[(size_t)slot * topk + r] = (int32_t)p;
        }
    }

    // 3. finish
    int total = 0;
    for (int i = 0; i < slots; ++i) total += reg_mask[i] != 0;
    const int start = cursor[call & 1];
    int before = 0;
    for (int slot = 0; slot < slots; ++slot) {
        if (reg_mask[slot] == 0) continue;
        const int64_t dst = (int64_t)start + before++;
        if (dst < 0 || dst >= cap) continue;
        float part[RM_LANES];
        for (int t = 0; t < RM_LANES; ++t) part[t] = rm_lane_partial(t, topk, w.depth + (size_t)slot * topk);
        for (int s = RM_LANES / 2; s > 0; s >>= 1)
            for (int t = 0; t < s; ++t) part[t] = RM_ADD(part[t], part[t + s]);
        const float depth = part[0] / (float)topk;
        const int b = slot / a.M;
        const float *vec = reg_pois + (size_t)slot * a.C;
        const float *tab = calib + (size_t)b * 6;
        const RmSlot s = rm_slot(target_centers, offset_3D, pad_size, b, slot);
        rm_location(a, s, vec[a.ch_offset], vec[a.ch_offset + 1], depth, tab, pred_location + dst * 3);
        rm_location(a, s, s.off_x, s.off_y, locations[(size_t)slot * 3 + 2], tab, gt_location + dst * 3);
        pred_rot[dst] = rm_roty(a, vec, pred_location + dst * 3);
        image[dst] = image_numbers[b];
        for (int k = 0; k < nk; ++k) rm_normalise(w.kps + ((size_t)slot * nk + k) * 2, calib, kpts_2d + (dst * nk + k) * 2);
        memcpy(kpts_3d + dst * nk * 3, vec + a.ch_kpts3d, sizeof(float) * 3 * nk);
    }
    const int64_t next = (int64_t)start + total;
    cursor[(call + 1) & 1] = next > 0x7fffffffLL ? 0x7fffffff : (int32_t)next;
    per_call[call] = total;
    return DCD_OK;
}
