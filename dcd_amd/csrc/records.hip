// records.hip -- GMW's training records of a batch, collected on the device (include/dcd_hip.h, dcd_gmw_train_records).
//
// Three launches per call, nothing read back:
//   records_prepare   one wave per slot (b, m): the slot's key points in image pixels, its 3-D key points, the target yaw and
//                     Calib_P in the layout dcd_edge_depth_forward reads; an empty slot gets zeros and a unit P, so the solver
//                     works on finite numbers there
//   edge_depth_fwd    the existing solver launch (heads.hip) over all B M slots, training form: the top-1 500 pairs
//   records_finish    one wave per slot: the fixed-order mean of the slot's kept depths (lane partials in rank order, a shuffle
//                     tree in the order of the host build's loop), locations, yaw, normalisation, and the row stores at
//                     cursor + (set mask bytes before the slot).  B M is a few hundred mask bytes, so every wave counts them
//                     itself: no atomics, no "last block".  The cursor is a pair used alternately -- every workgroup reads
//                     cursor[call & 1], workgroup 0 writes cursor[(call + 1) & 1] -- so no workgroup reads what another writes.
// The work is small (<= 320 waves, 6 KB in and 1.5 KB out each): the three launches are the cost.  The arithmetic is
// csrc/records_math.h; all stores are plain vector stores.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dcd_hip.h"
#include "records_math.h"

namespace {

__global__ __launch_bounds__(RM_LANES) void records_prepare(const float *__restrict__ reg_pois, const dcd_records_args a,
                                                            const uint8_t *__restrict__ reg_mask,
                                                            const int32_t *__restrict__ centers,
                                                            const float *__restrict__ offset_3D, const float *__restrict__ rotys,
                                                            const float *__restrict__ calib_P,
                                                            const int64_t *__restrict__ pad_size, const RmWorkspace w)
{
    const int slot = blockIdx.x, lane = threadIdx.x;
    const int b = slot / a.M, nk = a.nk;
    const bool set = reg_mask[slot] != 0;                               // uniform over the wave
    const float *vec = reg_pois + (size_t)slot * a.C;
    float *kps = w.kps + (size_t)slot * nk * 2, *k3 = w.kps3d + (size_t)slot * nk * 3;
    if (set) {
        const RmSlot s = rm_slot(centers, offset_3D, pad_size, b, slot);
        for (int k = lane; k < nk; k += RM_LANES) {
            float uv[2];
            rm_kpt_img(a, vec, s, k, uv);
            kps[2 * k] = uv[0];
            kps[2 * k + 1] = uv[1];
        }
        for (int t = lane; t < 3 * nk; t += RM_LANES) k3[t] = vec[a.ch_kpts3d + t];
    } else {
        for (int t = lane; t < 2 * nk; t += RM_LANES) kps[t] = 0.f;
        for (int t = lane; t < 3 * nk; t += RM_LANES) k3[t] = 0.f;
    }
    if (lane < 12) {
        const float unit = (lane == 0 || lane == 5 || lane == 10) ? 1.f : 0.f;
        w.P[(size_t)slot * 12 + lane] = set ? calib_P[(size_t)slot * 12 + lane] : unit;
    } else if (lane == 12) {
        w.rot[slot] = set ? rotys[slot] : 0.f;
    }
}

__device__ __forceinline__ int records_wave_sum(int v)
{
#pragma unroll
    for (int o = RM_LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(RM_LANES) void records_finish(const float *__restrict__ reg_pois, const dcd_records_args a,
                                                           const uint8_t *__restrict__ reg_mask,
                                                           const int32_t *__restrict__ centers,
                                                           const float *__restrict__ offset_3D,
                                                           const float *__restrict__ locations,
                                                           const int64_t *__restrict__ pad_size, const float *__restrict__ calib,
                                                           const int32_t *__restrict__ image_numbers, const RmWorkspace w, int cap,
                                                           float *__restrict__ kpts_2d, float *__restrict__ kpts_3d,
                                                           float *__restrict__ pred_rot, float *__restrict__ gt_location,
                                                           float *__restrict__ pred_location, int32_t *__restrict__ image,
                                                           const int32_t *__restrict__ cursor_in, int32_t *__restrict__ cursor_out,
                                                           int32_t *__restrict__ count_out)
{
    const int slot = blockIdx.x, lane = threadIdx.x;
    const int slots = a.B * a.M, nk = a.nk;

    // the compaction: set flags before this slot, and in the whole batch
    int before = 0, total = 0;
    for (int i = lane; i < slots; i += RM_LANES) {
        const int f = reg_mask[i] != 0;
        total += f;
        before += (i < slot) ? f : 0;
    }
    before = records_wave_sum(before);
    total = records_wave_sum(total);
    const int start = *cursor_in;
    if (slot == 0 && lane == 0) {
        const int64_t next = (int64_t)start + total;
        *cursor_out = next > 0x7fffffffLL ? 0x7fffffff : (int32_t)next;
        *count_out = total;
    }
    if (reg_mask[slot] == 0) return;                                    // uniform over the wave
    const int64_t dst = (int64_t)start + before;
    if (dst < 0 || dst >= cap) return;                                  // the surplus is counted, not written

    // the mean of the kept depths in a fixed order: lane partials in rank order, then the tree part[t] += part[t + s]
    const int topk = rm_topk(nk);
    float part = rm_lane_partial(lane, topk, w.depth + (size_t)slot * topk);
#pragma unroll
    for (int s = RM_LANES / 2; s > 0; s >>= 1) part = RM_ADD(part, __shfl_down(part, s));
    const float depth = __shfl(part, 0) / (float)topk;

    const int b = slot / a.M;
    const float *vec = reg_pois + (size_t)slot * a.C;
    const float *tab = calib + (size_t)b * 6;
    const RmSlot s = rm_slot(centers, offset_3D, pad_size, b, slot);
    float ploc[3], gloc[3];
    rm_location(a, s, vec[a.ch_offset], vec[a.ch_offset + 1], depth, tab, ploc);
    rm_location(a, s, s.off_x, s.off_y, locations[(size_t)slot * 3 + 2], tab, gloc);
    const float roty = rm_roty(a, vec, ploc);
    if (lane < 3) {
        pred_location[dst * 3 + lane] = lane == 0 ? ploc[0] : (lane == 1 ? ploc[1] : ploc[2]);
        gt_location[dst * 3 + lane] = lane == 0 ? gloc[0] : (lane == 1 ? gloc[1] : gloc[2]);
    } else if (lane == 3) {
        pred_rot[dst] = roty;
        image[dst] = image_numbers[b];
    }
    const float *kps = w.kps + (size_t)slot * nk * 2;
    float *k2 = kpts_2d + dst * nk * 2, *k3 = kpts_3d + dst * nk * 3;
    for (int k = lane; k < nk; k += RM_LANES) {
        const float uv[2] = {kps[2 * k], kps[2 * k + 1]};
        float out[2];
        rm_normalise(uv, calib, out);                                   // image 0's intrinsics for every object
        k2[2 * k] = out[0];
        k2[2 * k + 1] = out[1];
    }
    for (int t = lane; t < 3 * nk; t += RM_LANES) k3[t] = vec[a.ch_kpts3d + t];
}

}  // namespace

extern "C" {

size_t dcd_gmw_train_records_workspace_bytes(int B, int M, int nk)
{
    if (B < 1 || M < 1 || nk < 2 || nk > RM_MAXK || (int64_t)B * M > 0x7fffffffLL / 2) return 0;
    return sizeof(float) * rm_workspace_floats(B * M, nk);
}

int dcd_gmw_train_records(void *stream_, const float *reg_pois, const dcd_records_args *args, const uint8_t *reg_mask,
                          const int32_t *target_centers, const float *offset_3D, const float *rotys, const float *locations,
                          const float *calib_P, const int64_t *pad_size, const float *calib, const int32_t *image_numbers, int cap,
                          float *kpts_2d, float *kpts_3d, float *pred_rot, float *gt_location, float *pred_location, int32_t *image,
                          int32_t *cursor, int32_t *per_call, int call, int n_calls, void *workspace, size_t workspace_bytes)
{
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (!args) return DCD_ERR_BAD_ARG;
    const dcd_records_args a = *args;
    if (!reg_pois || !reg_mask || !target_centers || !offset_3D || !rotys || !locations || !calib_P || !pad_size || !calib ||
        !image_numbers || !kpts_2d || !kpts_3d || !pred_rot || !gt_location || !pred_location || !image || !cursor || !per_call ||
        !workspace)
        return DCD_ERR_BAD_ARG;
    if (!rm_args_ok(a) || cap < 1 || call < 0 || call >= n_calls) return DCD_ERR_BAD_ARG;
    const int slots = a.B * a.M;
    if (workspace_bytes < sizeof(float) * rm_workspace_floats(slots, a.nk)) return DCD_ERR_WORKSPACE;
    const RmWorkspace w = rm_workspace(workspace, slots, a.nk);

    hipLaunchKernelGGL(records_prepare, dim3((unsigned)slots), dim3(RM_LANES), 0, stream, reg_pois, a, reg_mask, target_centers,
                       offset_3D, rotys, calib_P, pad_size, w);
    if (hipGetLastError() != hipSuccess) return DCD_ERR_LAUNCH;
    const int st = dcd_edge_depth_forward(stream_, w.kps, w.kps3d, w.rot, w.P, nullptr, slots, a.nk, rm_topk(a.nk), RM_ZMIN, RM_ZMAX, 0, 1,
                                          w.depth, w.pair_idx, nullptr);
    if (st != DCD_OK) return st;
    hipLaunchKernelGGL(records_finish, dim3((unsigned)slots), dim3(RM_LANES), 0, stream, reg_pois, a, reg_mask, target_centers,
                       offset_3D, locations, pad_size, calib, image_numbers, w, cap, kpts_2d, kpts_3d, pred_rot, gt_location,
                       pred_location, image, cursor + (call & 1), cursor + ((call + 1) & 1), per_call + call);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}

}  // extern "C"
