// resident.hip -- one batch out of a split that stays in device memory (dcd_amd/data/resident.py).
//
// A KITTI split is decoded ONCE and kept on the device: one uint8 buffer of frames plus six small tables with a row per
// (image, flip) -- the image kernel's record, the raw label values, the calibration, the size, the object count.  A batch is then
// B row numbers from the host and this gather: dst[t] row b = src[t] row index[b] for every table t, in ONE launch (six
// `index_select` calls would be six launches plus the index conversions; launch count is a tracked figure of the step).
//
// The rows are 4 B to ~60 KB and B <= 32, so the launch is latency-bound: what matters is that every (table, row) has enough
// workgroups in flight, not the bytes per lane.  A workgroup owns one GATHER_CHUNK-byte piece of one row of one table; the table
// descriptors travel BY VALUE in the kernel arguments (as in optim.hip), so nothing but `index` is read from device memory
// before the payload and the call is safe inside a stream capture -- a replay follows whatever `index` holds then.
// 16-byte accesses where the table's row size and both bases allow it, 4-byte accesses otherwise.  An index outside the source
// table gives a zero row: nothing outside src is read, nothing outside dst[t][0 : B * row_bytes[t]] is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dcd_hip.h"

namespace {

constexpr int GATHER_THREADS = 256;
constexpr int GATHER_CHUNK = GATHER_THREADS * 16;    // bytes of a row per workgroup: one 16-byte access per lane
constexpr int GATHER_MAXT = 8;

struct GatherTable {
    const uint8_t *src[GATHER_MAXT];
    uint8_t *dst[GATHER_MAXT];
    int64_t row_bytes[GATHER_MAXT];
    int64_t src_rows[GATHER_MAXT];
    int blk0[GATHER_MAXT + 1];                       // first chunk of table t in a row's worth of workgroups; blk0[count] = all
    int vec[GATHER_MAXT];                            // 16-byte accesses are safe for this table
    int count;
};

__global__ __launch_bounds__(GATHER_THREADS) void gather_rows(GatherTable t, const int32_t *__restrict__ index)
{
    int k = 0;                                       // the table of this workgroup: blk0[k] <= blockIdx.x < blk0[k + 1]
    while (k + 1 < t.count && (int)blockIdx.x >= t.blk0[k + 1]) ++k;
    const int b = blockIdx.y;
    const int64_t row_bytes = t.row_bytes[k];
    const int64_t begin = (int64_t)((int)blockIdx.x - t.blk0[k]) * GATHER_CHUNK;
    const int64_t end = begin + GATHER_CHUNK < row_bytes ? begin + GATHER_CHUNK : row_bytes;
    const int64_t row = index[b];
    const bool inside = row >= 0 && row < t.src_rows[k];
    const uint8_t *s = t.src[k] + (inside ? row : 0) * row_bytes;      // never dereferenced when !inside
    uint8_t *d = t.dst[k] + (int64_t)b * row_bytes;
    if (t.vec[k]) {
        const int64_t o = begin + (int64_t)threadIdx.x * 16;           // row_bytes % 16 == 0: o < end implies o + 16 <= end
        if (o < end) {
            uint4 v = {0u, 0u, 0u, 0u};
            if (inside) v = *(const uint4 *)(s + o);
            *(uint4 *)(d + o) = v;
        }
    } else {
        for (int64_t o = begin + (int64_t)threadIdx.x * 4; o < end; o += GATHER_THREADS * 4) {   // row_bytes % 4 == 0
            uint32_t v = 0u;
            if (inside) v = *(const uint32_t *)(s + o);
            *(uint32_t *)(d + o) = v;
        }
    }
}

}  // namespace

extern "C" {

int dcd_gather_rows(void *stream_, int n_tables, const void *const *src, void *const *dst, const int64_t *row_bytes,
                    const int64_t *src_rows, const int32_t *index, int B)
{
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (!src || !dst || !row_bytes || !src_rows || !index) return DCD_ERR_BAD_ARG;
    // B is gridDim.y.  A grid that passes these checks and is still more than the runtime takes (blocks x B x 256 threads past 2^32)
    // comes back as DCD_ERR_LAUNCH, not as a bad argument; the callers' rows are <= 60 KB and B <= 32.
    if (n_tables < 1 || n_tables > GATHER_MAXT || B < 1 || B > 65535) return DCD_ERR_BAD_ARG;
    GatherTable t = {};
    int64_t blocks = 0;
    for (int k = 0; k < n_tables; ++k) {
        if (!src[k] || !dst[k] || row_bytes[k] <= 0 || row_bytes[k] % 4 != 0 || src_rows[k] < 0) return DCD_ERR_BAD_ARG;
        if (((uintptr_t)src[k] & 3) != 0 || ((uintptr_t)dst[k] & 3) != 0) return DCD_ERR_BAD_ARG;
        t.src[k] = (const uint8_t *)src[k];
        t.dst[k] = (uint8_t *)dst[k];
        t.row_bytes[k] = row_bytes[k];
        t.src_rows[k] = src_rows[k];
        t.vec[k] = row_bytes[k] % 16 == 0 && ((uintptr_t)src[k] & 15) == 0 && ((uintptr_t)dst[k] & 15) == 0;
        t.blk0[k] = (int)blocks;
        blocks += (row_bytes[k] + GATHER_CHUNK - 1) / GATHER_CHUNK;
        if (blocks > ((int64_t)1 << 30)) return DCD_ERR_BAD_ARG;
    }
    t.blk0[n_tables] = (int)blocks;
    t.count = n_tables;
    hipLaunchKernelGGL(gather_rows, dim3((unsigned)blocks, (unsigned)B), dim3(GATHER_THREADS), 0, stream, t, index);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}

}  // extern "C"
