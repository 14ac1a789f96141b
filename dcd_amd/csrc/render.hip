// render.hip -- the detections of a batch drawn on the device (include/dcd_hip.h, dcd_render_detections / dcd_render_primitives).
// The rule and its arithmetic are csrc/render_math.h.
//
// Two launches per batch:
//   render_setup   one workgroup per image, one thread per ground-truth slot or detection: the object's entries of the image's
//                  primitive table (fixed layout, rd_slots), the float ends for whoever asked, and -- an LDS integer max -- the
//                  index one past the image's last drawn entry.
//   render_raster  one workgroup per 32 x 32 tile of the CANVAS (the bytes outside the picture are this kernel's zeros).  The
//                  threads share the image's entries; an entry that reaches the tile is walked over the steps that do (closed
//                  form) and leaves its key -- (order + 1) << 13 | index -- in the tile's LDS words by integer max, which
//                  is commutative: the result is the serial painter's, whatever order the waves run in.  Then every pixel
//                  becomes its winner's colour, the frame's pixel, the bird's-eye background or 0 in an LDS byte row, and the
//                  rows go out as whole dwords between at most three single bytes at either end (a tile's bytes are its own:
//                  3 bytes per pixel and an odd width leave the rows unaligned, the canvas is not padded).
// No global atomics, no workspace beyond the table, nothing read back: two calls give the same bytes.
// LDS per workgroup: 4 KB of keys + 3 KB of bytes.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/dcd_hip.h"
#include "render_math.h"

namespace {

constexpr int SETUP_THREADS = 256;
constexpr int TILE = 32;
constexpr int RASTER_THREADS = 256;
static_assert(TILE * 3 / 4 + 6 <= 32, "a tile row is at most 32 store items: its dwords and three bytes at either end");

__global__ __launch_bounds__(SETUP_THREADS) void render_setup(const RdArgs a, int slots, int *__restrict__ table,
                                                              int *__restrict__ counts, float *__restrict__ ends)
{
    __shared__ int s_count;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_count = 0;
    __syncthreads();
    int w, h, flip;
    int64_t off, pitch;
    rd_frame(a.recs, a.staged_bytes, b, a.in_h, a.in_w, &w, &h, &off, &pitch, &flip);
    int *ent = table + (int64_t)b * slots * RD_ENTRY;
    float *f = ends ? ends + (int64_t)b * slots * 4 : nullptr;
    int last = 0;
    for (int obj = tid; obj < a.M + a.K; obj += SETUP_THREADS) {
        const int l = rd_object(a, b, obj, h, ent, f);
        last = l > last ? l : last;
    }
    if (last) atomicMax(&s_count, last);
    __syncthreads();
    if (tid == 0) counts[b] = s_count;
}

__global__ __launch_bounds__(RASTER_THREADS) void render_raster(const uint8_t *__restrict__ staged, uint64_t staged_bytes,
                                                                const int *__restrict__ table, const int *__restrict__ counts,
                                                                int stride, int in_h, int in_w, uint8_t *__restrict__ canvas)
{
    __shared__ uint32_t s_key[TILE * TILE];
    __shared__ uint8_t s_rgb[TILE][TILE * 3];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int CW = in_w + in_h;
    const int tx0 = blockIdx.x * TILE, ty0 = blockIdx.y * TILE;
    const int cx1 = (tx0 + TILE < CW ? tx0 + TILE : CW) - 1, cy1 = (ty0 + TILE < in_h ? ty0 + TILE : in_h) - 1;   // inclusive
    int w, h, flip;
    int64_t off, pitch;
    rd_frame((const int64_t *)staged, staged_bytes, b, in_h, in_w, &w, &h, &off, &pitch, &flip);
    const int *ent = table + (int64_t)b * stride * RD_ENTRY;

    for (int i = tid; i < TILE * TILE; i += RASTER_THREADS) s_key[i] = 0;
    __syncthreads();

    if (ty0 < h && tx0 < w + h) {                                       // the tile holds pixels of the picture
        int count = counts[b];
        count = count < 0 ? 0 : (count > stride ? stride : count);
        for (int i = tid; i < count; i += RASTER_THREADS) {
            int e[RD_ENTRY];
            const int4 *src = (const int4 *)(ent + (int64_t)i * RD_ENTRY);
            for (int q = 0; q < RD_ENTRY / 4; ++q) {
                const int4 v = src[q];
                e[4 * q] = v.x;
                e[4 * q + 1] = v.y;
                e[4 * q + 2] = v.z;
                e[4 * q + 3] = v.w;
            }
            if (!rd_entry_ok(e)) continue;
            const int left = e[0] ? w : 0, pw = e[0] ? h : w;            // the panel's left edge on the canvas and its width
            const int rx0 = tx0 - left > 0 ? tx0 - left : 0, rx1 = cx1 - left < pw - 1 ? cx1 - left : pw - 1;
            const int ry1 = cy1 < h - 1 ? cy1 : h - 1;
            const uint32_t key = rd_key(e, i);
            rd_raster(e, rx0, ty0, rx1, ry1, [&](int x, int y) { atomicMax(&s_key[(y - ty0) * TILE + (x + left - tx0)], key); });
        }
    }
    __syncthreads();

    for (int p = tid; p < TILE * TILE; p += RASTER_THREADS) {
        const int ly = p / TILE, lx = p % TILE, X = tx0 + lx, Y = ty0 + ly;
        uint8_t r = 0, g = 0, bl = 0;
        if (Y < h && X < w + h) {
            const uint32_t key = s_key[p];
            if (key) {
                const int *e = ent + (int64_t)(key & (RD_MAX_ENTRIES - 1)) * RD_ENTRY;
                r = (uint8_t)e[7];
                g = (uint8_t)e[8];
                bl = (uint8_t)e[9];
            } else if (X < w) {
                const uint8_t *px = staged + off + (int64_t)Y * pitch + 3 * (int64_t)(flip ? w - 1 - X : X);
                r = px[0];
                g = px[1];
                bl = px[2];
            } else {
                r = g = bl = RD_BACKGROUND;
            }
        }
        s_rgb[ly][3 * lx] = r;
        s_rgb[ly][3 * lx + 1] = g;
        s_rgb[ly][3 * lx + 2] = bl;
    }
    __syncthreads();

    // the tile's rows: bytes [a, e) of the canvas each -- single bytes up to the first dword boundary, dwords, single bytes
    const int tw = cx1 - tx0 + 1, th = cy1 - ty0 + 1;
    for (int item = tid; item < th * 32; item += RASTER_THREADS) {
        const int ly = item / 32, j = item % 32;
        const uint64_t a = (((uint64_t)b * in_h + (ty0 + ly)) * CW + tx0) * 3, e = a + 3 * (uint64_t)tw;
        uint64_t first = (a + 3) & ~(uint64_t)3;
        first = first > e ? e : first;
        const int head = (int)(first - a), nd = (int)((e - first) / 4), tail = (int)(e - first) - 4 * nd;
        const uint8_t *src = s_rgb[ly];
        if (j < nd) {
            const int o = head + 4 * j;
            const uint32_t v = (uint32_t)src[o] | ((uint32_t)src[o + 1] << 8) | ((uint32_t)src[o + 2] << 16) | ((uint32_t)src[o + 3] << 24);
            *(uint32_t *)(canvas + first + 4 * (uint64_t)j) = v;
        } else if (j < nd + head) {
            const int o = j - nd;
            canvas[a + o] = src[o];
        } else if (j < nd + head + tail) {
            const int o = head + 4 * nd + (j - nd - head);
            canvas[a + o] = src[o];
        }
    }
}

bool raster_args_ok(const void *staged, uint64_t staged_bytes, const void *table, const void *counts, const void *canvas, int B,
                    int stride, int in_h, int in_w)
{
    if (!staged || !table || !counts || !canvas) return false;
    if (B < 1 || B > 65535 || stride < 1 || stride > RD_MAX_ENTRIES || in_h < 1 || in_w < 1 || in_h > 16384 || in_w > 16384) return false;
    if (staged_bytes < (uint64_t)B * 40) return false;
    if (((uintptr_t)staged & 7) || ((uintptr_t)table & 15) || ((uintptr_t)canvas & 3) || ((uintptr_t)counts & 3)) return false;
    return true;
}

int launch_raster(hipStream_t stream, const uint8_t *staged, uint64_t staged_bytes, const int *table, const int *counts, int B,
                  int stride, int in_h, int in_w, uint8_t *canvas)
{
    const dim3 grid((unsigned)((in_w + in_h + TILE - 1) / TILE), (unsigned)((in_h + TILE - 1) / TILE), (unsigned)B);
    hipLaunchKernelGGL(render_raster, grid, dim3(RASTER_THREADS), 0, stream, staged, staged_bytes, table, counts, stride, in_h, in_w,
                       canvas);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}

}  // namespace

extern "C" int dcd_render_slots(int M, int K, int nk)
{
    if (M < 0 || K < 1 || nk < 0 || M > 4096 || K > 128 || nk > 128) return -1;
    const int slots = rd_slots(M, K, nk);
    return slots > RD_MAX_ENTRIES ? -1 : slots;
}

extern "C" int dcd_render_detections(void *stream_, const uint8_t *staged, size_t staged_bytes, const float *rows, const float *aux,
                                     const float *kpts2d, const float *image_table, const float *gt_dims, const float *gt_locs,
                                     const float *gt_rotys, const uint8_t *gt_mask, int B, int K, int nk, int M, int in_h, int in_w,
                                     double det_threshold, double vis_threshold, int *table, int *counts, float *ends, uint8_t *canvas)
{
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    const int slots = dcd_render_slots(M, K, nk);
    if (slots < 1) return DCD_ERR_BAD_ARG;
    if (!rows || !aux || !image_table || (nk > 0 && !kpts2d)) return DCD_ERR_BAD_ARG;
    if (M > 0 && (!gt_dims || !gt_locs || !gt_rotys || !gt_mask)) return DCD_ERR_BAD_ARG;
    if (det_threshold != det_threshold || vis_threshold != vis_threshold) return DCD_ERR_BAD_ARG;
    if (!raster_args_ok(staged, staged_bytes, table, counts, canvas, B, slots, in_h, in_w)) return DCD_ERR_BAD_ARG;
    RdArgs a;
    a.B = B, a.K = K, a.nk = nk, a.M = M;
    a.det_threshold = (float)det_threshold, a.vis_threshold = (float)vis_threshold;
    a.rows = rows, a.aux = aux, a.k2 = kpts2d, a.table = image_table;
    a.gt_dims = gt_dims, a.gt_locs = gt_locs, a.gt_rotys = gt_rotys, a.gt_mask = gt_mask;
    a.recs = (const int64_t *)staged, a.staged_bytes = staged_bytes;
    a.in_h = in_h, a.in_w = in_w;
    hipLaunchKernelGGL(render_setup, dim3((unsigned)B), dim3(SETUP_THREADS), 0, stream, a, slots, table, counts, ends);
    if (hipGetLastError() != hipSuccess) return DCD_ERR_LAUNCH;
    return launch_raster(stream, staged, staged_bytes, table, counts, B, slots, in_h, in_w, canvas);
}

extern "C" int dcd_render_primitives(void *stream_, const uint8_t *staged, size_t staged_bytes, const int *table, const int *counts,
                                     int B, int stride, int in_h, int in_w, uint8_t *canvas)
{
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (!raster_args_ok(staged, staged_bytes, table, counts, canvas, B, stride, in_h, in_w)) return DCD_ERR_BAD_ARG;
    return launch_raster(stream, staged, staged_bytes, table, counts, B, stride, in_h, in_w, canvas);
}
