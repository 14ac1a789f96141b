// images.hip -- the image half of the input pipeline on the device: decoded uint8 frames in, the network's input batch out.
//
// Replaces, per training sample of the reference: the image side of `RandomHorizontallyFlip`
// (DGDE/data/augmentations/augmentations.py:33-36), `KITTIDataset.pad_image` (DGDE/data/datasets/kitti.py:262-272), `ToTensor`
// and `Normalize` with its `TO_BGR` permutation (DGDE/data/transforms/transforms.py:14-30).  The reference pads the uint8
// canvas BEFORE it normalises, so the border holds (0 - mean) / std; and it normalises the RGB planes BEFORE it permutes them,
// so under TO_BGR output plane c carries source channel 2 - c normalised with THAT channel's mean / std.
//
// The kernel has no arithmetic of its own: every output value is one entry of a 3 x 256 fp32 table the caller built with the
// reference's own operations (dcd_amd/data/input_pipeline.py), so the result is bit-equal to the reference's by construction.
// It is pure traffic (uint8 in, 4x as many fp32 bytes out).  One thread owns four consecutive pixels of an output row in all
// three planes: three 16-byte stores, a wave writes 1 KiB contiguous per plane.  Its 12 source bytes are contiguous (a flip
// reverses the pixel order inside them, not the bytes of a pixel) but start at any byte offset (3-byte pixels, odd pad_x), so
// they come from the four aligned dwords that cover them, shifted into place with v_alignbyte; neighbouring lanes share those
// dwords through the L1.  Groups that straddle the image border, and input widths that are not a multiple of four (VEC = 1),
// take byte loads.  The table sits in LDS (3 KiB): smooth image content reads it mostly as broadcasts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dcd_hip.h"

namespace {

constexpr int IMG_THREADS = 256;
constexpr int IMG_REC = 5;          // int64 per image: byte offset, row pitch, height, width, flip

template <int VEC>
__global__ __launch_bounds__(IMG_THREADS) void preprocess_images(const uint8_t *__restrict__ src, int64_t src_bytes,
                                                                 const int64_t *__restrict__ images, const float *__restrict__ table,
                                                                 int in_h, int in_w, int to_bgr, float *__restrict__ out)
{
    __shared__ float lut[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += IMG_THREADS) lut[i] = table[i];
    __syncthreads();

    const int groups = in_w / VEC;                                   // VEC == 4 only when in_w % 4 == 0
    const int unit = blockIdx.x * IMG_THREADS + threadIdx.x;
    if (unit >= in_h * groups) return;
    const int b = blockIdx.y, y = unit / groups, x0 = (unit - y * groups) * VEC;

    const int64_t *rec = images + (int64_t)b * IMG_REC;
    const int64_t off = rec[0], pitch = rec[1];
    int h = (int)rec[2], w = (int)rec[3];
    const bool flip = rec[4] != 0;
    // a record that does not lie inside the source buffer, or an image larger than the canvas, reads nothing: all border
    if (rec[2] <= 0 || rec[3] <= 0 || rec[2] > in_h || rec[3] > in_w || off < 0 || pitch < 3 * rec[3] ||
        off + (rec[2] - 1) * pitch + 3 * rec[3] > src_bytes)
        h = w = 0;
    const int pad_x = (in_w - w) / 2, pad_y = (in_h - h) / 2;        // kitti.py:266-267
    const int sy = y - pad_y, c0 = x0 - pad_x;                        // source row; image column of the group's first pixel

    uint8_t px[VEC][3];                                               // [output pixel][source channel]
#pragma unroll
    for (int i = 0; i < VEC; ++i) px[i][0] = px[i][1] = px[i][2] = 0;

    if (sy >= 0 && sy < h) {
        const uint8_t *row = src + off + (int64_t)sy * pitch;
        bool done = false;
        if (VEC == 4 && c0 >= 0 && c0 + 3 < w) {
            // the 12 bytes of source pixels lo .. lo + 3, from the aligned dwords around them
            const int lo = flip ? w - 1 - (c0 + 3) : c0;
            const uint8_t *p = row + 3 * lo;
            const uint32_t sh = (uint32_t)((uintptr_t)p & 3);
            const uint8_t *a = p - sh;                                // 4-byte aligned; the 16 bytes from it must lie in src
            if (a >= src && a + 16 <= src + src_bytes) {
                const uint32_t *q = (const uint32_t *)a;
                const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3];
                const uint32_t e[3] = {__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
                                       __builtin_amdgcn_alignbyte(d3, d2, sh)};
#pragma unroll
                for (int j = 0; j < 4; ++j) {                         // source pixel lo + j -> output pixel j (flip: 3 - j)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int k = 3 * j + c;
                        const uint8_t v = (uint8_t)(e[k >> 2] >> (8 * (k & 3)));
                        if (flip) px[3 - j][c] = v; else px[j][c] = v;
                    }
                }
                done = true;
            }
        }
        if (!done) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const int col = c0 + i;
                if (col >= 0 && col < w) {
                    const uint8_t *p = row + 3 * (flip ? w - 1 - col : col);
                    px[i][0] = p[0]; px[i][1] = p[1]; px[i][2] = p[2];
                }
            }
        }
    }

    const int64_t plane = (int64_t)in_h * in_w;
    float *o = out + (int64_t)b * 3 * plane + (int64_t)y * in_w + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int sc = to_bgr ? 2 - c : c;                            // the SOURCE channel, whose mean / std apply
        if (VEC == 4) {
            float4 v = {lut[sc * 256 + px[0][sc]], lut[sc * 256 + px[1][sc]], lut[sc * 256 + px[2][sc]], lut[sc * 256 + px[3][sc]]};
            *(float4 *)(o + c * plane) = v;
        } else {
            o[c * plane] = lut[sc * 256 + px[0][sc]];
        }
    }
}

}  // namespace

extern "C" {

int dcd_preprocess_images(void *stream_, const uint8_t *src, int64_t src_bytes, const int64_t *images, const float *table, int B,
                          int in_h, int in_w, int to_bgr, float *out)
{
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (!src || !images || !table || !out || src_bytes <= 0) return DCD_ERR_BAD_ARG;
    if (B <= 0 || B > 65535 || in_h <= 0 || in_w <= 0 || (int64_t)in_h * in_w > (int64_t)1 << 30) return DCD_ERR_BAD_ARG;
    const bool vec = in_w % 4 == 0 && ((uintptr_t)out & 15) == 0;     // 16-byte stores need a 16-byte aligned batch
    const int units = in_h * (vec ? in_w / 4 : in_w);
    const dim3 grid((units + IMG_THREADS - 1) / IMG_THREADS, B);
    if (vec)
        hipLaunchKernelGGL(preprocess_images<4>, grid, dim3(IMG_THREADS), 0, stream, src, src_bytes, images, table, in_h, in_w, to_bgr, out);
    else
        hipLaunchKernelGGL(preprocess_images<1>, grid, dim3(IMG_THREADS), 0, stream, src, src_bytes, images, table, in_h, in_w, to_bgr, out);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}

}  // extern "C"
