// conv_direct_bf16.inc -- the ONE-product form (DCD_PREC_BF16) of the 3x3 / stride 1 / pad 1 convolution as a DIRECT implicit
// GEMM on v_mfma_f32_32x32x16_bf16 (included by conv.hip inside its anonymous namespace).
//
// Why not Winograd here: on the bf16 matrix pipe the multiplies F(2x2, 3x3) saves are worth nothing -- the Winograd kernel's
// matrix pipe is 10 % busy, its time is the input transform's vector and LDS instructions and two barriers per chunk between
// waves that each own one transform row (DESIGN.md R5.1).  The direct form has NO transform: an operand is a 16-byte LDS read.
//
//   y[k][r][x] = sum_c sum_{a,b} w[k][c][a][b] x[c][r + a - 1][x + b - 1]          (backward-data: the prepared weights are
//                                                                                    transposed and flipped, same kernel)
//   * workgroup = 4 waves, region = 4 P rows x 32 columns x 32 NB output channels; wave = P consecutive rows.
//   * per chunk of 16 contraction channels: the (4 P + 2) x 34 window is loaded as fp32 (buffer loads, out of range = 0),
//     rounded to bf16 ONCE (v_cvt_pk_bf16_f32) and stored as [channel half][row][column] 16-byte slots (8 channels of a pixel):
//     the B operand of (window row i, tap column b) is ONE ds_read_b128 at slot (i, lane & 31 + b) of plane lane >> 5 -- 32
//     consecutive slots, conflict free.  The chunk's weight slab [tap 9][ob NB][lane 64] x 16 bytes goes global -> LDS
//     directly (global_load_lds, two buffers, a chunk ahead) and from there into 36 NB registers at the top of the chunk.
//   * a window row feeds up to three output rows (a = 0, 1, 2): per chunk and wave 3 (P + 2) B reads + 9 NB A reads for
//     9 NB P matrix instructions of 32 cycles (P = 4, NB = 2: 36 reads of 8 LDS cycles for 2 304 matrix cycles per SIMD).
//   * the next chunk's window loads are in flight during the matrix phase (registers), committed between the two barriers.
//   * accumulators go straight to global memory (lane & 31 = column: 128-byte runs per channel), bias / residual added there;
//     a split contraction writes partial images exactly like the Winograd kernels (wino_sum_partials adds them).
// Channels beyond Cc (the last chunk of the 27-channel offset convolutions' backward-data call) need no mask: the whole byte
// offset of a load sits in its VGPR operand, the descriptor ends at the image's Cc H W floats, and a raw buffer load past the
// end returns zero (so does the out-of-image sentinel 0x7ffffff0 + anything below 2^31).  Requires (Cc + 16) H W < 2^29.

constexpr int DC_NT = 256;
constexpr int DC_OOB = 0x7ffffff0;

// 16-byte slots of the direct-layout weights of one direction
__host__ __device__ inline size_t dc_weight_slots(int Cc, int Kk)
{
    const int nb = Kk <= 32 ? 1 : 2;
    return (size_t)((Cc + DC_CH - 1) / DC_CH) * ((Kk + 32 * nb - 1) / (32 * nb)) * 9 * nb * 64;
}

// ud[z][chunk][tap = 3 a + b][ob][lane] = the lane's A operand: output channel z 32 NB + 32 ob + (lane & 31), contraction channels
// chunk 16 + 8 (lane >> 5) + 0..7, rounded to bf16 (nearest even).  mode as wino_prep_body.
template <int NB>
__device__ __forceinline__ void dc_prep_body(const float *__restrict__ w, unsigned *__restrict__ ud, int Cc, int Kk, int mode, int nchunk,
                                             int nz, int first, int step)
{
    // one thread per (z, chunk, ob, lane): the nine taps of its eight channels are 72 consecutive floats of w (forward; eight runs
    // of nine in the backward-data direction, read back to front) -> nine 16-byte slots
    const int n = nz * nchunk * NB * 64;
    for (int idx = first; idx < n; idx += step) {
        int r = idx;
        const int lane = r & 63; r >>= 6;
        const int ob = r % NB; r /= NB;
        const int ck = r % nchunk, z = r / nchunk;
        const int k = z * 32 * NB + ob * 32 + (lane & 31), cb = ck * DC_CH + 8 * (lane >> 5);
        float v[9][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = cb + e;
            const bool ok = k < Kk && c < Cc;
            const float *src = w + (mode == 0 ? ((size_t)k * Cc + c) : ((size_t)c * Kk + k)) * 9;
#pragma unroll
            for (int t = 0; t < 9; ++t) v[t][e] = ok ? src[mode == 0 ? t : 8 - t] : 0.f;
        }
        sp_u32x4 *dst = reinterpret_cast<sp_u32x4 *>(ud) + ((size_t)(z * nchunk + ck) * 9 * NB + ob) * 64 + lane;
#pragma unroll
        for (int t = 0; t < 9; ++t) dst[(size_t)t * NB * 64] = __builtin_bit_cast(sp_u32x4, sp_round8(v[t]));
    }
}

struct DirectPrep {
    unsigned *ud[2];
    int Cc[2], Kk[2];
};

// both directions of one layer (blockIdx.y = direction; a null pointer skips it)
__global__ void direct_prep_weights_both(const float *__restrict__ w, DirectPrep p)
{
    const int mode = blockIdx.y;
    if (!p.ud[mode]) return;
    const int Cc = p.Cc[mode], Kk = p.Kk[mode];
    const int nb = Kk <= 32 ? 1 : 2, nchunk = (Cc + DC_CH - 1) / DC_CH, nz = (Kk + 32 * nb - 1) / (32 * nb);
    const int first = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    if (nb == 2) dc_prep_body<2>(w, p.ud[mode], Cc, Kk, mode, nchunk, nz, first, step);
    else dc_prep_body<1>(w, p.ud[mode], Cc, Kk, mode, nchunk, nz, first, step);
}

// MANY layers in one launch (blockIdx.z = table entry, blockIdx.y = direction): the five-word entries of wino_prep_weights_table
// (weight, forward buffer, backward buffer, Cin, Cout), the buffers in this file's layout.
__global__ void direct_prep_weights_table(const long long *__restrict__ table)
{
    const long long *e = table + 5 * (size_t)blockIdx.z;
    const float *w = reinterpret_cast<const float *>(e[0]);
    const int mode = blockIdx.y;
    unsigned *ud = reinterpret_cast<unsigned *>(e[1 + mode]);
    if (!w || !ud) return;
    const int Cin = (int)e[3], Cout = (int)e[4];
    const int Cc = mode ? Cout : Cin, Kk = mode ? Cin : Cout;
    const int nb = Kk <= 32 ? 1 : 2, nchunk = (Cc + DC_CH - 1) / DC_CH, nz = (Kk + 32 * nb - 1) / (32 * nb);
    const int first = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    if (nb == 2) dc_prep_body<2>(w, ud, Cc, Kk, mode, nchunk, nz, first, step);
    else dc_prep_body<1>(w, ud, Cc, Kk, mode, nchunk, nz, first, step);
}

// MODE 0: a chunk's weights resident in registers (36 NB), window rows streamed;  1: the wave's 3 (P + 2) window operands resident,
// weights streamed tap by tap;  2: both streamed (a weight operand serves the P rows of its tap, a window operand one product per
// output block): 9 NB + 9 P LDS reads per 9 NB P products, and few enough registers for four waves per SIMD.
// (the second launch bound is HIP's: waves per SIMD the register allocation must leave room for)
// WX: waves along x -- the workgroup is 4 WX waves and owns 4 P rows x 32 WX columns.  The +-1 column halo costs two extra 128-byte
// lines per window row whatever the width: 3 lines for 1 at WX = 1, 4 for 2 at WX = 2 (the kernel's time at 96x320 is L2 traffic).
template <int NB, int P, int MODE, int WX>
__device__ __forceinline__ void dc_body(const float *__restrict__ x, const unsigned *__restrict__ wd, float *y, float *__restrict__ part,
                                        const float *__restrict__ bias, const float *residual, int Cc, int H, int W, int Kk, int tiles_x,
                                        int nchunk, int nz)
{
    constexpr int NT = DC_NT * WX;
    // window columns c0-4 .. c0+32 WX+3 (the +-1 halo inside 16-byte aligned groups of four pixels: dwordx4 loads -- with
    // dword loads the kernel was bound by the number of memory instructions its texture path had to walk lane by lane)
    constexpr int WR = 4 * P + 2, RS = 32 * WX + 8, RQ = RS / 4;
    constexpr int NSLOT = 2 * WR * RS;                                // 16-byte slots of the window: [half][row][column]
    constexpr int NITEM = 2 * WR * RQ;                                // staging items: 8 channels x 4 pixels
    constexpr int WSLAB = 9 * NB * 64;                                // 16-byte slots of one weight slab
    constexpr int KIN = (NITEM + NT - 1) / NT;
    constexpr int KW = (WSLAB + NT - 1) / NT;
    extern __shared__ __attribute__((aligned(16))) unsigned dlds[];   // window | two weight slabs
    sp_u32x4 *win = reinterpret_cast<sp_u32x4 *>(dlds);
    sp_u32x4 *wbuf = win + NSLOT;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wy = wave & 3, wx = wave >> 2;
    const int n = lane & 31, kg = lane >> 5;
    int bx = blockIdx.x, b = blockIdx.y;
    xcd_remap(bx, b);
    // (the nz ksplit workgroups of one window are launched far apart -- blockIdx.z is the slowest index; dealing them to one XCD
    // back to back instead was measured SLOWER: 64 -> 256 @ 96x320 115 -> 135 us)
    const int z = blockIdx.z % nz, ks = blockIdx.z / nz, ksplit = gridDim.z / nz;
    const int ty = bx / tiles_x, tx = bx - ty * tiles_x;
    const int r0 = ty * (4 * P), c0 = tx * (32 * WX);
    const int ck0 = (int)((int64_t)ks * nchunk / ksplit), ck1 = (int)((int64_t)(ks + 1) * nchunk / ksplit);
    const int HW = H * W;

    const __amdgpu_buffer_rsrc_t rx =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(x + (size_t)b * Cc * HW), 0, (int)((size_t)Cc * HW * 4), 0x00020000);
    int voff[KIN], slot[KIN];
#pragma unroll
    for (int k = 0; k < KIN; ++k) {
        const int e = tid + NT * k;
        const int half = e / (WR * RQ), rem = e - half * (WR * RQ);
        const int row = rem / RQ, q = rem - row * RQ;
        const int yy = r0 - 1 + row, xx = c0 - 4 + 4 * q;
        const bool ok = e < NITEM && yy >= 0 && yy < H && xx >= 0 && xx < W;          // W % 4 == 0: a group is inside or outside
        voff[k] = ok ? (8 * half * HW + yy * W + xx) * 4 : DC_OOB;
        slot[k] = e < NITEM ? (half * WR + row) * RS + 4 * q : -1;
    }
    f32x4 rin[KIN][8];
    auto issue_in = [&](int ck) {
        const int sb = ck * DC_CH * HW * 4;
#pragma unroll
        for (int k = 0; k < KIN; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                rin[k][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, voff[k] + (sb + j * HW * 4), 0, 0));
    };
    auto commit_in = [&]() {
#pragma unroll
        for (int k = 0; k < KIN; ++k)
            if (slot[k] >= 0) {
#pragma unroll
                for (int px = 0; px < 4; ++px) {
                    const float v[8] = {rin[k][0][px], rin[k][1][px], rin[k][2][px], rin[k][3][px],
                                        rin[k][4][px], rin[k][5][px], rin[k][6][px], rin[k][7][px]};
                    win[slot[k] + px] = __builtin_bit_cast(sp_u32x4, sp_round8(v));
                }
            }
    };
    const unsigned *wd_z = wd + (size_t)z * nchunk * WSLAB * 4;
    auto issue_w = [&](int ck, int buf) {
        const unsigned *src = wd_z + (size_t)ck * WSLAB * 4 + tid * 4;
        unsigned *dst = reinterpret_cast<unsigned *>(wbuf + buf * WSLAB) + wave * 256;
#pragma unroll
        for (int q = 0; q < KW; ++q)
            if (q * (NT / 64) + wave < 9 * NB)
                __builtin_amdgcn_global_load_lds(src + q * (NT * 4), (__attribute__((address_space(3))) void *)(dst + q * (NT * 4)), 16, 0, 0);
    };

    f32x16 acc[P][NB];
#pragma unroll
    for (int r = 0; r < P; ++r)
#pragma unroll
        for (int ob = 0; ob < NB; ++ob)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[r][ob][j] = 0.f;

    issue_w(ck0, 0);
    issue_in(ck0);
    commit_in();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const sp_u32x4 *brow = win + (kg * WR + wy * P) * RS + wx * 32 + n + 3;     // column c0 - 1 + lane
    for (int ck = ck0; ck < ck1; ++ck) {
        const int cur = (ck - ck0) & 1;
        const bool more = ck + 1 < ck1;
        const sp_u32x4 *wl = wbuf + cur * WSLAB + lane;
        if constexpr (MODE == 2) {
            if (more) {
                issue_w(ck + 1, cur ^ 1);
                issue_in(ck + 1);
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                sp_bf16x8 A[NB];
#pragma unroll
                for (int ob = 0; ob < NB; ++ob) A[ob] = __builtin_bit_cast(sp_bf16x8, wl[(t * NB + ob) * 64]);
#pragma unroll
                for (int r = 0; r < P; ++r) {
                    const sp_bf16x8 Bv = __builtin_bit_cast(sp_bf16x8, brow[(r + t / 3) * RS + t % 3]);
#pragma unroll
                    for (int ob = 0; ob < NB; ++ob) acc[r][ob] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[ob], Bv, acc[r][ob], 0, 0, 0);
                }
            }
        } else if constexpr (MODE == 1) {
            sp_bf16x8 Bv[P + 2][3];
#pragma unroll
            for (int i = 0; i < P + 2; ++i)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) Bv[i][dx] = __builtin_bit_cast(sp_bf16x8, brow[i * RS + dx]);
            if (more) {
                issue_w(ck + 1, cur ^ 1);
                issue_in(ck + 1);
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                sp_bf16x8 A[NB];
#pragma unroll
                for (int ob = 0; ob < NB; ++ob) A[ob] = __builtin_bit_cast(sp_bf16x8, wl[(t * NB + ob) * 64]);
#pragma unroll
                for (int r = 0; r < P; ++r)
#pragma unroll
                    for (int ob = 0; ob < NB; ++ob)
                        acc[r][ob] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[ob], Bv[r + t / 3][t % 3], acc[r][ob], 0, 0, 0);
            }
        } else {
            sp_bf16x8 A[9][NB];
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int ob = 0; ob < NB; ++ob) A[t][ob] = __builtin_bit_cast(sp_bf16x8, wl[(t * NB + ob) * 64]);
            if (more) {
                issue_w(ck + 1, cur ^ 1);
                issue_in(ck + 1);
            }
#pragma unroll
            for (int i = 0; i < P + 2; ++i) {
                sp_bf16x8 Bv[3];
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) Bv[dx] = __builtin_bit_cast(sp_bf16x8, brow[i * RS + dx]);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int r = i - a;
                    if (r < 0 || r >= P) continue;
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                        for (int ob = 0; ob < NB; ++ob)
                            acc[r][ob] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[a * 3 + dx][ob], Bv[dx], acc[r][ob], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                      // every wave is done with the window
        if (more) commit_in();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the next chunk's weights have landed
        __syncthreads();
    }

    float *y_b = (ks == 0 ? y : part + (size_t)(ks - 1) * gridDim.y * Kk * HW) + (size_t)b * Kk * HW;
    const float *r_b = (residual && ks == 0) ? residual + (size_t)b * Kk * HW : nullptr;
    const int col = c0 + wx * 32 + n;
    if (col >= W) return;
#pragma unroll
    for (int r = 0; r < P; ++r) {
        const int orow = r0 + wy * P + r;
        if (orow >= H) continue;
#pragma unroll
        for (int ob = 0; ob < NB; ++ob)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int k = z * 32 * NB + ob * 32 + (j & 3) + 8 * (j >> 2) + 4 * kg;
                if (k < Kk) {
                    const size_t o = (size_t)k * HW + (size_t)orow * W + col;
                    float v = acc[r][ob][j];
                    if (bias && ks == 0) v += bias[k];
                    if (r_b) v += r_b[o];
                    y_b[o] = v;
                }
            }
    }
}

template <int NB, int P, int MODE, int WX>
__global__ __launch_bounds__(DC_NT * WX) void conv3x3_direct_bf16(const float *__restrict__ x, const unsigned *__restrict__ wd, float *y,
                                                                  float *__restrict__ part, const float *__restrict__ bias,
                                                                  const float *residual, int Cc, int H, int W, int Kk, int tiles_x,
                                                                  int nchunk, int nz)
{
    dc_body<NB, P, MODE, WX>(x, wd, y, part, bias, residual, Cc, H, W, Kk, tiles_x, nchunk, nz);
}

// MODE 2 compiled for four waves per SIMD (128 registers)
template <int NB, int P, int WX>
__global__ __launch_bounds__(DC_NT * WX, 4) void conv3x3_direct_bf16_w4(const float *__restrict__ x, const unsigned *__restrict__ wd, float *y,
                                                                        float *__restrict__ part, const float *__restrict__ bias,
                                                                        const float *residual, int Cc, int H, int W, int Kk,
                                                                        int tiles_x, int nchunk, int nz)
{
    dc_body<NB, P, 2, WX>(x, wd, y, part, bias, residual, Cc, H, W, Kk, tiles_x, nchunk, nz);
}

// ---------------------------------------------------------------------------------------------
// Weight gradient of the same convolution in the one-product form, also DIRECT:
//   dW[k][c][a][b] = sum_{n,y,x} dY[n][k][y][x] X[n][c][y + a - 1][x + b - 1]
// is, per tap, a [Cout x pixels] x [pixels x Cin] product whose contraction runs over PIXELS -- and eight consecutive pixels of one
// channel are exactly what a lane's k-slot of v_mfma_f32_32x32x16_bf16 wants: both operands are read in their native NCHW order,
// no transform, no transpose.
//   * workgroup = 8 waves = the 2 x 2 (output block, input block) pairs of 64 output x 64 input channels x the two 16-pixel
//     halves of a strip's rows; a wave holds the nine taps of its 32 x 32 pair (144 accumulators) and walks the workgroup's
//     strips of 2 rows x 32 columns (the partition of wino_wrw3x3_f32: nblk blocks x S splits of the strip list, partial sums
//     to the workspace, one reduce launch); the two halves of a pair are added through LDS at the end.
//   * per strip X (64 ch x 4 rows x columns -4 .. 35) and dY (64 ch x 2 rows x 32) are loaded as fp32 dwordx4 (buffer loads,
//     out of range = 0), rounded to bf16 once and stored channel-major, pixel-contiguous: LDS channel strides 100 / 36 dwords
//     (4 x odd: the 16 lanes of a ds_read_b128 group cover all 64 banks).  Two LDS buffers, the next strip's loads in flight
//     during the products: ONE barrier per strip.
//   * operands: dY[k][row y][8 pixels] is one ds_read_b128; X[c][row][8 pixels + b - 1] for b = 0, 1, 2 comes from one aligned
//     ds_read_b128 plus the dword before and after and eight v_alignbit_b32 (a 16-bit funnel shift = one pixel).  A window row
//     feeds the taps a with y = row - a in {0, 1}: per strip and wave 14 LDS reads, 32 shifts, 18 matrix instructions.
//   * every address of the staging map that does not depend on the strip is computed ONCE (with 255 registers the compiler had
//     recomputed them per load in the registers of loads still in flight: a vmcnt wait per load, 188 us instead of 70).
constexpr int DW_NT = 512;
constexpr int DW_XS = 100;                         // dwords per X channel: 4 rows x 24 (48 bf16: columns -8 .. 39) + 4
constexpr int DW_GS = 36;                          // dwords per dY channel: 2 rows x 16 + 4
constexpr int DW_BUF = 64 * (DW_XS + DW_GS);       // dwords of one buffer
constexpr int DW_EX = 4 * 5 * 16 * 64;             // dwords of the final exchange between the two pixel halves
constexpr int DW_LDS = 2 * DW_BUF > DW_EX ? 2 * DW_BUF : DW_EX;

__global__ __launch_bounds__(DW_NT) void conv3x3_wrw_direct_bf16(const float *__restrict__ x, const float *__restrict__ gy,
                                                                  float *__restrict__ part, int Cin, int Cout, int B, int H, int W,
                                                                  int strips_x, int S, int ncg, int nblk)
{
    extern __shared__ __attribute__((aligned(16))) unsigned wlds[];   // [2][X 64 x DW_XS | dY 64 x DW_GS]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ln = lane & 31, h = lane >> 5;
    // eight waves: (output block kb, input block cb) x the 16-pixel half `seg` of a strip's rows
    const int pair = wave & 3, kb = pair >> 1, cb = pair & 1, seg = wave >> 2;
    int split, blk;
    {
        const int L = blockIdx.x;
        if ((S & 7) == 0) {
            const int xcd = L & 7, u = L >> 3;
            blk = u % nblk;
            split = (u / nblk) * 8 + xcd;
        } else {
            blk = L % nblk;
            split = L / nblk;
        }
    }
    const int og = blk / ncg, cg = blk - og * ncg;
    const int HW = H * W;
    const int tiles_y = (H + 1) >> 1;
    const int T = B * tiles_y * strips_x;
    const int t0 = (int)((int64_t)split * T / S), t1 = (int)((int64_t)(split + 1) * T / S);

    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(x), 0, (int)((size_t)B * Cin * HW * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(gy), 0, (int)((size_t)B * Cout * HW * 4), 0x00020000);
    constexpr int KX = 64 * 4 * 10 / DW_NT;        // 5 dwordx4 per thread
    constexpr int KG = 64 * 2 * 8 / DW_NT;         // 2
    // strip-invariant parts of the staging map: byte offset inside the strip's window (or out of range for a channel beyond the
    // tensor), window row / column group for the per-strip bounds test, LDS dword
    int xoff[KX], xrq[KX], xlds[KX], goff[KG], grq[KG], glds[KG];
#pragma unroll
    for (int k = 0; k < KX; ++k) {
        const int e = tid + DW_NT * k;
        const int ch = e / 40, r2 = e - ch * 40;
        const int row = r2 / 10, q = r2 - row * 10;
        xoff[k] = cg * 64 + ch < Cin ? (ch * HW + row * W + 4 * q) * 4 : DC_OOB;
        xrq[k] = row | (q << 4);
        xlds[k] = ch * DW_XS + row * 24 + 2 + 2 * q;                  // element 8 + 4 q - 4
    }
#pragma unroll
    for (int k = 0; k < KG; ++k) {
        const int e = tid + DW_NT * k;
        const int o = e >> 4, row = (e >> 3) & 1, q = e & 7;
        goff[k] = og * 64 + o < Cout ? (o * HW + row * W + 4 * q) * 4 : DC_OOB;
        grq[k] = row | (q << 4);
        glds[k] = 64 * DW_XS + o * DW_GS + row * 16 + 2 * q;
    }
    f32x4 rxv[KX], rgv[KG];
    auto issue = [&](int t) {
        const int b = t / (tiles_y * strips_x);
        const int rem = t - b * (tiles_y * strips_x);
        const int ty = rem / strips_x, sx = rem - ty * strips_x;
        const int y0 = 2 * ty, x0 = 32 * sx;
        const int bx_ = ((b * Cin + cg * 64) * HW + (y0 - 1) * W + x0 - 4) * 4;          // scalar parts (may be negative)
        const int bg_ = ((b * Cout + og * 64) * HW + y0 * W + x0) * 4;
#pragma unroll
        for (int k = 0; k < KX; ++k) {
            const int yy = y0 - 1 + (xrq[k] & 15), xx = x0 - 4 + 4 * (xrq[k] >> 4);
            const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
            const int voff = ok ? bx_ + xoff[k] : DC_OOB;              // an invalid channel: DC_OOB + bx_ stays out of range
            rxv[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, voff, 0, 0));
        }
#pragma unroll
        for (int k = 0; k < KG; ++k) {
            const bool ok = y0 + (grq[k] & 15) < H && x0 + 4 * (grq[k] >> 4) < W;
            const int voff = ok ? bg_ + goff[k] : DC_OOB;
            rgv[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rg, voff, 0, 0));
        }
    };
    auto commit = [&](unsigned *buf) {
#pragma unroll
        for (int k = 0; k < KX; ++k) {
            sp_u32x2 v;
            v.x = __builtin_bit_cast(unsigned, __builtin_convertvector(sp_f32x2{rxv[k].x, rxv[k].y}, sp_bf16x2));
            v.y = __builtin_bit_cast(unsigned, __builtin_convertvector(sp_f32x2{rxv[k].z, rxv[k].w}, sp_bf16x2));
            *reinterpret_cast<sp_u32x2 *>(buf + xlds[k]) = v;
        }
#pragma unroll
        for (int k = 0; k < KG; ++k) {
            sp_u32x2 v;
            v.x = __builtin_bit_cast(unsigned, __builtin_convertvector(sp_f32x2{rgv[k].x, rgv[k].y}, sp_bf16x2));
            v.y = __builtin_bit_cast(unsigned, __builtin_convertvector(sp_f32x2{rgv[k].z, rgv[k].w}, sp_bf16x2));
            *reinterpret_cast<sp_u32x2 *>(buf + glds[k]) = v;
        }
    };

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[t][j] = 0.f;

    if (t0 < t1) {
        issue(t0);
        commit(wlds);
    }
    for (int t = t0; t < t1; ++t) {
        const int cur = (t - t0) & 1;
        const bool more = t + 1 < t1;
        __syncthreads();                           // buffer `cur` is complete, nobody reads the other one any more
        if (more) issue(t + 1);
        const unsigned *xs = wlds + cur * DW_BUF + (cb * 32 + ln) * DW_XS + 4 + 4 * h + 8 * seg;     // element 8 + 16 seg + 8 h
        const unsigned *gs = wlds + cur * DW_BUF + 64 * DW_XS + (kb * 32 + ln) * DW_GS + 4 * h + 8 * seg;
        sp_bf16x8 A[2];
#pragma unroll
        for (int yl = 0; yl < 2; ++yl) A[yl] = __builtin_bit_cast(sp_bf16x8, *reinterpret_cast<const sp_u32x4 *>(gs + yl * 16));
#pragma unroll
        for (int xr = 0; xr < 4; ++xr) {
            const unsigned *p = xs + xr * 24;
            const sp_u32x4 d = *reinterpret_cast<const sp_u32x4 *>(p);
            const unsigned prev = p[-1], next = p[4];
            sp_u32x4 b0, b2;
            b0[0] = __builtin_amdgcn_alignbit(d[0], prev, 16);
            b0[1] = __builtin_amdgcn_alignbit(d[1], d[0], 16);
            b0[2] = __builtin_amdgcn_alignbit(d[2], d[1], 16);
            b0[3] = __builtin_amdgcn_alignbit(d[3], d[2], 16);
            b2[0] = b0[1];
            b2[1] = b0[2];
            b2[2] = b0[3];
            b2[3] = __builtin_amdgcn_alignbit(next, d[3], 16);
            const sp_bf16x8 Bv[3] = {__builtin_bit_cast(sp_bf16x8, b0), __builtin_bit_cast(sp_bf16x8, d), __builtin_bit_cast(sp_bf16x8, b2)};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int yl = xr - a;
                if (yl < 0 || yl > 1) continue;
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    acc[a * 3 + b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[yl], Bv[b], acc[a * 3 + b], 0, 0, 0);
            }
        }
        if (more) commit(wlds + (cur ^ 1) * DW_BUF);
    }

    // the two pixel halves of a pair meet in LDS (two rounds: taps 0-4, 5-8), then the sums go to part[blk][split][tap][k 64][c 64]
    float *ex = reinterpret_cast<float *>(wlds) + (size_t)pair * 5 * 16 * 64 + lane;
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        const int tl = round ? 5 : 0, tn = round ? 4 : 5;
        __syncthreads();
        if (seg == 1)
            for (int t = 0; t < tn; ++t)
#pragma unroll
                for (int j = 0; j < 16; ++j) ex[(t * 16 + j) * 64] = acc[tl + t][j];
        __syncthreads();
        if (seg == 0)
            for (int t = 0; t < tn; ++t)
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[tl + t][j] += ex[(t * 16 + j) * 64];
    }
    if (seg == 0) {
        float *dst = part + ((size_t)(blk * S + split) * 9) * 4096 + (size_t)(kb * 32 + 4 * h) * 64 + cb * 32 + ln;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int j = 0; j < 16; ++j) dst[(size_t)t * 4096 + ((j & 3) + 8 * (j >> 2)) * 64] = acc[t][j];
    }
}

// gw[k][c][tap] = sum over the splits of part[blk][split][tap][k][c].  Block = (blk, output channel k, tap row a): 64 input
// channels x 4 split groups; a thread adds every fourth split of its three taps (coalesced 256-byte rows, independent loads), the
// four groups meet in LDS in a fixed order (bitwise reproducible).
__global__ __launch_bounds__(256) void conv3x3_wrw_direct_reduce(const float *__restrict__ part, float *__restrict__ gw, int Cin, int Cout,
                                                                 int S, int ncg)
{
    __shared__ float sm[4][3][64];
    const int blk = blockIdx.z, og = blk / ncg, cg = blk - og * ncg;
    const int kl = blockIdx.x, a = blockIdx.y;
    const int cl = threadIdx.x & 63, sg = threadIdx.x >> 6;
    float r[3] = {0.f, 0.f, 0.f};
    const float *src = part + ((size_t)blk * S * 9 + 3 * a) * 4096 + kl * 64 + cl;
    for (int s = sg; s < S; s += 4)
#pragma unroll
        for (int b = 0; b < 3; ++b) r[b] += src[((size_t)s * 9 + b) * 4096];
#pragma unroll
    for (int b = 0; b < 3; ++b) sm[sg][b][cl] = r[b];
    __syncthreads();
    const int k = og * 64 + kl, c = cg * 64 + cl;
    if (sg == 0 && k < Cout && c < Cin) {
        float *dst = gw + ((size_t)k * Cin + c) * 9 + 3 * a;
#pragma unroll
        for (int b = 0; b < 3; ++b) dst[b] = ((sm[0][b][cl] + sm[1][b][cl]) + sm[2][b][cl]) + sm[3][b][cl];
    }
}
