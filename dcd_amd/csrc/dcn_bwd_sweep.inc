// dcn_bwd_sweep.inc -- ONE-PASS DCNv2 backward for the 3x3 / stride 1 / pad 1 / dil 1 / one-group layers with Cout <= 64
// (round 3).  Replaces, for those layers, the three passes of rounds 1-2 (inverse lists + gather grad_input, grad_offset/mask,
// grad_weight: `W^T dY` computed twice, the corners gathered twice) -- the reference's per-sample loop of
// cuda/dcn_v2_cuda.cu:259-336 (GEMM -> col2im_coord -> col2im -> im2col -> GEMM) -- by one kernel in which
//
//   dcol[p, c] = sum_o dY[o, p] W[o, c, t]            one MFMA block per (16 pixels, tap, 16 channels), computed ONCE
//   grad_offset / grad_mask  from dcol and the four bilinear corners            (in registers)
//   grad_input               dcol * mask * bilinear weights added into an LDS window of the input gradient
//   grad_weight              dY x (mask * bilinear sample), the sample built from the SAME four corner reads
//
// Shape of the work.  A workgroup is ONE wave (no barrier anywhere).  It owns 16 input channels and a strip of 16 output
// pixels in x, and sweeps down the rows of its segment of the image.  Lane = (pixel quarter q = lane >> 4, channel c = lane & 15)
// -- the D layout of v_mfma_f32_16x16x4_f32 with M = pixels, N = channels: register r of the accumulator is pixel 4q + r.
//   * Every channel plane of the window belongs to exactly one lane column, and the wave is its only writer, so the
//     grad_input scatter is a plain LDS read-modify-write -- no atomics (measured this round, tools/micro/lds_atomic_rate.hip:
//     ds_add_f32 retires one LANE per 3 clocks per CU, 193 clk per wave instruction whatever the addresses; a plain
//     ds_write_b32 takes 7).  The four quarters of one instruction hold pixels 4 apart; if two of them could touch the same
//     cell (offsets differing by >= 2 px over 4 px -- decided per row, tap and pixel step when the sampling state is built)
//     that step's read-modify-write runs in two rounds, even quarters then odd ones (round 4; round 3 redid the whole tap
//     with LDS atomics).
//   * The window is a RING of 9 input rows x 24 columns (rows y-4 .. y+4 of the pixel row y in flight, columns x0-4 .. x0+19:
//     everything a sample displaced by less than TL_NEAR = 3 px can touch), x and its gradient interleaved ([c][cell][x, g])
//     so that the two corners of a row are ONE ds_read2_b64.  Advancing a row retires one ring row: its gradient is added to
//     grad_input with global atomics (24 x 16 values per row; the strips' halos overlap, like the reference's atomicAdd,
//     cuda/dcn_v2_im2col_cuda.cu:249) and the slot receives input row y+5.  Halo overhead 24/16 in x, none in y.
//   * The tap weights W[o, c, t] of the wave's 16 channels stay in registers for the whole sweep (144 VGPRs), the
//     grad_weight accumulators too (144): one wave per SIMD, 4 per CU.
//   * grad_offset / grad_mask are sums over all input channels: each 16-channel wave writes its partial sums to a scratch
//     plane and `dcn_sweep_reduce_coord` adds the planes in a fixed order (bit-reproducible); grad_weight partials are
//     summed by `dcn_sweep_reduce_dw`.
// Samples displaced by TL_NEAR px or more (outside the window) are taken one by one after the row's taps: corners from global
// memory, input gradient by global atomics (round 4; rounds 1-3 left them to the generic kernels' far-only pass over listed
// 32-pixel tiles).  When more than 1 in 64 offset coordinates is far the call goes to the generic kernels altogether.
//
// Algorithmic bytes per call (SURVEY 8d) are unchanged; what this kernel moves beyond them: the 1.5x halo of x, the partial
// planes (27 * B * HW floats per 16 channels, written once and read once) and the grad_weight partials.

#ifndef SW_ABL_TAPS
#define SW_ABL_TAPS 9                             // timing experiments: fewer taps per row (results wrong)
#endif
#ifdef SW_ABL_NOMFMA                              // timing experiment: one v_fma per matrix instruction (dependencies kept)
__device__ __forceinline__ f32x4 sw_fake_mfma(float a, float b, f32x4 c) { c.x = fmaf(a, b, c.x); c.y += a; c.z += b; c.w = fmaf(a, b, c.w); return c; }
#define SW_MFMA(a, b, c) sw_fake_mfma(a, b, c)
#else
#define SW_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0)
#endif
constexpr int SW_WW = 24;                         // window columns
constexpr int SW_RING = 9;                        // window rows
constexpr int SW_CELLS = SW_RING * SW_WW;         // 216
constexpr int SW_PLANE = SW_CELLS + 3;            // cells 216 .. 218: always-zero x / dummy gradient (invalid samples point here)
constexpr int SW_ZERO = SW_CELLS;

// Wp[ck][t][lane][s] = W[o = 4 s + (lane >> 4)][c = 16 ck + (lane & 15)][t], s < 16 nob (nob = blocks of 64 outputs): the lane's
// B operands of the k-steps of a tap are 64 nob contiguous bytes -- four 16-byte loads per tap and output block instead of
// sixteen dword loads
__device__ __forceinline__ void sweep_prep_weights_body(const float *__restrict__ w, float *__restrict__ wp, const Geom &g, int nck, int nob,
                                                        int bid, int nb)
{
    const int n = nck * SW_W_FLOATS * nob;
    const int ns = 16 * nob;
    for (int idx = bid * blockDim.x + threadIdx.x; idx < n; idx += nb * blockDim.x) {
        int r = idx;
        const int s = r % ns; r /= ns;
        const int lane = r & 63; r >>= 6;
        const int t = r % 9, ck = r / 9;
        const int o = 4 * s + (lane >> 4), c = ck * SW_CH + (lane & 15);
        wp[idx] = (o < g.Co && c < g.C) ? w[((size_t)o * g.C + c) * 9 + t] : 0.f;
    }
}

// Split-bf16 form (DCD_PREC_BF16X3): Wq[ck][t][kh][part][lane][d] (kh < 2 nob), dword d = bf16 pair (k = 2d, 2d+1) of
// part(W[o = 32 kh + 8 (lane >> 4) + k][c = 16 ck + (lane & 15)][t]), part 0 = hi = rne(w), part 1 = lo = rne(w - hi): the B operand
// of v_mfma_f32_16x16x32_bf16 (lane holds B[k = 8 (lane >> 4) + 0..7][n = lane & 15]); one 16-byte load per (tap, kh, part).
__device__ __forceinline__ void sweep_prep_weights_bf16_body(const float *__restrict__ w, unsigned *__restrict__ wq, const Geom &g, int nck,
                                                             int nob, int bid, int nb)
{
    const int n = nck * SW_W_FLOATS * nob;
    for (int idx = bid * blockDim.x + threadIdx.x; idx < n; idx += nb * blockDim.x) {
        int r = idx;
        const int d = r & 3; r >>= 2;
        const int lane = r & 63; r >>= 6;
        const int part = r & 1; r >>= 1;
        const int kh = r % (2 * nob); r /= 2 * nob;
        const int t = r % 9, ck = r / 9;
        const int c = ck * SW_CH + (lane & 15);
        float v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int o = 32 * kh + 8 * (lane >> 4) + 2 * d + e;
            v[e] = (o < g.Co && c < g.C) ? w[((size_t)o * g.C + c) * 9 + t] : 0.f;
        }
        unsigned hi, lo;
        split_pair(v[0], v[1], hi, lo);
        wq[idx] = part ? lo : hi;
    }
}

// Round 4: the call's small launches before the sweep folded into two (they were four: generic weight layouts, zero fill, sweep
// weight layout, offset scan -- ~5 us of dependent-launch latency each, 16 layers a step).
//   A: blocks [0, nb_gen) prepare Wf / Wb (the generic kernels' layouts: only read when the call is handed to them), the rest the
//      sweep's Wp; block 0 also resets the call's device scalars (the scan of launch B accumulates into them).
//   B: blocks [0, nb_zero) zero-fill the gradients the sweep / its reductions accumulate into, the rest scan the offsets.
__global__ __launch_bounds__(256) void dcn_sweep_prologue_a(const float *__restrict__ w, float *__restrict__ wf, float *__restrict__ wb,
                                                           float *__restrict__ wp, unsigned *__restrict__ scal, Geom g, int nck, int nob,
                                                           int split, int nb_gen, unsigned far_limit)
{
    if (blockIdx.x == 0 && threadIdx.x < 4) scal[threadIdx.x] = threadIdx.x == 3 ? (FAR_BY_COUNT | (FAR_COUNT_PIVOT - far_limit)) : 0u;
    if ((int)blockIdx.x < nb_gen) prep_weights_body(w, wf, wb, g, blockIdx.x, nb_gen);
    else if (split) sweep_prep_weights_bf16_body(w, (unsigned *)wp, g, nck, nob, blockIdx.x - nb_gen, gridDim.x - nb_gen);
    else sweep_prep_weights_body(w, wp, g, nck, nob, blockIdx.x - nb_gen, gridDim.x - nb_gen);
}

__global__ __launch_bounds__(256) void dcn_sweep_prologue_b(ZeroRanges z, int nb_zero, const float *__restrict__ off, int64_t noff,
                                                           unsigned *__restrict__ scal, int HoWo, int tiles_per_img)
{
    if ((int)blockIdx.x < nb_zero) zero_ranges_body(z, blockIdx.x, nb_zero);
    else offset_absmax_body(off, noff, scal, HoWo, 18, tiles_per_img, nullptr, nullptr, blockIdx.x - nb_zero, gridDim.x - nb_zero);
}

typedef short sw_s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned sw_u32x2 __attribute__((ext_vector_type(2)));
// 16 nob dwords of a lane = [kh][part][4 dwords] -> the bf16x8 operand (kh, part)
template <int NV>
__device__ __forceinline__ bf16x8 sw_op8(const float (&d)[NV], int kh, int part)
{
    const int b = kh * 8 + part * 4;
    const u32x4 v = {__float_as_uint(d[b]), __float_as_uint(d[b + 1]), __float_as_uint(d[b + 2]), __float_as_uint(d[b + 3])};
    return __builtin_bit_cast(bf16x8, v);
}
// 16 nob fp32 values [kh][8] -> in place [kh][hi 4 dwords | lo 4 dwords] (bf16 pairs, even k in the low half)
template <int NV>
__device__ __forceinline__ void sw_split16(float (&d)[NV])
{
#pragma unroll
    for (int kh = 0; kh < NV / 8; ++kh) {
        unsigned h[4], l[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) split_pair(d[kh * 8 + 2 * e], d[kh * 8 + 2 * e + 1], h[e], l[e]);
#pragma unroll
        for (int e = 0; e < 4; ++e) { d[kh * 8 + e] = __uint_as_float(h[e]); d[kh * 8 + 4 + e] = __uint_as_float(l[e]); }
    }
}
// four fp32 values -> {hi pair 0, hi pair 1, lo pair 0, lo pair 1} as bit patterns
__device__ __forceinline__ f32x4 sw_split4(const f32x4 v)
{
    unsigned h0, l0, h1, l1;
    split_pair(v.x, v.y, h0, l0);
    split_pair(v.z, v.w, h1, l1);
    return f32x4{__uint_as_float(h0), __uint_as_float(h1), __uint_as_float(l0), __uint_as_float(l1)};
}
// one-product forms (DCD_PREC_BF16): operands rounded to bf16, no low halves (the hi slots of the same register layouts)
template <int NV>
__device__ __forceinline__ void sw_round16(float (&d)[NV])
{
#pragma unroll
    for (int kh = 0; kh < NV / 8; ++kh) {
        unsigned h[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = round_pair(d[kh * 8 + 2 * e], d[kh * 8 + 2 * e + 1]);
#pragma unroll
        for (int e = 0; e < 4; ++e) d[kh * 8 + e] = __uint_as_float(h[e]);
    }
}
__device__ __forceinline__ f32x4 sw_round4(const f32x4 v)
{
    return f32x4{__uint_as_float(round_pair(v.x, v.y)), __uint_as_float(round_pair(v.z, v.w)), 0.f, 0.f};
}
__device__ __forceinline__ f32x4 sw_mfma16(float a0, float a1, float b0, float b1, f32x4 c)
{
    const sw_u32x2 a = {__float_as_uint(a0), __float_as_uint(a1)}, b = {__float_as_uint(b0), __float_as_uint(b1)};
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(sw_s16x4, a), __builtin_bit_cast(sw_s16x4, b), c, 0, 0, 0);
}
// grad_weight of one tap, split form: D[o][c] += dY[o][px 0..15] col[px][c] with K = the sixteen pixels of the row step
// (lane: k = 4 (lane >> 4) + r -- exactly the pixel 4 q + r the lane holds); small terms first
template <bool ONE = false>
__device__ __forceinline__ f32x4 sw_dw_split(const f32x4 &dy_split, const f32x4 &col_split, f32x4 c)
{
    if (!ONE) {
        c = sw_mfma16(dy_split.z, dy_split.w, col_split.x, col_split.y, c);      // lo * hi
        c = sw_mfma16(dy_split.x, dy_split.y, col_split.z, col_split.w, c);      // hi * lo
    }
    c = sw_mfma16(dy_split.x, dy_split.y, col_split.x, col_split.y, c);      // hi * hi
    return c;
}

__device__ __forceinline__ float sw_dpp_quad_xor1(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
}
__device__ __forceinline__ float sw_dpp_quad_xor2(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
}
__device__ __forceinline__ float sw_dpp_row_ror4(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x124, 0xF, 0xF, true));
}
__device__ __forceinline__ float sw_dpp_row_ror8(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));
}
// lane j of a row of 16 receives the value of lane j + 4 (lanes 12..15: zero)
__device__ __forceinline__ int sw_dpp_row_shl4(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x104, 0xF, 0xF, true); }

// Sums of four per-lane values P[0..3] over the 16 lanes of each quarter: afterwards lane j of the quarter holds the total of
// P[j & 3] (11 VALU instead of 16: the first two levels halve the number of live registers).
__device__ __forceinline__ float sw_reduce4(const float (&P)[4], bool bit0, bool bit1)
{
    const float a01 = bit0 ? P[1] : P[0], b01 = bit0 ? P[0] : P[1];
    const float a23 = bit0 ? P[3] : P[2], b23 = bit0 ? P[2] : P[3];
    const float x01 = a01 + sw_dpp_quad_xor1(b01);
    const float x23 = a23 + sw_dpp_quad_xor1(b23);
    const float a = bit1 ? x23 : x01, b = bit1 ? x01 : x23;
    float y = a + sw_dpp_quad_xor2(b);
    y += sw_dpp_row_ror4(y);
    y += sw_dpp_row_ror8(y);
    return y;
}

// uniform base (SGPR pair) + 32-bit per-lane byte offset: keeps the address arithmetic of the row loop on the scalar unit and
// ONE offset register per access pattern instead of a 64-bit pointer per load (hoisted out of the row loop they spilled)
__device__ __forceinline__ f32x4 sw_ldg4(const float *base, unsigned byte_off)
{
    return *reinterpret_cast<const f32x4 *>(reinterpret_cast<const char *>(base) + byte_off);
}
__device__ __forceinline__ void sw_stg(float *base, unsigned byte_off, float v)
{
    *reinterpret_cast<float *>(reinterpret_cast<char *>(base) + byte_off) = v;
}

#ifdef SW_PROFILE
// timing experiment: shader-clock stamps of one wave (block SW_PROFILE_BLOCK), read back through dcd_debug_sweep_profile
__device__ unsigned long long sw_prof_buf[2048];
#define SW_STAMP(slot) do { if (prof_on && (slot) < 2048) { const unsigned long long tt = __builtin_amdgcn_s_memtime(); if (lane == 0) sw_prof_buf[(slot)] = tt; } } while (0)
#else
#define SW_STAMP(slot) do { } while (0)
#endif

struct SweepArgs {
    const float *in, *off, *msk, *wp, *gy;
    float *gin, *cpart, *dwpart;
    float *col;                                    // DWK = false: the masked samples [b][c * 9 + t][p] for the grad_weight product
    const unsigned *far_scal;
    Geom g;
    int nstrip, nseg, seg_rows, nck, nv;
    int nslot;                                     // waves of the launch (multiple of 8 * nck): a wave takes units id, id + nslot, ...
};

// Four INDEPENDENT waves per workgroup (no barrier, no shared data): a workgroup's waves are dealt to the CU's four SIMDs one
// each, which single-wave workgroups are not -- two of those can land on one SIMD while another idles, and this kernel, one
// wave per SIMD by its register count, then runs at half speed there.
constexpr int SW_WAVES = 4;
constexpr int SW_ST = 8;                          // floats per state-table entry
constexpr int SW_LDS_FLOATS = SW_CH * SW_PLANE * 2 + 9 * 16 * SW_ST + 9 * 16 * 4;   // per wave: ring | state table | fix-up states

// PREC = DCD_PREC_F32: exact fp32 (v_mfma_f32_16x16x4_f32).  PREC = DCD_PREC_BF16X3: both contractions on the bf16 matrix cores
// with split operands (hi*hi + hi*lo + lo*hi, fp32 accumulate, ~2^-16 per product): dcol as 6 x v_mfma_f32_16x16x32_bf16 per
// tap, grad_weight as 12 x v_mfma_f32_16x16x16_bf16 per tap (K = the row step's 16 pixels) -- the matrix work leaves the vector
// lanes (the f32-input MFMA shares them: DESIGN.md R3.2), what remains is the kernel's vector / LDS instruction stream.
// Sampling, coordinate gradients and the window update stay fp32.
//
// NOB = blocks of 64 outputs the dcol product contracts over (Cout <= 64 NOB; round 4: 2 and 4 for the Cout 128 / 256 layers,
// which rounds 2-3 ran as column buffer -> GEMM -> col2im / coordinate kernels -> column buffer -> GEMM).  DWK: grad_weight
// inside this kernel (the 144 accumulators of ONE block of 64 outputs are all a wave can hold: NOB = 1 only).  DWK = false:
// the wave writes its masked samples m * val -- the B operand it would have fed to the grad_weight MFMAs -- to
// col[b][c * 9 + t][p], 16 bytes per lane and tap (four consecutive pixels), and grad_weight is ONE batched product
// dY x col^T afterwards (sgemm_f32.inc); grad_input / grad_offset / grad_mask still leave this kernel finished, nothing of the
// backward's data half goes through a buffer any more.
template <int PREC, int NOB, bool DWK>
__global__ __launch_bounds__(64 * SW_WAVES) void dcn_bwd_sweep(SweepArgs a)
{
    // PREC = DCD_PREC_BF16: the split form's layouts and instruction shapes with the low halves left out -- ONE product of bf16-rounded
    // operands per pair (mixed precision, MODEL.FP16)
    constexpr bool SPLIT = PREC != DCD_PREC_F32;
    constexpr bool ONE = PREC == DCD_PREC_BF16;
    constexpr int NS = 16 * NOB;                     // k-steps (f32) / operand dwords (split) of one tap's dcol product
    static_assert(!DWK || NOB == 1, "grad_weight accumulators of more than 64 outputs do not fit a wave");
    const Geom &g = a.g;
    if (far_dominated(a.far_scal, g.B * ((g.HoWo + 31) / 32))) return;      // the generic kernels do the whole job instead
    extern __shared__ __attribute__((aligned(16))) float sw_lds[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // uniform for the compiler too (else every address below is per lane)
    float *const ring = sw_lds + wave * SW_LDS_FLOATS;                        // [c][cell][x, g]
    float *const stt = ring + SW_CH * SW_PLANE * 2;
    float *const stt2 = stt + 9 * 16 * SW_ST;
    // state table: [tap][pixel]{pos, lh, lw, m | m w1..w4}: everything of a sample that does not depend on the channel is computed
    // ONCE per (pixel, tap) when the row's table is built -- in this layout every lane of a quarter would otherwise redo it.
    // (Round 5: the four products m hw, m lw, m hh, m lh that rounds 3-4 kept for the coordinate gradients are gone -- those
    // gradients are d m (bot - top) and d m (ex + lh (fx - ex)), terms the sample value needs anyway: one LDS read and three vector
    // instructions less per pixel step.)  stt2: {image coordinates, lh, lw, m} of the row's far samples (far loop after the taps).
    const int lane = threadIdx.x & 63;
    const int q = lane >> 4, j = lane & 15;
    const bool bit0 = lane & 1, bit1 = lane & 2;
#ifdef SW_PROFILE
    const bool prof_on = blockIdx.x == 300 && threadIdx.x < 64;
    int prof_slot = 0;
#endif

    // work unit: the nck chunk-waves of one (image, segment, strip) sit 8 ids apart.  Putting them into ONE workgroup (same CU:
    // shared L1 / L2 for the dY rows, offsets and mask that every chunk-wave reads) was measured and is SLOWER (64->64 0.985 vs
    // 0.970 ms, 128->64 0.561 vs 0.533, same box; -DSW_UNIT_PER_WG): the kernel is bound by instruction issue, not by traffic
    // (PMC: 573 MB per call against 160 MB algorithmic, L2 hit 0.55), and four waves marching through the same addresses collide.
    // A wave is PERSISTENT over its units (id, id + nslot, ...: same channel chunk, since nslot is a multiple of 8 * nck): the
    // grad_weight accumulators live across them -- one partial per wave instead of one per unit (70 MB of partials per 64->64 call
    // before) -- and the launch is one round of resident waves instead of 1.9.
    const int id0 = blockIdx.x * SW_WAVES + wave;
    const int ck = (id0 % (8 * a.nck)) >> 3;
    f32x4 accw[9][4];                              // DWK = false: never live
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) accw[t][ob] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};          // grad_bias partial (chunk 0): o = 16 ob + j, this lane's four pixels per row
    const int H = g.H, W = g.W, HW = g.H * g.W;
    for (int id = id0;; id += a.nslot) {
    const int grp_ = id / (8 * a.nck), rem_ = id - grp_ * (8 * a.nck);
    const int v = grp_ * 8 + (rem_ & 7);
    if (v >= a.nv) break;
    const int b = v / (a.nstrip * a.nseg), r2 = v - b * (a.nstrip * a.nseg);
    const int seg = r2 / a.nstrip, strip = r2 - seg * a.nstrip;
    const int x0 = strip * SW_PX, y0 = seg * a.seg_rows;
    const int y1 = min(y0 + a.seg_rows, g.H);

    const float *in_c = a.in + ((size_t)b * g.C + (size_t)ck * SW_CH) * HW;
    float *gin_c = a.gin + ((size_t)b * g.C + (size_t)ck * SW_CH) * HW;
    // Global operands go through buffer instructions: descriptor (uniform base + byte count) in SGPRs, ONE 32-bit lane-offset
    // register per access pattern, the row / plane part as a scalar offset.  A lane that must not access memory carries an
    // out-of-range offset (loads return 0, stores are dropped): no divergent branches in the tap loop, no 64-bit per-lane
    // addresses (hoisted out of the row loop as flat addresses they spilled).  Byte counts run to the END of each tensor: dY rows
    // o >= Cout of a padded block read the next image's values (finite) and meet zero weights.
    constexpr int SW_OOB = 0x7ffffff0;
    const size_t img = (size_t)HW * 4;
    const __amdgpu_buffer_rsrc_t r_gy = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(a.gy + (size_t)b * g.Co * HW), 0, (int)((size_t)(g.B - b) * g.Co * img), 0x00020000);
    const __amdgpu_buffer_rsrc_t r_off = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.off + (size_t)b * 18 * HW), 0, (int)(18 * img), 0x00020000);
    const __amdgpu_buffer_rsrc_t r_msk = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.msk + (size_t)b * 9 * HW), 0, (int)(9 * img), 0x00020000);
    const __amdgpu_buffer_rsrc_t r_cp = __builtin_amdgcn_make_buffer_rsrc(a.cpart + ((size_t)ck * g.B + b) * 27 * HW, 0, (int)(27 * img), 0x00020000);
    const int cleft = g.C - ck * SW_CH;                        // channels of this chunk that exist
    const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(in_c), 0, (int)((size_t)(cleft < SW_CH ? cleft : SW_CH) * img), 0x00020000);

    // ---- tap weights: B operands of the dcol product (16 per tap and lane, one coalesced 256-byte row each).  All nine taps
    // resident would need 144 registers on top of the 144 grad_weight accumulators (the compiler spills); they are re-read
    // per tap from L1 / L2 instead, one tap ahead of their use.
    // buffer loads: descriptor in SGPRs, ONE lane-offset register, tap / k-step as scalar + immediate offsets (as flat loads
    // the compiler hoisted 144 per-lane 64-bit addresses out of the row loop and spilled them)
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(a.wp + (size_t)ck * SW_W_FLOATS * NOB), 0, SW_W_FLOATS * NOB * 4, 0x00020000);
    auto load_w = [&](int t, float (&w)[NS]) {
        if (SPLIT) {                                            // [kh][part] x one 16-byte load: w[kh * 8 + part * 4 + d]
#pragma unroll
            for (int u = 0; u < 4 * NOB; ++u) {
                if (ONE && (u & 1)) continue;                       // the low halves are not used
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, lane * 16 + u * 1024, t * 4096 * NOB, 0);
#pragma unroll
                for (int d = 0; d < 4; ++d) w[u * 4 + d] = __uint_as_float(v[d]);
            }
        } else {
#pragma unroll
            for (int u = 0; u < 4 * NOB; ++u) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, lane * 64 * NOB + u * 16, t * 4096 * NOB, 0);
#pragma unroll
                for (int d = 0; d < 4; ++d) w[u * 4 + d] = __uint_as_float(v[d]);
            }
        }
    };
    // dcol += dY^T W of one tap: all of it (prologue / fix-up) or the share of pixel step r (pipelined pass).
    // DWK = false: the k-steps alternate between TWO accumulators (c, c2; summed when the tap is handed over): a
    // v_mfma_f32_16x16x4_f32 issues every 32 clocks but its result is ready for a dependent one after 40, and without the
    // grad_weight MFMAs in between a single chain of 32 / 64 would wait 8 clocks per link.
    auto dcol_part2 = [&](f32x4 &c, f32x4 &c2, const float (&dy)[NS], const float (&w)[NS], int r) {
        constexpr int KS[5] = {0, 6 * NOB, 11 * NOB, 16 * NOB, 16 * NOB};
#pragma unroll
        for (int s = 0; s < NS; ++s)
            if (r < 0 || (s >= KS[r] && s < KS[r + 1])) {
                if (s & 1) c2 = SW_MFMA(dy[s], w[s], c2);
                else c = SW_MFMA(dy[s], w[s], c);
            }
    };
    auto dcol_part = [&](f32x4 c, const float (&dy)[NS], const float (&w)[NS], int r) {
        if (ONE) {
            // one product per kh (2 NOB of them), dealt to the steps 0..2
#pragma unroll
            for (int i = 0; i < 2 * NOB; ++i)
                if (r < 0 || i % 3 == r)
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sw_op8(dy, i, 0), sw_op8(w, i, 0), c, 0, 0, 0);
        } else if (SPLIT) {
            // per kh three products (dY part, W part), small terms first: 6 NOB products, 2 NOB per step 0..2
            constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};
#pragma unroll
            for (int i = 0; i < 6 * NOB; ++i)
                if (r < 0 || i / (2 * NOB) == r)
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sw_op8(dy, i / 3, PA[i % 3]), sw_op8(w, i / 3, PB[i % 3]), c, 0, 0, 0);
        } else {
            constexpr int KS[5] = {0, 6 * NOB, 11 * NOB, 16 * NOB, 16 * NOB};
#pragma unroll
            for (int s = 0; s < NS; ++s)
                if (r < 0 || (s >= KS[r] && s < KS[r + 1])) c = SW_MFMA(dy[s], w[s], c);
        }
        return c;
    };
    // ---- ring: all zero, then input rows y0-4 .. y0+4
    {
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
        for (int e = lane; e < SW_CH * SW_PLANE * 2 / 4; e += 64) reinterpret_cast<f32x4 *>(ring)[e] = z4;
    }
    // one ring row = 16 channels x 6 float4: element e = lane + 64 k, k = 0, 1 (second half: lanes 0..31)
    int rl_off[2];                                                 // lane offsets of the two float4 of a window row (x0 - 4 folded in)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int e = lane + 64 * k;
        const int ch = e / 6, qq = e - ch * 6;
        const int xx = x0 - 4 + 4 * qq;
        rl_off[k] = (e < 96 && ch < cleft && xx >= 0 && xx < W) ? (ch * HW + xx) * 4 : SW_OOB;
    }
    auto row_load = [&](int yy, f32x4 (&rx)[2]) {
        const bool rowv = yy >= 0 && yy < H;                       // uniform
#pragma unroll
        for (int k = 0; k < 2; ++k)
            rx[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_in, rowv ? rl_off[k] : SW_OOB, rowv ? yy * W * 4 : 0, 0));
    };
    auto row_store = [&](int slot, const f32x4 (&rx)[2]) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int e = lane + 64 * k;
            const int ch = e / 6, qq = e - ch * 6;
            if (e < 96) {
                float *d = ring + (ch * SW_PLANE + slot * SW_WW + 4 * qq) * 2;
                d[0] = rx[k].x; d[2] = rx[k].y; d[4] = rx[k].z; d[6] = rx[k].w;
            }
        }
    };
    // slot of input row yy: (yy + 4) mod 9
    for (int yy = y0 - 4; yy <= y0 + 4; ++yy) {
        f32x4 rx[2];
        row_load(yy, rx);
        row_store((yy + 4) % SW_RING, rx);
    }

    // ---- per-row operands
    const bool pxv = x0 + j < W;                                   // this lane's pixel (as "lane = pixel") exists
    const bool q4v = x0 + 4 * q < W;                               // the lane's quarter of four pixels exists (W % 4 == 0)
    const int dyo_off = q4v ? (j * HW + x0 + 4 * q) * 4 : SW_OOB;
    // A operand of dcol.  f32: d[s] = dY[o = 4 s + q][x0 + j] (k-step s).  split: d[kh * 8 + i] = dY[o = 32 kh + 8 q + i][x0 + j],
    // converted in place by sw_split16 once the loads have landed.
    const int dyp_off = pxv ? ((SPLIT ? 8 * q : q) * HW + x0 + j) * 4 : SW_OOB;
    auto load_dyp = [&](int y, float (&d)[NS]) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int o0 = SPLIT ? 32 * (s >> 3) + (s & 7) : 4 * s;
            d[s] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r_gy, dyp_off, (o0 * HW + y * W) * 4, 0));
        }
    };
    auto load_dyo = [&](int y, f32x4 (&d)[4]) {                    // A operand of grad_weight: dY[o = 16 ob + j][x0 + 4 q + r]
#pragma unroll
        for (int ob = 0; ob < 4; ++ob)
            d[ob] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_gy, dyo_off, (16 * ob * HW + y * W) * 4, 0));
    };
    struct Raw { float oh[3], ow[3], m[3]; };
    const int roff_o = pxv ? (2 * q * HW + x0 + j) * 4 : SW_OOB, roff_m = pxv ? (q * HW + x0 + j) * 4 : SW_OOB;
    auto load_raw = [&](int y, Raw &r) {                           // lane = (tap 4 p + q, pixel j), p = 0, 1, 2; taps >= 9: out of range -> 0
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const bool tv = 4 * p + q < 9;
            r.oh[p] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r_off, tv ? roff_o : SW_OOB, (8 * p * HW + y * W) * 4, 0));
            r.ow[p] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r_off, tv ? roff_o : SW_OOB, ((8 * p + 1) * HW + y * W) * 4, 0));
            r.m[p] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r_msk, tv ? roff_m : SW_OOB, (4 * p * HW + y * W) * 4, 0));
        }
    };

    float dyp[NS], dyp_n[NS];
    f32x4 dyo[4], dyo_n[4];
    Raw raw, raw_n;
    load_dyp(y0, dyp);
    if (DWK) load_dyo(y0, dyo);
    load_raw(y0, raw);
    if (DWK && ck == 0) {
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) bsum[ob] += (dyo[ob].x + dyo[ob].y) + (dyo[ob].z + dyo[ob].w);
    }
    if (SPLIT) {
        if (ONE) sw_round16(dyp); else sw_split16(dyp);
        if (DWK) {
#pragma unroll
            for (int ob = 0; ob < 4; ++ob) dyo[ob] = ONE ? sw_round4(dyo[ob]) : sw_split4(dyo[ob]);
        }
    }
    // DWK = false: the masked samples of a tap leave as one 16-byte store per lane: col[b][(16 ck + j) * 9 + t][y * W + x0 + 4 q ..+3]
    const __amdgpu_buffer_rsrc_t r_col = __builtin_amdgcn_make_buffer_rsrc(
        DWK ? a.gin : a.col + ((size_t)b * g.C + (size_t)ck * SW_CH) * 9 * HW, 0, (int)((size_t)(cleft < SW_CH ? cleft : SW_CH) * 9 * img), 0x00020000);
    const int col_off = q4v ? (j * 9 * HW + x0 + 4 * q) * 4 : SW_OOB;
    auto col_store = [&](int t, int y, const float (&cv)[4]) {
        const u32x4 v = {__float_as_uint(cv[0]), __float_as_uint(cv[1]), __float_as_uint(cv[2]), __float_as_uint(cv[3])};
        __builtin_amdgcn_raw_buffer_store_b128(v, r_col, col_off, (t * HW + y * W) * 4, 0);
    };

    // dcol of (row, tap 0), one tap ahead of its use
    constexpr bool TWO = !DWK && !SPLIT;                           // two dcol chains (see dcol_part2)
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
    // tap weights rotate through THREE register sets: during tap t the dcol product of tap t + 1 reads set (t + 1) % 3 and the
    // weights of tap t + 2 are loaded into set (t + 2) % 3 -- the period divides the nine taps, so the assignment is the same in
    // every row and no set is ever copied (rounds 3-4: wcur = wnxt after every tap, 16 v_mov per tap).  Two sets are live at a time.
    float wr[3][NS];
    load_w(0, wr[0]);
    if (TWO) dcol_part2(acc, acc2, dyp, wr[0], -1);
    else acc = dcol_part(acc, dyp, wr[0], -1);
    load_w(1, wr[1]);                                               // weights of the NEXT tap's dcol (computed during tap 0)

    float pend_col = 0.f;                                          // mask * sample of the pixel step whose grad_weight MFMAs are pending
    float dyo_p3[4] = {0.f, 0.f, 0.f, 0.f};
    const int cp_off = (j < 4 && x0 + 4 * q + j < W) ? (x0 + 4 * q + j) * 4 : SW_OOB;       // lanes 0..3 of a quarter publish its sums
    char *const lane_plane = reinterpret_cast<char *>(ring) + j * (SW_PLANE * 8);      // this lane's channel plane (bytes)
    int s0 = y0 % SW_RING;                                         // slot of input row y - 4

    for (int y = y0; y < y1; ++y) {
        const bool more = y + 1 < y1;
#ifdef SW_PROFILE
        prof_slot = (y - y0) * 64;
        SW_STAMP(prof_slot + 0);
#endif
        // ---- requests for the next row (consumed at the end of this one)
        f32x4 rx[2];
        row_load(y + 5, rx);
        if (more) { load_dyp(y + 1, dyp_n); if (DWK) load_dyo(y + 1, dyo_n); load_raw(y + 1, raw_n); }
        else {
#pragma unroll
            for (int s = 0; s < NS; ++s) dyp_n[s] = 0.f;
#pragma unroll
            for (int ob = 0; ob < 4; ++ob) dyo_n[ob] = f32x4{0.f, 0.f, 0.f, 0.f};
        }

        // ---- sampling state of the row's 16 x 9 (pixel, tap) pairs -> LDS table; collision test for the quarters
        unsigned long long cmask = 0ull;                           // bit 4 t + r: pixel step r of tap t has quarters that meet in a cell
        unsigned long long fm[3];                                  // far samples of the row: bit 16 q' + j of fm[p] = (tap 4 p + q', pixel j)
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int t = 4 * p + q;
            const int ky = t / 3, kx = t - ky * 3;
            const float oh = raw.oh[p], ow = raw.ow[p];
            const float hf = (float)(y - 1 + ky) + oh, wf = (float)(x0 + j - 1 + kx) + ow;
            const bool inimg = t < 9 && pxv && hf > -1.f && wf > -1.f && hf < (float)H && wf < (float)W;
            const bool nearb = fabsf(oh) < TL_NEAR && fabsf(ow) < TL_NEAR;
            const bool sv = inimg && nearb;
            // a sample displaced by TL_NEAR px or more lies outside the window: the pipelined pass sees an invalid state for it
            // (zero contributions) and the far loop after the taps takes it from global memory
            const bool fv = inimg && !nearb;
            fm[p] = __ballot(fv);
            const float hlf = floorf(hf), wlf = floorf(wf);
            const int yl = (int)hlf, xl = (int)wlf;
            int st = s0 + (yl - (y - 4));                          // ring slot of the upper row
            st = st >= SW_RING ? st - SW_RING : st;
            int sb = st + 1;
            sb = sb >= SW_RING ? 0 : sb;
            const int col = xl - (x0 - 4);
            const int pt = sv ? st * SW_WW + col : SW_ZERO, pb = sv ? sb * SW_WW + col : SW_ZERO;
            f32x4 e;
            e.x = __uint_as_float((unsigned)(pt * 8) | ((unsigned)(pb * 8) << 16));
            e.y = sv ? hf - hlf : 0.f;
            e.z = sv ? wf - wlf : 0.f;
            e.w = sv ? raw.m[p] : 0.f;
            // pixels j and j + 4 share an instruction (quarters q, q + 1): their 2 x 2 footprints must not meet in a cell.  A pixel
            // STEP (tap, r) where they could (a jump of >= 2 px over 4 px) is skipped by the pipelined pass -- the state of its
            // four pixels there is "invalid" -- and done afterwards by the fix-up loop, whose read-modify-write runs in two rounds,
            // even quarters then odd ones (quarters 8 px apart cannot meet: both samples are displaced by less than TL_NEAR =
            // 3 px).  Round 3 skipped the whole TAP and redid it with LDS atomics: ~4000 clk per tap, every third tap at 1 px.
            const int xe = sv ? xl : 100000 + 16 * j;
            const int xn = sw_dpp_row_shl4(xe);
            const bool bad = j < 12 && (unsigned)(xn - xe + 1) <= 2u;
            const unsigned long long bm = __ballot(bad);
            const unsigned m16q = (unsigned)(bm >> (16 * q)) & 0xffffu;           // this lane's tap: bit 4 q' + r = pixels 4 q' + r, + 4
            const bool stepbad = (((m16q | (m16q >> 4) | (m16q >> 8)) >> (j & 3)) & 1u) != 0u;
            if (t < 9) {
                const f32x4 inval = {__uint_as_float((unsigned)(SW_ZERO * 8) | ((unsigned)(SW_ZERO * 8) << 16)), 0.f, 0.f, 0.f};
                const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
                const float lh = e.y, lw = e.z, m = e.w, hh = 1.f - lh, hw = 1.f - lw;
                const f32x4 e2 = {m * (hh * hw), m * (hh * lw), m * (lh * hw), m * (lh * lw)};
                f32x4 *dst = reinterpret_cast<f32x4 *>(stt + (t * 16 + j) * SW_ST);
                dst[0] = stepbad ? inval : e;
                dst[1] = stepbad ? zero4 : e2;
                // far sample: {(yl + 1) | (xl + 1) << 16, lh, lw, m} -- image coordinates of the upper left corner (-1 .. H - 1)
                const f32x4 ef = {__uint_as_float((unsigned)(yl + 1) | ((unsigned)(xl + 1) << 16)), hf - hlf, wf - wlf, raw.m[p]};
                *reinterpret_cast<f32x4 *>(stt2 + (t * 16 + j) * 4) = fv ? ef : e;
            }
#pragma unroll
            for (int tp = 0; tp < 4; ++tp)
                if (4 * p + tp < 9) {
                    const unsigned m16 = (unsigned)(bm >> (16 * tp)) & 0xffffu;        // bit 4 q + r: pixels 4 q + r and 4 q + r + 4
                    cmask |= (unsigned long long)((m16 | (m16 >> 4) | (m16 >> 8)) & 15u) << (4 * (4 * p + tp));
                }
        }

        SW_STAMP(prof_slot + 1);
        // ---- the nine taps = 36 pixel steps, software-pipelined by hand.  With ONE wave per SIMD nothing hides a latency
        // unless the instruction stream does, so a step is cut in two phases:
        //   FRONT  the step's window values have arrived: four FMAs (gradient increment, prepared earlier) and the two
        //          ds_write2 of the read-modify-write, then AT ONCE the two ds_read2_b64 of the NEXT step (LDS keeps a wave's
        //          order, so the reads see this step's writes);
        //   HEAVY  everything else of the step runs in the shadow of those reads: 9/9/8/6 MFMAs (the dcol product of tap t + 1
        //          and the grad_weight MFMAs of the previous step), the sample value, the three coordinate products, the
        //          increments of the next step, one 16-lane reduction of tap t - 1; sampling states of tap t + 1 and weights
        //          of tap t + 2 are requested here, one tap ahead.
        // sched_barrier pins the phases, sched_group_barrier asks for MFMA / VALU alternation inside HEAVY.
        auto cp_store = [&](int plane, float v) {                // plane: 0..17 grad_offset, 18..26 grad_mask
#ifdef SW_ABL_NOCP
            if (v == 123.456f)
#endif
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r_cp, cp_off, (plane * HW + y * W) * 4, 0);
        };
        {
            struct Step { f32x4 e0, e2; };                         // state of one pixel step (this lane's quarter)
            auto ld_state = [&](int k) {                           // k = 4 tap + r
                const f32x4 *src = reinterpret_cast<const f32x4 *>(stt + ((k >> 2) * 16 + 4 * q + (k & 3)) * SW_ST);
                Step sx;
                sx.e0 = src[0]; sx.e2 = src[1];
                return sx;
            };
            float Pm_p[4], Ph_p[4], Pw_p[4];                       // products of the previous tap, reduced during this one
#pragma unroll
            for (int r = 0; r < 4; ++r) { Pm_p[r] = 0.f; Ph_p[r] = 0.f; Pw_p[r] = 0.f; }
            f32x4 d4 = TWO ? acc + acc2 : acc;                     // dcol of tap 0 (computed during the previous row / prologue)
            acc = f32x4{0.f, 0.f, 0.f, 0.f};
            acc2 = f32x4{0.f, 0.f, 0.f, 0.f};
            Step cur = ld_state(0), nxt = ld_state(1);
            float d_cur = d4[0];
            char *pT = lane_plane + (__float_as_uint(cur.e0.x) & 0xffffu), *pB = lane_plane + (__float_as_uint(cur.e0.x) >> 16);
            f32x2 t0 = reinterpret_cast<const f32x2 *>(pT)[0], t1 = reinterpret_cast<const f32x2 *>(pT)[1];
            f32x2 b0 = reinterpret_cast<const f32x2 *>(pB)[0], b1 = reinterpret_cast<const f32x2 *>(pB)[1];
#pragma unroll
            for (int t = 0; t < SW_ABL_TAPS; ++t) {
                float (&wcur)[NS] = wr[(t + 1) % 3];
                float (&wnxt)[NS] = wr[(t + 2) % 3];
                float Pm[4], Ph[4], Pw[4], cv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = 4 * t + r;
                    const bool has_next = k + 1 < 36;
                    // ---------------- FRONT: finish this step's read-modify-write, start the next step's reads
                    __builtin_amdgcn_sched_barrier(0);
                    reinterpret_cast<float *>(pT)[1] = t0.y + d_cur * cur.e2.x;
                    reinterpret_cast<float *>(pT)[3] = t1.y + d_cur * cur.e2.y;
                    reinterpret_cast<float *>(pB)[1] = b0.y + d_cur * cur.e2.z;
                    reinterpret_cast<float *>(pB)[3] = b1.y + d_cur * cur.e2.w;
                    const float v1 = t0.x, v2 = t1.x, v3 = b0.x, v4 = b1.x;
                    const Step me = cur;
                    const float d = d_cur;
                    if (has_next) {
                        if (r == 3) {                                                 // dcol of tap t + 1: its chain ended in step 2
                            d4 = TWO ? acc + acc2 : acc;
                            acc = f32x4{0.f, 0.f, 0.f, 0.f};
                            acc2 = f32x4{0.f, 0.f, 0.f, 0.f};
                        }
                        d_cur = d4[r == 3 ? 0 : r + 1];
                        cur = nxt;
                        pT = lane_plane + (__float_as_uint(cur.e0.x) & 0xffffu);
                        pB = lane_plane + (__float_as_uint(cur.e0.x) >> 16);
                        t0 = reinterpret_cast<const f32x2 *>(pT)[0]; t1 = reinterpret_cast<const f32x2 *>(pT)[1];
                        b0 = reinterpret_cast<const f32x2 *>(pB)[0]; b1 = reinterpret_cast<const f32x2 *>(pB)[1];
                    }
                    __builtin_amdgcn_sched_barrier(0);
#ifdef SW_PROFILE
                    if (SW_PROFILE == 2) SW_STAMP(prof_slot + 16 + k);
#endif
                    // ---------------- HEAVY: in the shadow of those reads
                    if (k + 2 < 36) nxt = ld_state(k + 2);
                    if (r == 0) load_w(t + 2 < 9 ? t + 2 : t + 2 - 9, wnxt);       // weights of tap t + 2's dcol (used during tap t + 1)
                    // dcol of tap t + 1 (tap 0 of the next row after tap 8) in three shares (f32: k-steps 0-5 | 6-10 | 11-15, split: two
                    // of the six products each): the chain ends in step 2 because step 3's front already takes the first step of
                    // tap t + 1 from it
                    if (r < 3) {
                        if (TWO) {
                            if (t < 8) dcol_part2(acc, acc2, dyp, wcur, r);
                            else dcol_part2(acc, acc2, dyp_n, wcur, r);
                        } else {
                            acc = t < 8 ? dcol_part(acc, dyp, wcur, r) : dcol_part(acc, dyp_n, wcur, r);
                        }
                    }
                    if (DWK && !SPLIT) {
                        // grad_weight of the previous pixel step: D[o][c] += dY[o][pixel 4 q' + r] * col[pixel 4 q' + r][c]
#pragma unroll
                        for (int ob = 0; ob < 4; ++ob) {
                            if (r > 0) accw[t][ob] = SW_MFMA(dyo[ob][r > 0 ? r - 1 : 0], pend_col, accw[t][ob]);
                            else if (t > 0) accw[t > 0 ? t - 1 : 0][ob] = SW_MFMA(dyo[ob][3], pend_col, accw[t > 0 ? t - 1 : 0][ob]);
                            else accw[8][ob] = SW_MFMA(dyo_p3[ob], pend_col, accw[8][ob]);
                        }
                    }
                    const float lh = me.e0.y, lw = me.e0.z, m = me.e0.w;
                    const float ex = v2 - v1, fx = v4 - v3;
                    const float top = v1 + lw * ex, bot = v3 + lw * fx;       // the sample's two row interpolants
                    const float dv = bot - top;                                // d val / d h
                    const float val = top + lh * dv;
                    const float dm = d * m;
                    Pm[r] = d * val;
                    Ph[r] = dm * dv;
                    Pw[r] = dm * (ex + lh * (fx - ex));                        // d val / d w = hh ex + lh fx
                    pend_col = m * val;
                    if (SPLIT || !DWK) cv[r] = pend_col;
                    if (!DWK) {
                        if (r == 3) col_store(t, y, cv);           // the tap's four masked samples of this lane
                    } else if (SPLIT) {
                        if (r == 3) {                              // grad_weight of this tap: K = the step's sixteen pixels
                            const f32x4 cv4 = {cv[0], cv[1], cv[2], cv[3]};
                            const f32x4 cs = ONE ? sw_round4(cv4) : sw_split4(cv4);
#pragma unroll
                            for (int ob = 0; ob < 4; ++ob) accw[t][ob] = sw_dw_split<ONE>(dyo[ob], cs, accw[t][ob]);
                        }
                    }
                    // next row's dcol operand: converted once its loads have landed (before tap 8 uses it)
                    if (SPLIT && t == 7 && r == 3) { if (ONE) sw_round16(dyp_n); else sw_split16(dyp_n); }
                    if (t > 0) {                                   // coordinate gradients of tap t - 1
                        if (r == 1) cp_store(2 * (t - 1), sw_reduce4(Ph_p, bit0, bit1));
                        if (r == 2) cp_store(2 * (t - 1) + 1, sw_reduce4(Pw_p, bit0, bit1));
                        if (r == 3) cp_store(18 + t - 1, sw_reduce4(Pm_p, bit0, bit1));
                    }
                    // MFMAs of this step: the dcol share (6 / 5 / 5 / 0 per output block) + four of grad_weight, spread over the step's
                    // ~30 vector instructions (three per MFMA with ten of them; two / one with 12 / 24: NOB = 2 / 4)
                    constexpr int VPM = DWK ? 3 : (NOB == 2 ? 2 : 1);
#pragma unroll
                    for (int i = 0; i < (SPLIT ? 0 : (r == 0 ? 6 * NOB : (r == 3 ? 0 : 5 * NOB)) + (DWK ? 4 : 0)); ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     // one MFMA
                        __builtin_amdgcn_sched_group_barrier(0x002, VPM, 0);   // VPM VALU
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) { Pm_p[r] = Pm[r]; Ph_p[r] = Ph[r]; Pw_p[r] = Pw[r]; }
#ifdef SW_PROFILE
                if (SW_PROFILE == 1) SW_STAMP(prof_slot + 2 + t);
#endif
            }
            __builtin_amdgcn_sched_barrier(0);
            // tap 8's coordinate gradients
            cp_store(16, sw_reduce4(Ph_p, bit0, bit1));
            cp_store(17, sw_reduce4(Pw_p, bit0, bit1));
            cp_store(26, sw_reduce4(Pm_p, bit0, bit1));
        }
        // grad_weight of one tap from four masked samples per lane, for a run-time tap (registers cannot be indexed: nine copies)
        auto add_dw = [&](int t, const float (&colv)[4]) {
            const f32x4 colv4 = {colv[0], colv[1], colv[2], colv[3]};
            const f32x4 cs = ONE ? sw_round4(colv4) : (SPLIT ? sw_split4(colv4) : f32x4{0.f, 0.f, 0.f, 0.f});
#define SW_FIX_CASE(TT)                                                                                                 \
    case TT:                                                                                                            \
        if (SPLIT) {                                                                                                    \
            _Pragma("unroll") for (int ob = 0; ob < 4; ++ob) accw[TT][ob] = sw_dw_split<ONE>(dyo[ob], cs, accw[TT][ob]); \
        } else {                                                                                                        \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) _Pragma("unroll") for (int ob = 0; ob < 4; ++ob)              \
                accw[TT][ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(dyo[ob][r], colv[r], accw[TT][ob], 0, 0, 0);         \
        }                                                                                                               \
        break;
            switch (t) {
                SW_FIX_CASE(0) SW_FIX_CASE(1) SW_FIX_CASE(2) SW_FIX_CASE(3) SW_FIX_CASE(4) SW_FIX_CASE(5) SW_FIX_CASE(6) SW_FIX_CASE(7)
                SW_FIX_CASE(8)
            }
#undef SW_FIX_CASE
        };
        auto full_dcol = [&](int t) {
            float wt[NS];
            load_w(t, wt);
            f32x4 d4 = {0.f, 0.f, 0.f, 0.f};
            if (TWO) {
                f32x4 d4b = {0.f, 0.f, 0.f, 0.f};
                dcol_part2(d4, d4b, dyp, wt, -1);
                d4 += d4b;
            } else {
                d4 = dcol_part(d4, dyp, wt, -1);
            }
            return d4;
        };
        // ---- fix-up: the pixel steps skipped above (cmask), tap by tap, not pipelined: dcol of the tap again, then per flagged step
        // the window update in two rounds -- even quarters, then the odd ones on the gradients as the even ones left them (a wave's
        // LDS operations keep their order).  No divergent branches: the order of two branches with disjoint lanes is the
        // compiler's choice; every lane executes both rounds and writes to its plane's dummy cell in the round that is not its own.
        // ---- after-pass over the taps that still have work (none in most rows): (a) the pixel steps skipped above (cmask) -- the window
        // update in two rounds, even quarters, then the odd ones on the gradients as the even ones left them (a wave's LDS operations
        // keep their order; NO divergent branches: the order of two branches with disjoint lanes is the compiler's choice, so every
        // lane executes both rounds and writes to its plane's dummy cell in the round that is not its own); (b) the row's far samples
        // (displaced by TL_NEAR px or more): the four corners from global memory, the input gradient by global atomics (the
        // reference's col2im is an atomicAdd per corner too, cuda/dcn_v2_im2col_cuda.cu:249).  Per tap: dcol again (one product for
        // both), then coordinate gradients / masked samples stored over the zeros the pipelined pass left for these pixels.
        // (b) replaces the generic kernels' far-only pass over listed tiles (rounds 1-3: a whole 32-pixel tile of every channel
        // block redone per far sample).  One loop for both: as two loops the split-bf16 variant spilled into its tap loop.
        unsigned tapwork = 0u;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const unsigned w_ = ((unsigned)(cmask >> (4 * t)) & 15u) | ((unsigned)(fm[t >> 2] >> (16 * (t & 3))) & 0xffffu);
            tapwork |= (w_ != 0u ? 1u : 0u) << t;
        }
#ifdef SW_ABL_NOAFTER
        tapwork = 0u;
#endif
#pragma unroll 1
        for (unsigned tw = tapwork; tw != 0u; tw &= tw - 1u) {
            const int t = __builtin_ctz(tw);
            const unsigned f4 = (unsigned)(cmask >> (4 * t)) & 15u;                     // flagged steps of this tap
            const unsigned pm16 = (unsigned)(fm[t >> 2] >> (16 * (t & 3))) & 0xffffu;   // far pixels of this tap
            const unsigned farq = (pm16 >> (4 * q)) & 15u;                              // ... of this lane's quarter
            const f32x4 d4 = full_dcol(t);
            float Pm[4], Ph[4], Pw[4], colv[4];
            char *const dummy = lane_plane + SW_ZERO * 8;
            const bool odd = q & 1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Pm[r] = 0.f; Ph[r] = 0.f; Pw[r] = 0.f; colv[r] = 0.f;
                if ((f4 >> r) & 1u) {                              // uniform
                    const f32x4 e = *reinterpret_cast<const f32x4 *>(stt2 + (t * 16 + 4 * q + r) * 4);
                    const bool isf = (farq >> r) & 1u;             // far pixel inside a flagged step: part (b)'s
                    const unsigned pp = isf ? ((unsigned)(SW_ZERO * 8) | ((unsigned)(SW_ZERO * 8) << 16)) : __float_as_uint(e.x);
                    const float lh = isf ? 0.f : e.y, lw = isf ? 0.f : e.z, m = isf ? 0.f : e.w;
                    char *const pT = lane_plane + (pp & 0xffffu), *const pB = lane_plane + (pp >> 16);
                    const float v1 = reinterpret_cast<const float *>(pT)[0], v2 = reinterpret_cast<const float *>(pT)[2];
                    const float v3 = reinterpret_cast<const float *>(pB)[0], v4 = reinterpret_cast<const float *>(pB)[2];
                    const float d = d4[r], hh = 1.f - lh, hw = 1.f - lw, dm = d * m;
                    const float ex = v2 - v1, fx = v4 - v3, ay = v3 - v1, by = v4 - v2;
                    const float top = v1 + lw * ex, bot = v3 + lw * fx;
                    const float val = top + lh * (bot - top);
                    Pm[r] = d * val;
                    Ph[r] = dm * (hw * ay + lw * by);
                    Pw[r] = dm * (hh * ex + lh * fx);
                    colv[r] = m * val;
                    const float w1 = dm * (hh * hw), w2 = dm * (hh * lw), w3 = dm * (lh * hw), w4 = dm * (lh * lw);
                    {
                        const float g1 = reinterpret_cast<const float *>(pT)[1], g2 = reinterpret_cast<const float *>(pT)[3];
                        const float g3 = reinterpret_cast<const float *>(pB)[1], g4 = reinterpret_cast<const float *>(pB)[3];
                        char *const aT = odd ? dummy : pT, *const aB = odd ? dummy : pB;
                        reinterpret_cast<float *>(aT)[1] = g1 + w1;
                        reinterpret_cast<float *>(aT)[3] = g2 + w2;
                        reinterpret_cast<float *>(aB)[1] = g3 + w3;
                        reinterpret_cast<float *>(aB)[3] = g4 + w4;
                    }
                    __builtin_amdgcn_wave_barrier();
                    {
                        const float g1 = reinterpret_cast<const float *>(pT)[1], g2 = reinterpret_cast<const float *>(pT)[3];
                        const float g3 = reinterpret_cast<const float *>(pB)[1], g4 = reinterpret_cast<const float *>(pB)[3];
                        char *const cT = odd ? pT : dummy, *const cB = odd ? pB : dummy;
                        reinterpret_cast<float *>(cT)[1] = g1 + w1;
                        reinterpret_cast<float *>(cT)[3] = g2 + w2;
                        reinterpret_cast<float *>(cB)[1] = g3 + w3;
                        reinterpret_cast<float *>(cB)[3] = g4 + w4;
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
            if (pm16 != 0u) {                                      // uniform: far samples in this tap
                float cv[4][4], lhv[4], lwv[4], mv[4];
                int gofs[4];
                bool ok[4][4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {                       // all sixteen corner loads first: one round trip per tap
                    const f32x4 e = *reinterpret_cast<const f32x4 *>(stt2 + (t * 16 + 4 * q + r) * 4);
                    const bool isf = ((farq >> r) & 1u) && j < cleft;
                    const unsigned pp = __float_as_uint(e.x);
                    const int yl = (int)(pp & 0xffffu) - 1, xl = (int)(pp >> 16) - 1;
                    lhv[r] = isf ? e.y : 0.f; lwv[r] = isf ? e.z : 0.f; mv[r] = isf ? e.w : 0.f;
                    ok[r][0] = isf && yl >= 0 && xl >= 0;
                    ok[r][1] = isf && yl >= 0 && xl + 1 < W;
                    ok[r][2] = isf && yl + 1 < H && xl >= 0;
                    ok[r][3] = isf && yl + 1 < H && xl + 1 < W;
                    gofs[r] = (j * HW + yl * W + xl) * 4;
                    constexpr int DO[4] = {0, 1, 0, 1};
#pragma unroll
                    for (int c_ = 0; c_ < 4; ++c_)
                        cv[r][c_] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                                  r_in, ok[r][c_] ? gofs[r] + (DO[c_] + (c_ >> 1) * W) * 4 : SW_OOB, 0, 0));
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v1 = cv[r][0], v2 = cv[r][1], v3 = cv[r][2], v4 = cv[r][3];
                    const float lh = lhv[r], lw = lwv[r], m = mv[r];
                    const float d = d4[r], hh = 1.f - lh, hw = 1.f - lw, dm = d * m;
                    const float ex = v2 - v1, fx = v4 - v3, ay = v3 - v1, by = v4 - v2;
                    const float top = v1 + lw * ex, bot = v3 + lw * fx;
                    const float val = top + lh * (bot - top);
                    Pm[r] += d * val;                               // (lanes without a far sample loaded four zeros)
                    Ph[r] += dm * (hw * ay + lw * by);
                    Pw[r] += dm * (hh * ex + lh * fx);
                    float *gp = reinterpret_cast<float *>(reinterpret_cast<char *>(gin_c) + gofs[r]);
                    if (ok[r][0]) atomicAdd(gp, dm * (hh * hw));
                    if (ok[r][1]) atomicAdd(gp + 1, dm * (hh * lw));
                    if (ok[r][2]) atomicAdd(gp + W, dm * (lh * hw));
                    if (ok[r][3]) atomicAdd(gp + W + 1, dm * (lh * lw));
                    colv[r] += m * val;
                }
            }
            // lanes 0..3 of a quarter publish the sums of its pixels 4 q + j: here only the pixels redone above (the pipelined pass
            // stored zeros for them)
            const unsigned redo = f4 | farq;
            const int cpx = (j < 4 && ((redo >> (j & 3)) & 1u) && x0 + 4 * q + j < W) ? (x0 + 4 * q + j) * 4 : SW_OOB;
            auto cpx_store = [&](int plane, float v) {
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r_cp, cpx, (plane * HW + y * W) * 4, 0);
            };
            cpx_store(2 * t, sw_reduce4(Ph, bit0, bit1));
            cpx_store(2 * t + 1, sw_reduce4(Pw, bit0, bit1));
            cpx_store(18 + t, sw_reduce4(Pm, bit0, bit1));
            if (!DWK) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, colv[r]), r_col,
                                                          (q4v && ((redo >> r) & 1u)) ? (j * 9 * HW + x0 + 4 * q + r) * 4 : SW_OOB,
                                                          (t * HW + y * W) * 4, 0);
            } else {
                add_dw(t, colv);
            }
        }
        if (DWK && !SPLIT) {
#pragma unroll
            for (int ob = 0; ob < 4; ++ob) dyo_p3[ob] = dyo[ob][3];    // A operands of the pixel step still pending
        }

        SW_STAMP(prof_slot + 12);
        // ---- retire input row y - 4: its gradient is complete (row y + 1 reaches up to y - 3).  slot s0 then takes row y + 5
        {
            const int yy = y - 4;
            float *gbase = gin_c + (yy * W + x0 - 4);             // uniform
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int e = lane + 64 * k;
                const int ch = e / SW_WW, col = e - ch * SW_WW;
                float *cell = ring + (ch * SW_PLANE + s0 * SW_WW + col) * 2 + 1;
                const float gv = *cell;
                *cell = 0.f;
                const int xx = x0 - 4 + col;
#ifndef SW_ABL_NOFLUSH
                if (gv != 0.f && ch < cleft && yy >= 0 && xx >= 0 && xx < W)
                    atomicAdd(reinterpret_cast<float *>(reinterpret_cast<char *>(gbase) + (unsigned)(ch * HW + col) * 4u), gv);
#endif
            }
            row_store(s0, rx);
        }
        SW_STAMP(prof_slot + 13);
        s0 = s0 + 1 == SW_RING ? 0 : s0 + 1;
#pragma unroll
        for (int s = 0; s < NS; ++s) dyp[s] = dyp_n[s];
        if (DWK) {
            if (ck == 0) {                             // grad_bias: this wave's pixels of the next row (zeros after the last one)
#pragma unroll
                for (int ob = 0; ob < 4; ++ob) bsum[ob] += (dyo_n[ob].x + dyo_n[ob].y) + (dyo_n[ob].z + dyo_n[ob].w);
            }
#pragma unroll
            for (int ob = 0; ob < 4; ++ob) dyo[ob] = ONE ? sw_round4(dyo_n[ob]) : (SPLIT ? sw_split4(dyo_n[ob]) : dyo_n[ob]);
        }
        raw = raw_n;
    }

    // ---- the eight rows still in the ring: y1-4 .. y1+3 (slots s0 ..)
    for (int i = 0; i < SW_RING - 1; ++i) {
        const int yy = y1 - 4 + i;
        int sl = s0 + i;
        sl = sl >= SW_RING ? sl - SW_RING : sl;
        for (int k = 0; k < 6; ++k) {
            const int e = lane + 64 * k;
            const int ch = e / SW_WW, col = e - ch * SW_WW;
            const float gv = ring[(ch * SW_PLANE + sl * SW_WW + col) * 2 + 1];
            const int xx = x0 - 4 + col;
            if (gv != 0.f && ch < cleft && yy >= 0 && yy < H && xx >= 0 && xx < W) atomicAdd(gin_c + (size_t)ch * HW + yy * W + xx, gv);
        }
    }

    if (DWK && !SPLIT) {
#pragma unroll
        for (int ob = 0; ob < 4; ++ob)
            accw[8][ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(dyo_p3[ob], pend_col, accw[8][ob], 0, 0, 0);
    }
    }   // units of this wave

    // ---- partial of this wave: grad_weight [tap][o][c] (lane (q, j), block ob, register i -> o = 16 ob + 4 q + i, c = j), then
    // grad_bias [o] (chunk 0; the four quarters of a lane column hold different pixels of the same o = 16 ob + j)
    if (DWK) {
        float *dst = a.dwpart + ((size_t)ck * (a.nslot / a.nck) + (id0 / (8 * a.nck)) * 8 + (id0 & 7)) * SW_PART_FLOATS;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int ob = 0; ob < 4; ++ob)
#pragma unroll
                for (int i = 0; i < 4; ++i) dst[(t * 64 + 16 * ob + 4 * q + i) * SW_CH + j] = accw[t][ob][i];
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) {
            float v_ = bsum[ob];
            v_ += __shfl_xor(v_, 16);
            v_ += __shfl_xor(v_, 32);
            if (q == 0) dst[SW_DW_FLOATS + 16 * ob + j] = v_;
        }
    }
}

// grad_offset[b][p] = sum_ck cpart[ck][b][p], p < 18; grad_mask[b][t] = sum_ck cpart[ck][b][18 + t]  (fixed order)
__device__ __forceinline__ void sweep_reduce_coord_body(const float *__restrict__ cpart, float *__restrict__ goff,
                                                        float *__restrict__ gmsk, int B, int HW, int nck,
                                                        const unsigned *__restrict__ far_scal, int total_tiles, int bid, int nb)
{
    // far samples dominate: no partial planes were written and the generic kernel accumulates into these tensors with
    // atomics when its channel blocks are split -> hand it zeros
    const bool zero = far_dominated(far_scal, total_tiles);
    const int64_t n4 = (int64_t)B * 27 * HW / 4, per_b4 = (int64_t)27 * HW / 4, off4 = (int64_t)18 * HW / 4;
    const size_t stride4 = (size_t)B * 27 * HW / 4;
    for (int64_t i = (int64_t)bid * blockDim.x + threadIdx.x; i < n4; i += (int64_t)nb * blockDim.x) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        if (!zero) s = reinterpret_cast<const f32x4 *>(cpart)[i];
        for (int ck = 1; ck < nck && !zero; ++ck) {
            const f32x4 v = reinterpret_cast<const f32x4 *>(cpart)[i + ck * stride4];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        const int64_t b = i / per_b4, r = i - b * per_b4;
        if (r < off4) reinterpret_cast<f32x4 *>(goff)[b * off4 + r] = s;
        else reinterpret_cast<f32x4 *>(gmsk)[b * (per_b4 - off4) + (r - off4)] = s;
    }
}

// grad_weight[o][16 ck + c][t] += sum_v dwpart[ck][v][t][o][c]   (grid.y groups of v, atomics onto the zero-filled gradient:
// <= gridDim.y per address; the far-only pass of the generic kernel adds to the same tensor)
// (bx, nbx, by, nby: the block's virtual 2-D index)
__device__ __forceinline__ void sweep_reduce_dw_body(const float *__restrict__ part, float *__restrict__ gw, float *__restrict__ gbias,
                                                     const Geom &g, int nck, int nvp, const unsigned *__restrict__ far_scal,
                                                     int total_tiles, int bx, int nbx, int by, int nby)
{
    if (far_dominated(far_scal, total_tiles)) return;
    const int n = nck * SW_DW_FLOATS + 64;                 // the last 64: grad_bias from chunk 0's partials
    const int v0 = (int)((int64_t)by * nvp / nby), v1 = (int)((int64_t)(by + 1) * nvp / nby);
    for (int idx = bx * blockDim.x + threadIdx.x; idx < n; idx += nbx * blockDim.x) {
        const bool is_bias = idx >= nck * SW_DW_FLOATS;
        const int ck = is_bias ? 0 : idx / SW_DW_FLOATS, e = is_bias ? SW_DW_FLOATS + (idx - nck * SW_DW_FLOATS) : idx - ck * SW_DW_FLOATS;
        const int c = e & 15, o = is_bias ? e - SW_DW_FLOATS : (e >> 4) & 63, t = e >> 10;
        const int cc = ck * SW_CH + c;
        if (o >= g.Co || (!is_bias && cc >= g.C)) continue;
        const float *src = part + (size_t)ck * nvp * SW_PART_FLOATS + e;
        float s = 0.f;
#pragma unroll 8
        for (int vv = v0; vv < v1; ++vv) s += src[(size_t)vv * SW_PART_FLOATS];
        if (is_bias) atomicAdd(gbias + o, s);
        else atomicAdd(gw + ((size_t)o * g.C + cc) * 9 + t, s);
    }
}

// grad_weight[i] = sum_s part[s][i]  (nob > 1: the partials of the dY x col^T product, fixed order; plain stores -- the far-only
// pass of the generic kernel, launched afterwards, adds the far samples' share with atomics).  Far samples dominating the call:
// col was never written and the generic kernel owns grad_weight (zero-filled) -> nothing to do.
__device__ __forceinline__ void sweep_reduce_gemm_body(const float *__restrict__ part, float *__restrict__ gw, int n, int S,
                                                       const unsigned *__restrict__ far_scal, int total_tiles, int bid, int nb)
{
    if (far_dominated(far_scal, total_tiles)) return;
    for (int i = (bid * blockDim.x + threadIdx.x) * 4; i < n; i += nb * blockDim.x * 4) {
        if (i + 3 < n) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int s = 0; s < S; ++s) acc += *reinterpret_cast<const f32x4 *>(part + (size_t)s * n + i);
            *reinterpret_cast<f32x4 *>(gw + i) = acc;
        } else {
            for (int j = 0; i + j < n; ++j) {
                float a = 0.f;
                for (int s = 0; s < S; ++s) a += part[(size_t)s * n + i + j];
                gw[i + j] = a;
            }
        }
    }
}

// Round 4: the call's reductions after the sweep as ONE launch (they were three): blocks [0, nb_coord) sum the coordinate-gradient
// planes, the next Cout * bias_splits are dcn_bias_grad's (grad_bias when no sweep wave summed dY: wide outputs, or the call was
// handed to the generic kernels), the rest reduce grad_weight -- from the waves' partials (dw_by > 0: a dw_bx x dw_by grid) or from
// the product's partials.
struct SweepEpilogueArgs {
    const float *cpart, *gy, *dwpart;
    float *goff, *gmsk, *gw, *gbias;
    const unsigned *far_scal, *bias_only_if_far;
    Geom g;
    int nck, nvp, total_tiles, nb_coord, bias_splits, dw_bx, dw_by, gemm_n, gemm_S;
    unsigned *far_report = nullptr;   // mapped host word: the call's far-coordinate count for the host's hand-over policy (dcn_v2.hip)
    unsigned far_base = 0;            // the count field's start value (pivot - limit)
};
__global__ __launch_bounds__(256) void dcn_sweep_epilogue(SweepEpilogueArgs a)
{
    int bid = blockIdx.x;
    if (a.far_report && bid == 0 && threadIdx.x == 0) {
        const unsigned c = a.far_scal[3] & ~FAR_BY_COUNT;
        *a.far_report = c >= a.far_base ? c - a.far_base : 0u;
    }
    if (bid < a.nb_coord) {
        sweep_reduce_coord_body(a.cpart, a.goff, a.gmsk, a.g.B, a.g.HoWo, a.nck, a.far_scal, a.total_tiles, bid, a.nb_coord);
        return;
    }
    bid -= a.nb_coord;
    const int nb_bias = a.g.Co * a.bias_splits;
    if (bid < nb_bias) {
        bias_grad_body(a.gy, a.gbias, a.g.B, a.g.Co, a.g.HoWo, a.bias_only_if_far, bid % a.g.Co, bid / a.g.Co, a.bias_splits);
        return;
    }
    bid -= nb_bias;
    if (a.dw_by > 0)
        sweep_reduce_dw_body(a.dwpart, a.gw, a.gbias, a.g, a.nck, a.nvp, a.far_scal, a.total_tiles, bid % a.dw_bx, a.dw_bx, bid / a.dw_bx, a.dw_by);
    else
        sweep_reduce_gemm_body(a.dwpart, a.gw, a.gemm_n, a.gemm_S, a.far_scal, a.total_tiles, bid, (int)gridDim.x - a.nb_coord - nb_bias);
}
