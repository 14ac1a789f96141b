// dcn_v2_bf16x3.inc -- DCD_PREC_BF16X3: the weight contractions of the workgroup-tiled DCNv2 kernels on
// v_mfma_f32_32x32x16_bf16 with split-bf16 operands.  Included inside dcn_v2.hip's anonymous namespace (shares Geom, TapRaw,
// the window constants and the rescue / far-only kernels, which stay exact fp32).
//
// Every fp32 operand x is split as x = hi + lo + r with hi = bf16(x), lo = bf16(x - hi), |r| <= 2^-17 |x| (both roundings
// to nearest even: v_cvt_pk_bf16_f32), and a product is evaluated as a_hi*b_hi + a_hi*b_lo + a_lo*b_hi with fp32
// accumulation -- three matrix instructions of K = 16 in 3 x 32 cycles where the f32 form needs eight of K = 2 in 8 x 64:
// 5.3x less matrix time at ~2^-16 relative error per product (the dropped terms a_lo*b_lo, r_a*b, a*r_b).  Sampling itself
// (bilinear weights, mask) stays fp32; only the finished column value is split.
//
// Operand maps of v_mfma_f32_32x32x16_bf16 (cdna_hip_programming.md section 3): lane l holds A[i = l & 31][k = 8 (l >> 5) + j]
// and B[k = 8 (l >> 5) + j][n = l & 31], j = 0..7 (four VGPRs each); C/D as the f32 form: D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31].

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct Split8 {
    bf16x8 hi, lo;
};

// (a, b) -> packed bf16 pairs (a in the low half): hi = rne(x), lo = rne(x - hi)
__device__ __forceinline__ void split_pair(float a, float b, unsigned &hi, unsigned &lo)
{
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
    const float ah = __uint_as_float(hi << 16), bh = __uint_as_float(hi & 0xffff0000u);
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a - ah, b - bh}, bf16x2));
}

__device__ __forceinline__ Split8 split8(const float (&v)[8])
{
    u32x4 h, l;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        unsigned hh, ll;
        split_pair(v[2 * q], v[2 * q + 1], hh, ll);
        h[q] = hh;
        l[q] = ll;
    }
    Split8 s;
    s.hi = __builtin_bit_cast(bf16x8, h);
    s.lo = __builtin_bit_cast(bf16x8, l);
    return s;
}

// eight fp32 values -> bf16 (nearest even), no low part: the operand of the one-product form (DCD_PREC_BF16)
__device__ __forceinline__ bf16x8 round8(const float (&v)[8])
{
    u32x4 h;
#pragma unroll
    for (int q = 0; q < 4; ++q) h[q] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v[2 * q], v[2 * q + 1]}, bf16x2));
    return __builtin_bit_cast(bf16x8, h);
}
__device__ __forceinline__ unsigned round_pair(float a, float b)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
}

// acc += A * B over K = 16, small terms first
__device__ __forceinline__ f32x16 mfma_bf16x3(const bf16x8 &a_hi, const bf16x8 &a_lo, const Split8 &b, f32x16 acc)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b.hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b.lo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b.hi, acc, 0, 0, 0);
    return acc;
}

// ---------------------------------------------------------------------------------------------
// Forward, workgroup-tiled (same tiling, window and far-sample rules as dcn_fwd_tile_f32): chunks of 16 input channels.
// LDS per buffer: window [16][WH][40] fp32 + the chunk's pre-split weight slab
//     Ws[tap 9][ob 2][hi|lo][lane 64][8 bf16]   (a wave's A operand of (tap, ob, part) is ONE lane-linear ds_read_b128)
// prepared in that order in the workspace by dcn_prep_weights_tile_bf16, so staging it is a straight copy.
// TR = 8: two LDS buffers (152 KB), one workgroup of 8 waves per CU, one barrier per chunk.
// TR = 4: one LDS buffer (66 KB), two workgroups per CU; the next chunk travels through registers during the MFMA work and
//         is written between two barriers.
// ---------------------------------------------------------------------------------------------
constexpr int TB_NW = TB_W_FLOATS / 4;                   // 2304 dwordx4
template <int TR> struct TileCfgB {
    static constexpr int WH = TR + 8;
    static constexpr int PLANE = WH * TL_WW;
    static constexpr int IN_FLOATS = TB_CH * PLANE;
    static constexpr int BUF = IN_FLOATS + TB_W_FLOATS;
    static constexpr int NBUF = TR == 8 ? 2 : 1;
    static constexpr int NIN = TB_CH * WH * (TL_WW / 4);
    static constexpr int NT = TR * 64;
    static constexpr int KIN = (NIN + NT - 1) / NT, KW = (TB_NW + NT - 1) / NT;
};

// Ws[z][chunk][tap][ob][part][lane][j] = part(W[z*64 + ob*32 + (lane & 31)][chunk*16 + 8 (lane >> 5) + j][tap]); also the
// region flags / far counter and the fp32 rescue layout Wf9, exactly like dcn_prep_weights_tile.
__global__ void dcn_prep_weights_tile_bf16(const float *__restrict__ w, unsigned short *__restrict__ ws, Geom g, int nchunk, int nz,
                                           unsigned *__restrict__ flags, int nflag_words, float *__restrict__ wf9)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nflag_words; i += gridDim.x * blockDim.x) flags[i] = 0u;
    if (wf9) {
        const int K = g.C * 9, n9 = K * g.Cop;
        for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n9; idx += gridDim.x * blockDim.x) {
            const int k = idx / g.Cop, o = idx - k * g.Cop;
            wf9[idx] = (o < g.Co) ? w[(size_t)o * K + k] : 0.f;
        }
    }
    const int n = nz * nchunk * 9 * 2 * 64 * 8;           // one thread per element, writes its hi and lo halves
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += gridDim.x * blockDim.x) {
        int r = idx;
        const int j = r & 7; r >>= 3;
        const int lane = r & 63; r >>= 6;
        const int ob = r & 1; r >>= 1;
        const int t = r % 9; r /= 9;
        const int ck = r % nchunk, z = r / nchunk;
        const int oo = z * TL_OB + ob * 32 + (lane & 31), c = ck * TB_CH + 8 * (lane >> 5) + j;
        const float v = (oo < g.Co && c < g.C) ? w[((size_t)oo * g.C + c) * 9 + t] : 0.f;
        unsigned hi, lo;
        split_pair(v, 0.f, hi, lo);
        const size_t base = ((((size_t)(z * nchunk + ck) * 9 + t) * 2 + ob) * 2) * 64 * 8;
        ws[base + lane * 8 + j] = (unsigned short)(hi & 0xffffu);
        ws[base + 64 * 8 + lane * 8 + j] = (unsigned short)(lo & 0xffffu);
    }
}

// NP = 3: split-bf16.  NP = 1 (DCD_PREC_BF16): one product of bf16-rounded operands (the hi halves of the same prepared weights).
template <int TR, int NP>
__global__ __launch_bounds__(TR * 64) void dcn_fwd_tile_bf16x3(const float *__restrict__ in, const float *__restrict__ off,
                                                           const float *__restrict__ msk, const float *__restrict__ ws,
                                                           const float *__restrict__ bias, float *__restrict__ out, Geom g,
                                                           int tiles_x, int nchunk, unsigned char *__restrict__ rescue_flags,
                                                           const float *__restrict__ wf9, int rescue_taps,
                                                           const unsigned *__restrict__ far_count, unsigned far_limit)
{
    typedef TileCfgB<TR> T;
    constexpr int WH = T::WH, PLANE = T::PLANE, IN_FLOATS = T::IN_FLOATS, BUF = T::BUF, NIN = T::NIN, NT = T::NT, KIN = T::KIN,
                  KW = T::KW, NBUF = T::NBUF;
    extern __shared__ __attribute__((aligned(16))) float lds[];       // NBUF x BUF
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int p = lane & 31, h = lane >> 5;
    int bx = blockIdx.x, b = blockIdx.y;
    xcd_remap(bx, b);
    if (*far_count > far_limit) {                              // far samples dominate this call: every region goes to the rescue kernel
        if (tid == 0) rescue_flags[(size_t)b * gridDim.x + bx] = 1;
        return;
    }
    const int ty = bx / tiles_x, tx = bx - ty * tiles_x;
    const int r0 = ty * TR, c0 = tx * 32;
    const int ho = r0 + wave, wo = c0 + p;
    const bool pv = ho < g.Ho && wo < g.Wo;
    const int Pc = pv ? ho * g.Wo + wo : 0;
    const int z = blockIdx.z;
    const int HW = g.H * g.W;
    const int Y0 = r0 - 4, X0 = c0 - 4;

    const float *in_b = in + (size_t)b * g.C * HW;
    const float *off_b = off + (size_t)b * 18 * g.HoWo;
    const float *msk_b = msk + (size_t)b * 9 * g.HoWo;
    const float *ws_z = ws + (size_t)z * nchunk * TB_W_FLOATS;

    // ---- staging map (chunk invariant)
    int sg[KIN], sl[KIN];            // global float offset inside the chunk's 16 planes (-1: zeros), LDS float offset
#pragma unroll
    for (int k = 0; k < KIN; ++k) {
        const int e = tid + NT * k;
        const int ch = e / (WH * 10), rem = e - ch * (WH * 10);
        const int row = rem / 10, q = rem - row * 10;
        const int y = Y0 + row, x = X0 + 4 * q;
        sg[k] = (e < NIN && y >= 0 && y < g.H && x >= 0 && x < g.W) ? ch * HW + y * g.W + x : -1;
        sl[k] = e < NIN ? ch * PLANE + row * TL_WW + 4 * q : -1;
    }
    f32x4 rin[KIN], rw[KW];
    auto issue = [&](int ck) {
        const float *src = in_b + (size_t)ck * TB_CH * HW;
        const int cleft = g.C - ck * TB_CH;                      // channels left (may be < 16 in the last chunk)
#pragma unroll
        for (int k = 0; k < KIN; ++k) {
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
            rin[k] = zero4;
            if (sg[k] >= 0 && (tid + NT * k) / (WH * 10) < cleft) rin[k] = *reinterpret_cast<const f32x4 *>(src + sg[k]);
        }
        const float *wsrc = ws_z + (size_t)ck * TB_W_FLOATS;
#pragma unroll
        for (int k = 0; k < KW; ++k)
            if (tid + NT * k < TB_NW) rw[k] = *reinterpret_cast<const f32x4 *>(wsrc + 4 * (tid + NT * k));
    };
    auto commit = [&](float *buf) {
#pragma unroll
        for (int k = 0; k < KIN; ++k)
            if (sl[k] >= 0) *reinterpret_cast<f32x4 *>(buf + sl[k]) = rin[k];
#pragma unroll
        for (int k = 0; k < KW; ++k)
            if (tid + NT * k < TB_NW) *reinterpret_cast<f32x4 *>(buf + IN_FLOATS + 4 * (tid + NT * k)) = rw[k];
    };

    issue(0);

    // ---- sampling state of the nine taps of this lane's pixel (while the first chunk is in flight)
    int lo[9];
    float wq[9][4];
    unsigned farbits = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const TapRaw raw = load_tap_raw(off_b, msk_b, g, t, Pc);
        const float hf = (float)(ho - 1 + t / 3) + raw.oh, wf_ = (float)(wo - 1 + t % 3) + raw.ow;
        const bool sv = pv && hf > -1.f && wf_ > -1.f && hf < (float)g.H && wf_ < (float)g.W;
        const float hlf = floorf(hf), wlf = floorf(wf_);
        const int ly = sv ? (int)hlf - Y0 : 0, lx = sv ? (int)wlf - X0 : 0;
        const bool inside = ly >= 0 && lx >= 0 && ly <= WH - 2 && lx <= TL_WW - 2;
        farbits |= (sv && !inside) ? (1u << t) : 0u;
        lo[t] = (inside ? ly * TL_WW + lx : 0) + 8 * h * PLANE;
        const float lh = hf - hlf, lw = wf_ - wlf;
        const float m = (sv && inside) ? raw.m : 0.f;
        wq[t][0] = (1.f - lh) * (1.f - lw) * m; wq[t][1] = (1.f - lh) * lw * m;
        wq[t][2] = lh * (1.f - lw) * m;         wq[t][3] = lh * lw * m;
    }

    f32x16 acc[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mb][r] = 0.f;

    // workgroup-uniform escape for large learned offsets, as in the f32 kernel
    int wave_far_taps = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) wave_far_taps += __any((farbits >> t) & 1u) ? 1 : 0;
    __shared__ int far_worst;
    if (tid == 0) far_worst = 0;
    __syncthreads();
    if (lane == 0) atomicMax(&far_worst, wave_far_taps);
    __syncthreads();
    if (far_worst >= rescue_taps) {
        if (tid == 0) rescue_flags[(size_t)b * gridDim.x + bx] = 1;      // dcn_fwd9_f32<., true> computes this region
        return;
    }

    commit(lds);
    __syncthreads();

    for (int ck = 0; ck < nchunk; ++ck) {
        const float *buf = lds + (NBUF == 2 ? (ck & 1) * BUF : 0);
        if (ck + 1 < nchunk) issue(ck + 1);
        const u32x4 *wsl = reinterpret_cast<const u32x4 *>(buf + IN_FLOATS) + lane;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const bf16x8 a0h = __builtin_bit_cast(bf16x8, wsl[((t * 2 + 0) * 2 + 0) * 64]);
            const bf16x8 a1h = __builtin_bit_cast(bf16x8, wsl[((t * 2 + 1) * 2 + 0) * 64]);
            const float *cp = buf + lo[t];
            const float q0 = wq[t][0], q1 = wq[t][1], q2 = wq[t][2], q3 = wq[t][3];
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float *c2 = cp + j * PLANE;
                v[j] = q0 * c2[0] + q1 * c2[1] + q2 * c2[TL_WW] + q3 * c2[TL_WW + 1];
            }
            if constexpr (NP == 1) {
                const bf16x8 bh = round8(v);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, bh, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, bh, acc[1], 0, 0, 0);
            } else {
                const bf16x8 a0l = __builtin_bit_cast(bf16x8, wsl[((t * 2 + 0) * 2 + 1) * 64]);
                const bf16x8 a1l = __builtin_bit_cast(bf16x8, wsl[((t * 2 + 1) * 2 + 1) * 64]);
                const Split8 bq = split8(v);
                acc[0] = mfma_bf16x3(a0h, a0l, bq, acc[0]);
                acc[1] = mfma_bf16x3(a1h, a1l, bq, acc[1]);
            }
        }
        if (NBUF == 1) __syncthreads();                               // everyone is done reading the single buffer
        if (ck + 1 < nchunk) commit(lds + (NBUF == 2 ? ((ck + 1) & 1) * BUF : 0));
        __syncthreads();
    }

    if (__any(farbits != 0u)) {
        // samples whose 2x2 footprint left the staged window: gathered from global memory by their lane, exact fp32 MFMA
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
            if (!__any((farbits >> t) & 1u)) continue;
            const bool mine = (farbits >> t) & 1u;
            const Tap s = make_tap(off_b, msk_b, g, t, t, ho, wo, Pc, pv);
            const float *w9 = wf9 + (size_t)t * g.Cop + z * TL_OB + p;
            const bool second = z * TL_OB + 32 < g.Cop;
            const int cend = (g.C + 1) & ~1;
            for (int cc0 = h; cc0 < cend; cc0 += 8) {
                f32x2 gt[4], gb[4];
                float wa[4], wb2[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = cc0 + 2 * u;
                    const int cc = c < g.C ? c : g.C - 1;
                    const float *gp = in_b + (size_t)cc * HW;
                    gt[u] = ldg2(gp, (unsigned)s.pt * 4u);
                    gb[u] = ldg2(gp, (unsigned)s.pb * 4u);
                    const float *wr = w9 + (size_t)cc * 9 * g.Cop;
                    wa[u] = wr[0];
                    wb2[u] = second ? wr[32] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = cc0 + 2 * u;
                    const bool live = mine && c < g.C;
                    const float val = live ? (s.a0 * gt[u].x + s.a1 * gt[u].y + s.b0 * gb[u].x + s.b1 * gb[u].y) * s.m : 0.f;
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[u], val, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wb2[u], val, acc[1], 0, 0, 0);
                }
            }
        }
    }

    float *out_b = out + (size_t)b * g.Co * g.HoWo;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        const int obase = z * TL_OB + mb * 32 + 4 * h;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = obase + (r & 3) + 8 * (r >> 2);
            if (pv && o < g.Co) out_b[(size_t)o * g.HoWo + ho * g.Wo + wo] = acc[mb][r] + bias[o];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// grad_weight, workgroup-tiled, second generation (both precisions: PREC = DCD_PREC_F32 / DCD_PREC_BF16X3).
//
// Same tiling as dcn_bwd_weight_tile_f32 (2 x 32-pixel tile x 32 input channels x 64 outputs, six waves = (tile row, kernel
// row), lane = channel, accumulators persist over the workgroup's share of tiles, partials summed by dcn_dw_reduce), but the
// inner loop is re-cut around what bounded that kernel -- a serial chain bpermute -> LDS gather -> FMA -> MFMA per pixel pair
// with six waves in lockstep (DESIGN.md section 4: its components added up instead of overlapping):
//   * the sampling state of every (row, tap, pixel) -- window offset + 4 mask-scaled bilinear weights -- is written to an LDS
//     table once per tile by the lane that owns the pixel; the 32 lanes of a half then fetch the state of "their" pixel with a
//     broadcast ds_read_b128 + ds_read_b32 (conflict-free by construction) instead of five ds_bpermute;
//   * a lane evaluates EIGHT pixels per (step, tap) before any matrix instruction: eight independent table-read -> gather
//     chains in flight, then the MFMAs back to back;
//   * f32:    pixels 2j + h of the 16-pixel step, eight k-steps of v_mfma_f32_32x32x2_f32 per output block;
//     bf16x3: pixels 8h + j are exactly the lane's K = 16 operand; the dY tile is split into bf16 hi / lo planes when it is
//             staged (once per tile, not once per wave), the B operand is one ds_read_b128 per plane.
// ---------------------------------------------------------------------------------------------
constexpr int DW2_DY_F32 = TL_OB * DW_DYS;                 // 4160 floats  [64 o][65]
constexpr int DW2_DYB_STRIDE = 36;                         // dwords per output row of one bf16 plane: 64 px * 2 B + 16 B pad
constexpr int DW2_DY_BF16 = 2 * TL_OB * DW2_DYB_STRIDE;    // 4608 dwords  hi plane | lo plane
constexpr int DW2_STQ = DW_TR * 9 * 32 * 4;                // 2304 floats  [row][tap][pixel][4 weights]
constexpr int DW2_STP = DW_TR * 9 * 32;                    // 576 ints     [row][tap][pixel] window offset
template <int PREC> struct Dw2Cfg {
    static constexpr int DY = PREC == DCD_PREC_BF16X3 ? DW2_DY_BF16 : DW2_DY_F32;
    static constexpr int FLOATS = DW_IN_FLOATS + DY + DW2_STQ + DW2_STP;
};

template <int PREC>
__global__ __launch_bounds__(DW_NT, 3) void dcn_bwd_weight_tile_v2(const float *__restrict__ in, const float *__restrict__ off,
                                                                   const float *__restrict__ msk, const float *__restrict__ gy,
                                                                   float *__restrict__ part, Geom g, int tiles_x, int tiles_y,
                                                                   int nsplit, const unsigned *__restrict__ far_scal, int col_major)
{
    if (far_dominated(far_scal, g.B * ((g.HoWo + 31) / 32))) return;      // the generic kernel does the whole job instead
    constexpr bool SPLIT = PREC == DCD_PREC_BF16X3;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *win = lds, *dyt = lds + DW_IN_FLOATS;
    float *stq = dyt + Dw2Cfg<PREC>::DY;
    int *stp = reinterpret_cast<int *>(stq + DW2_STQ);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int row = wave & 1, ky = wave >> 1;
    const int cb = blockIdx.x, zo = blockIdx.z;
    const int HW = g.H * g.W;
    const int total = g.B * tiles_x * tiles_y;
    const int t0 = (int)((int64_t)blockIdx.y * total / nsplit), t1 = (int)((int64_t)(blockIdx.y + 1) * total / nsplit);

    f32x16 acc[3][2];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][mb][r] = 0.f;

    constexpr int KDY = (TL_OB * DW_TR * 8 + DW_NT - 1) / DW_NT;       // 3 dY dwordx4 per thread

    for (int ti = t0; ti < t1; ++ti) {
        const int b = ti / (tiles_x * tiles_y);
        const int rem = ti - b * (tiles_x * tiles_y);
        // tile order inside a workgroup's share: down a column strip (col_major).  Successive 10-row windows then overlap in 8
        // rows that this CU has just read (L1 / this XCD's L2) instead of 8 columns of 40 -- the window is 6.25x the tile.
        const int ty = col_major ? rem % tiles_y : rem / tiles_x, tx = col_major ? rem / tiles_y : rem - ty * tiles_x;
        const int r0 = ty * DW_TR, c0 = tx * 32;
        const int Y0 = r0 - 4, X0 = c0 - 4;
        const float *in_b = in + ((size_t)b * g.C + (size_t)cb * DW_CB) * HW;
        const float *gy_b = gy + ((size_t)b * g.Co + (size_t)zo * TL_OB) * g.HoWo;
        const int cleft = g.C - cb * DW_CB, oleft = g.Co - zo * TL_OB;

        // ---- sampling state of this wave's (row, ky): lane = pixel (both halves compute it, half 0 publishes it)
        const int ho = r0 + row, wo = c0 + i;
        const bool pv = ho < g.Ho && wo < g.Wo;
        const int Pc = pv ? ho * g.Wo + wo : 0;
        const float *off_b = off + (size_t)b * 18 * g.HoWo;
        const float *msk_b = msk + (size_t)b * 9 * g.HoWo;
        int posv[3];
        f32x4 wv[3];
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int t = ky * 3 + kx;
            const TapRaw raw = load_tap_raw(off_b, msk_b, g, t, Pc);
            const float hf = (float)(ho - 1 + ky) + raw.oh, wf_ = (float)(wo - 1 + kx) + raw.ow;
            const bool sv = pv && hf > -1.f && wf_ > -1.f && hf < (float)g.H && wf_ < (float)g.W &&
                            fabsf(raw.oh) < TL_NEAR && fabsf(raw.ow) < TL_NEAR;
            const float hlf = floorf(hf), wlf = floorf(wf_);
            // the window is a ring of DW_WH rows: input row y lives in slot (y + 4) mod DW_WH whatever the tile, so a tile that
            // continues its predecessor's column strip stages only its DW_TR new rows; the bilinear pair's lower row is the next
            // slot, i.e. -(DW_WH-1) rows away when the upper one sits in the last slot (bit 16)
            const int slot = sv ? ((int)hlf + 4) % DW_WH : 0, lx = sv ? (int)wlf - X0 : 0;
            posv[kx] = (slot * TL_WW + lx) | (slot == DW_WH - 1 ? 1 << 16 : 0);
            const float lh = hf - hlf, lw = wf_ - wlf;
            const float m = sv ? raw.m : 0.f;
            wv[kx] = f32x4{(1.f - lh) * (1.f - lw) * m, (1.f - lh) * lw * m, lh * (1.f - lw) * m, lh * lw * m};
        }

        __syncthreads();                                   // previous tile fully consumed (window, dY and state table)
        if (h == 0) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int e = (row * 9 + ky * 3 + kx) * 32 + i;
                *reinterpret_cast<f32x4 *>(stq + 4 * e) = wv[kx];
                stp[e] = posv[kx];
            }
        }
        {
            // ---- stage the window (three batches of three dwordx4 per thread: bounded register use) and the dY tile
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
            typedef float f32x2_ __attribute__((ext_vector_type(2)));
            // rows to stage: all DW_WH of them, or -- when this tile lies directly below the previous one of this workgroup
            // (same image, same column strip) -- only the DW_TR rows that entered the window
            const bool cont = col_major && ti > t0 && ty > 0;
            const int wr0 = cont ? DW_WH - DW_TR : 0, nrow = DW_WH - wr0;
            const int nel = DW_CB * nrow * 10;
#pragma unroll 1
            for (int k0 = 0; k0 * DW_NT < nel; k0 += 3) {
                f32x4 rin[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int e = tid + DW_NT * (k0 + k);
                    const int ch = e / (nrow * 10), rm = e - ch * (nrow * 10);
                    const int wr = wr0 + rm / 10, q = rm % 10;
                    const int y = Y0 + wr, x = X0 + 4 * q;
                    rin[k] = zero4;
                    if (e < nel && ch < cleft && y >= 0 && y < g.H && x >= 0 && x < g.W)
                        rin[k] = *reinterpret_cast<const f32x4 *>(in_b + (size_t)ch * HW + y * g.W + x);
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int e = tid + DW_NT * (k0 + k);
                    const int ch = e / (nrow * 10), rm = e - ch * (nrow * 10);
                    if (e < nel) {
                        const int wr = wr0 + rm / 10, q = rm % 10;
                        float *d = win + ch * DW_PLANE + (((Y0 + wr + 4) % DW_WH) * 10 + q) * 4;
                        *reinterpret_cast<f32x2_ *>(d) = f32x2_{rin[k].x, rin[k].y};
                        *reinterpret_cast<f32x2_ *>(d + 2) = f32x2_{rin[k].z, rin[k].w};
                    }
                }
            }
            f32x4 rdy[KDY];
#pragma unroll
            for (int k = 0; k < KDY; ++k) {
                const int e = tid + DW_NT * k;
                const int o = e / (DW_TR * 8), rm = e - o * (DW_TR * 8);
                const int wr = rm / 8, q = rm - wr * 8;
                const int y = r0 + wr, x = c0 + 4 * q;
                rdy[k] = zero4;
                if (e < TL_OB * DW_TR * 8 && o < oleft && y < g.Ho && x < g.Wo)
                    rdy[k] = *reinterpret_cast<const f32x4 *>(gy_b + (size_t)o * g.HoWo + y * g.Wo + x);
            }
#pragma unroll
            for (int k = 0; k < KDY; ++k) {
                const int e = tid + DW_NT * k;
                const int o = e / (DW_TR * 8), rm = e - o * (DW_TR * 8);
                if (e < TL_OB * DW_TR * 8) {
                    if (SPLIT) {
                        unsigned h0, l0, h1, l1;
                        split_pair(rdy[k].x, rdy[k].y, h0, l0);
                        split_pair(rdy[k].z, rdy[k].w, h1, l1);
                        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                        unsigned *d = reinterpret_cast<unsigned *>(dyt) + o * DW2_DYB_STRIDE + rm * 2;
                        *reinterpret_cast<u32x2 *>(d) = u32x2{h0, h1};
                        *reinterpret_cast<u32x2 *>(d + TL_OB * DW2_DYB_STRIDE) = u32x2{l0, l1};
                    } else {
                        float *d = dyt + o * DW_DYS + rm * 4;
                        d[0] = rdy[k].x; d[1] = rdy[k].y; d[2] = rdy[k].z; d[3] = rdy[k].w;
                    }
                }
            }
        }
        __syncthreads();

        const float *wl_ = win + i * DW_PLANE;                 // this lane's channel plane
#pragma unroll 1
        for (int step = 0; step < 2; ++step) {
            // B operands of this 16-pixel step (independent of the tap)
            const int px0 = row * 32 + step * 16;
            float dq[2][8];
            const unsigned *dyb = reinterpret_cast<const unsigned *>(dyt) + i * DW2_DYB_STRIDE + (px0 + 8 * h) / 2;
            if (!SPLIT) {
                const float *dl = dyt + i * DW_DYS + px0 + h;
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int j = 0; j < 8; ++j) dq[mb][j] = dl[mb * 32 * DW_DYS + 2 * j];
            }
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int e0 = (row * 9 + ky * 3 + kx) * 32 + step * 16;
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int e = e0 + (SPLIT ? 8 * h + j : 2 * j + h);     // pixel of this lane half (uniform per half: broadcast)
                    const f32x4 q = *reinterpret_cast<const f32x4 *>(stq + 4 * e);
                    const int pe = stp[e];
                    const float *cp = wl_ + (pe & 0xffff);
                    const float *cb_ = cp + ((pe >> 16) ? -(DW_WH - 1) * TL_WW : TL_WW);      // lower row of the pair: next ring slot
                    v[j] = q.x * cp[0] + q.y * cp[1] + q.z * cb_[0] + q.w * cb_[1];
                    if (SPLIT && j == 3) __builtin_amdgcn_sched_barrier(0);   // two batches of four: bounds the loads in flight (VGPRs)
                }
                if (SPLIT) {
                    const Split8 a = split8(v);
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb) {
                        // B operand re-read per tap (4 x 16 B per lane): keeping it live across the gathers spills at 168 VGPRs
                        const bf16x8 bhi = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(dyb + mb * 32 * DW2_DYB_STRIDE));
                        const bf16x8 blo =
                            __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(dyb + (TL_OB + mb * 32) * DW2_DYB_STRIDE));
                        f32x16 c = acc[kx][mb];
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.lo, bhi, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, blo, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, bhi, c, 0, 0, 0);
                        acc[kx][mb] = c;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        acc[kx][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j], dq[0][j], acc[kx][0], 0, 0, 0);
                        acc[kx][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j], dq[1][j], acc[kx][1], 0, 0, 0);
                    }
                }
            }
        }
    }

    // epilogue: as dcn_bwd_weight_tile_f32 (the two tile rows summed in LDS in the weight tensor's [o][c][t] order, coalesced
    // partial stores, dcn_dw_reduce adds the partials)
    constexpr int STG = DW_CB * 9 + 1;                     // 289: lanes (o) hit distinct banks
    float *stage = lds;                                    // 32 x 289 floats (reuses the window area)
    float *mine = part + ((size_t)(cb * gridDim.z + zo) * nsplit + blockIdx.y) * (2 * 32 * DW_CB * 9);
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        __syncthreads();
        if (row == 0) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    stage[i * STG + ((r & 3) + 8 * (r >> 2) + 4 * h) * 9 + ky * 3 + kx] = acc[kx][mb][r];
        }
        __syncthreads();
        if (row == 1) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    stage[i * STG + ((r & 3) + 8 * (r >> 2) + 4 * h) * 9 + ky * 3 + kx] += acc[kx][mb][r];
        }
        __syncthreads();
        for (int e = tid; e < 32 * DW_CB * 9; e += DW_NT) {
            const int ol = e / (DW_CB * 9), j = e - ol * (DW_CB * 9);
            mine[mb * (32 * DW_CB * 9) + e] = stage[ol * STG + j];
        }
    }
}
