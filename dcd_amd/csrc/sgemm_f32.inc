// fp32 GEMM on v_mfma_f32_32x32x2_f32 for the DENSE deformable-convolution path (dcn_dense.inc): the three products of
// a layer whose input is wide and whose map is small (Cin >= 256 at <= 24x80 in DGDE) are plain matrix products over a
// sampled-column buffer, and a column buffer of 70-140 MB is cheap on this part (reference: cuda/dcn_v2_cuda.cu:88-113
// forward, :258-327 backward -- there cuBLAS per image; here one batched launch per product).
//
//     C[z] (M x N, row-major, ldc) = A[z] (M x K) * B[z] (K x N)   (+ bias[m])
//
// Either operand may have its contraction index contiguous (AK / BK) or its free index contiguous:
//     A(m,k) = AK ? A[m*lda + k] : A[k*lda + m]          B(k,n) = BK ? B[n*ldb + k] : B[k*ldb + n]
// grid = (ceil(N/128), ceil(M/128), Z*nsplit); blockIdx.z = z*nsplit + s handles k in [s*kchunk, min(K, (s+1)*kchunk)) and
// writes to C + z*strideC + s*strideCs (split-K partials are summed by the caller's reduction kernel: deterministic).
//
// Workgroup = 4 waves as 2x2, tile 128x128, wave tile 64x64 (2x2 MFMA blocks, 64 accumulator registers); K step 16:
// both tiles live k-major in LDS ([16][128+4] floats each, double-buffered: one barrier per step), global loads of step s+1 are
// issued before the 32 MFMAs of step s and written to LDS after them.  Operand reads are ds_read2_b32 (the lane's two
// blocks are 32 floats apart): two per four MFMAs.
#pragma once
#include "sgemm_tile.h"

namespace {

constexpr int SG_S = SG_T + 4;   // LDS row stride (floats)

template <int N> struct IntK { static constexpr int value = N; };

struct SgemmArgs {
    const float *A, *B;
    float *C;
    const float *bias;           // per row m, or nullptr
    int M, N, K;
    int lda, ldb, ldc;
    long long strideA, strideB, strideC, strideCs;
    int nsplit, kchunk;
    int ct;                      // 1: store C transposed, C[n*ldc + m] (four consecutive m per lane -> one 16-byte store)
    const long long *b_off;      // BOFF kernels: element offset of B's row (BK: row n; otherwise row k) instead of row * ldb --
                                 // rows may then start at any 4-byte aligned address (shifted views of one buffer)
    float alpha = 1.f;           // C = alpha * A B (+ C when accumulate) (+ bias)
    int accumulate = 0;
    int lower_only = 0;          // skip tiles that lie entirely above the diagonal (symmetric rank-k updates)
    const unsigned *skip_count = nullptr;   // device scalar: the whole product is skipped when (*skip_count & 0x7fffffff) > skip_above
    unsigned skip_above = 0;                // (a guarded launch: the caller's other path produces the result in that case)
};

typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));

// TM = rows of the workgroup tile: 128 (waves 2x2, wave tile 64x64) or 64 (waves 1x4, wave tile 64x32: half the accumulators,
// for products with 64 rows, which would leave half of a 128-row tile idle)
template <bool AK, bool BK, int TM, bool BOFF>
__global__ __launch_bounds__(256) void sgemm_f32_tile(SgemmArgs a)
{
    constexpr int SA = TM + 4;                   // LDS row stride of the A tile
    constexpr int WM = TM / 64, WN = 4 / WM;     // waves along m / n
    constexpr int NJ = (SG_T / WN) / 32;         // 32-column blocks per wave
    constexpr int NVA = TM / 64, NVB = SG_T / 64;   // float4 per thread and tile
    __shared__ float lds[2][SG_K * SA + SG_K * SG_S];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave - wm * WN;
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    if (a.skip_count && (*a.skip_count & 0x7fffffffu) > a.skip_above) return;
    if (BOFF) {
        // Shifted-view products (trunk autocorrelations: 64 x 832 x pixels): the column tiles of one (image, split) read the same
        // pixel chunk of X through different row offsets.  Workgroups are dealt to the 8 XCDs round-robin, so by default those
        // tiles land on different L2s; deal whole (by, bz) groups to one XCD instead.
        const int nx = gridDim.x, NG = gridDim.y * gridDim.z;
        if ((NG & 7) == 0) {
            const int L = bx + nx * (by + (int)gridDim.y * bz);
            const int xcd = L & 7, slot = L >> 3;
            const int g = (slot / nx) * 8 + xcd;
            bx = slot % nx;
            by = g % (int)gridDim.y;
            bz = g / (int)gridDim.y;
        }
    }
    const int z = bz / a.nsplit, s = bz - z * a.nsplit;
    const int m0 = by * TM, n0 = bx * SG_T;
    if (a.lower_only && n0 >= m0 + TM) return;
    const int k_begin = s * a.kchunk;
    const int k_end = k_begin + a.kchunk < a.K ? k_begin + a.kchunk : a.K;
    const float *A = a.A + (size_t)z * a.strideA, *B = a.B + (size_t)z * a.strideB;
    float *C = a.C + (size_t)z * a.strideC + (size_t)s * a.strideCs;

    auto ld4 = [](const float *p, bool unaligned) -> f32x4 {
        if (unaligned) {
            const f32x4_u v = *reinterpret_cast<const f32x4_u *>(p);
            return f32x4{v.x, v.y, v.z, v.w};
        }
        return *reinterpret_cast<const f32x4 *>(p);
    };
    // k-contiguous operand with F rows: 256/F threads per row, 16/(256/F) consecutive k each
    // free-index-contiguous operand with F columns: thread = (k row tid>>4, column group tid&15), float4 at columns 4*(tid&15) (+64)
    auto load_tile = [&](const float *P, bool kc, int ld, const long long *off, int f0, int F, auto &r, int k0, auto fw) {
        constexpr int FW = decltype(fw)::value;
        constexpr int NV = FW / 64, TPR = 256 / FW, KPER = SG_K / TPR;
        if (kc) {
            const int row = f0 + tid / TPR, kk = k0 + (tid % TPR) * KPER;
            const bool rv = row < F;
            const int rr = rv ? row : 0;
            const float *p = P + (off ? off[rr] : (long long)rr * ld) + kk;
#pragma unroll
            for (int h = 0; h < NV; ++h) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (rv && kk + 4 * h + 3 < k_end) v = ld4(p + 4 * h, off != nullptr);
                else if (rv) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (kk + 4 * h + j < k_end) v[j] = p[4 * h + j];
                }
                r[h] = v;
            }
        } else {
            const int kk = k0 + (tid >> 4);
            const bool kv = kk < k_end;
            const int kr = kv ? kk : 0;
            const float *p = P + (off ? off[kr] : (long long)kr * ld);
#pragma unroll
            for (int h = 0; h < NV; ++h) {
                const int col = f0 + 4 * (tid & 15) + 64 * h;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (kv && col + 3 < F) v = ld4(p + col, off != nullptr);
                else if (kv) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (col + j < F) v[j] = p[col + j];
                }
                r[h] = v;
            }
        }
    };
    auto store_tile = [&](float *L, bool kc, int stride, const auto &r, auto fw) {
        constexpr int FW = decltype(fw)::value;
        constexpr int NV = FW / 64, TPR = 256 / FW, KPER = SG_K / TPR;
        if (kc) {
            const int row = tid / TPR, kk = (tid % TPR) * KPER;
#pragma unroll
            for (int h = 0; h < NV; ++h)
#pragma unroll
                for (int j = 0; j < 4; ++j) L[(kk + 4 * h + j) * stride + row] = r[h][j];
        } else {
            const int kk = tid >> 4;
#pragma unroll
            for (int h = 0; h < NV; ++h) *reinterpret_cast<f32x4 *>(L + kk * stride + 4 * (tid & 15) + 64 * h) = r[h];
        }
    };

    f32x4 ra[NVA], rb[NVB];
    f32x16 acc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const long long *boff = BOFF ? a.b_off : nullptr;
    const int nsteps = (k_end - k_begin + SG_K - 1) / SG_K;
    if (nsteps > 0) {
        load_tile(A, AK, a.lda, (const long long *)nullptr, m0, a.M, ra, k_begin, IntK<TM>{});
        load_tile(B, BK, a.ldb, boff, n0, a.N, rb, k_begin, IntK<SG_T>{});
        store_tile(lds[0], AK, SA, ra, IntK<TM>{});
        store_tile(lds[0] + SG_K * SA, BK, SG_S, rb, IntK<SG_T>{});
    }
    __syncthreads();
    const int la = wm * 64 + (lane & 31), lb = wn * (SG_T / WN) + (lane & 31), kh = lane >> 5;
    for (int st = 0; st < nsteps; ++st) {
        const int cur = st & 1;
        const bool more = st + 1 < nsteps;
        if (more) {
            load_tile(A, AK, a.lda, (const long long *)nullptr, m0, a.M, ra, k_begin + (st + 1) * SG_K, IntK<TM>{});
            load_tile(B, BK, a.ldb, boff, n0, a.N, rb, k_begin + (st + 1) * SG_K, IntK<SG_T>{});
        }
        const float *La = lds[cur], *Lb = lds[cur] + SG_K * SA;
#pragma unroll
        for (int k2 = 0; k2 < SG_K / 2; ++k2) {
            const int kk = 2 * k2 + kh;
            const float a0 = La[kk * SA + la], a1 = La[kk * SA + la + 32];
            float bv[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) bv[j] = Lb[kk * SG_S + lb + 32 * j];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv[j], acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv[j], acc[1][j], 0, 0, 0);
            }
        }
        if (more) {
            store_tile(lds[cur ^ 1], AK, SA, ra, IntK<TM>{});
            store_tile(lds[cur ^ 1] + SG_K * SA, BK, SG_S, rb, IntK<SG_T>{});
        }
        __syncthreads();
    }

    if (a.ct) {
        // the lane's registers 4*r4 .. 4*r4+3 are rows m .. m+3 of column n: contiguous in the transposed result (M % 4 == 0)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int n = n0 + wn * (SG_T / WN) + j * 32 + (lane & 31);
                if (n >= a.N) continue;
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const int m = m0 + wm * 64 + i * 32 + 8 * r4 + 4 * kh;
                    if (m + 3 < a.M) {
                        const f32x4 v = {acc[i][j][4 * r4], acc[i][j][4 * r4 + 1], acc[i][j][4 * r4 + 2], acc[i][j][4 * r4 + 3]};
                        *reinterpret_cast<f32x4 *>(C + (size_t)n * a.ldc + m) = v;
                    } else {
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (m + u < a.M) C[(size_t)n * a.ldc + m + u] = acc[i][j][4 * r4 + u];
                    }
                }
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (m >= a.M) continue;
            const float bv = a.bias ? a.bias[m] : 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int n = n0 + wn * (SG_T / WN) + j * 32 + (lane & 31);
                if (n < a.N) {
                    float *cp = C + (size_t)m * a.ldc + n;
                    *cp = a.alpha * acc[i][j][r] + bv + (a.accumulate ? *cp : 0.f);
                }
            }
        }
}

// 128-row tiles, rows of B at row * ldb (the dense DCN path)
inline void sgemm_f32(hipStream_t stream, bool ak, bool bk, const SgemmArgs &a, int Z)
{
    dim3 grid((a.N + SG_T - 1) / SG_T, (a.M + SG_T - 1) / SG_T, Z * a.nsplit), block(256);
    if (ak && bk) hipLaunchKernelGGL((sgemm_f32_tile<true, true, 128, false>), grid, block, 0, stream, a);
    else if (ak) hipLaunchKernelGGL((sgemm_f32_tile<true, false, 128, false>), grid, block, 0, stream, a);
    else if (bk) hipLaunchKernelGGL((sgemm_f32_tile<false, true, 128, false>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((sgemm_f32_tile<false, false, 128, false>), grid, block, 0, stream, a);
}

// 64-row tiles, A k-contiguous, rows of B at the offsets a.b_off lists (shifted views: the autocorrelation products of heads.hip)
inline void sgemm_f32_rows64(hipStream_t stream, bool bk, const SgemmArgs &a, int Z)
{
    dim3 grid((a.N + SG_T - 1) / SG_T, (a.M + 63) / 64, Z * a.nsplit), block(256);
    if (bk) hipLaunchKernelGGL((sgemm_f32_tile<true, true, 64, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((sgemm_f32_tile<true, false, 64, true>), grid, block, 0, stream, a);
}

}  // namespace
