// DENSE path of the deformable convolution: sampled-column buffer + three matrix products (sgemm_f32.inc; under
// DCD_PREC_BF16X3 the same products on sgemm_bf16x3.inc).
//
// Which layers: wide inputs on small maps (DGDE: 512->256 @ 12x40, 256->{256,128,64} @ 24x80).  There the fused kernels
// of dcn_v2.hip run at 13-25 TF (few hundred workgroups, gathers in the MFMA loop, far samples from large fan-in offset
// convolutions), while the column buffer is only 70-140 MB at batch 8 and a plain GEMM reaches 80-100 TF.  The dense path does
// not care how large the offsets are: every sample is gathered straight from the (L2-resident) input plane.
//
//   forward   col[b][c*KK+t][p] = mask * bilinear(x[b,c], p, t)            dcn_dense_im2col
//             Y[b] = W (Cout x K9) * col[b] (K9 x HoWo) + bias              sgemm (A k-contiguous), split-K when few tiles
//   backward  T[b] = Wb^T (Kp x Cout) * dY[b] (Cout x HoWo), stored TRANSPOSED: Tt[b][p][seg*cpgp + c]   sgemm (ct = 1)
//                 (Wb = dcn_prep_weights' [Cout][(group, tap), channel] layout: a pixel's channels of one tap are contiguous,
//                 so the two consumers below read 16-byte pieces instead of one dword per channel)
//             grad_input[b,c,q] = sum_t sum_{(p,w) in list(q,t)} w * Tt[b][p][t,c]          dcn_dense_col2im (inverse lists)
//             grad_offset / grad_mask [b,t,p] = sum_c Tt[b][p][t,c] * d(sample)/d(.)         dcn_dense_coord_grad
//                 (+ atomics into grad_input for what the lists do not hold: samples beyond the search radius, overflowed cells)
//             col again (same buffer), dW = sum_b dY[b] (Cout x HoWo) * col[b]^T            sgemm (both k-contiguous), split
//             over images and pixel chunks into partials, summed in a fixed order (dcn_dense_reduce)
// Reference: cuda/dcn_v2_cuda.cu:88-113 (forward: im2col + gemm per image), :258-327 (backward: gemm, col2im_coord, col2im,
// im2col, gemm per image), cuda/dcn_v2_im2col_cuda.cu:126-190 (im2col), :193-262 (col2im), :265-352 (col2im_coord).
#pragma once
#include "sgemm_f32.inc"
#include "sgemm_bf16x3.inc"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
// 4-byte aligned 8-byte load (global memory allows it)
__device__ __forceinline__ f32x2 ld2(const float *p)
{
    typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
    const f32x2u v = *reinterpret_cast<const f32x2u *>(p);
    return f32x2{v.x, v.y};
}

// one thread per output pixel (lane) and tap (blockIdx.y); the four waves split the group's channels
__global__ __launch_bounds__(256) void dcn_dense_im2col(const float *__restrict__ in, const float *__restrict__ off,
                                                        const float *__restrict__ msk, float *__restrict__ col, Geom g)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int P = blockIdx.x * 64 + lane, seg = blockIdx.y, b = blockIdx.z;
    const bool pv = P < g.HoWo;
    const int Pc = pv ? P : g.HoWo - 1;
    const int ho = Pc / g.Wo, wo = Pc - ho * g.Wo;
    const int grp = seg / g.KK, t = seg - grp * g.KK;
    const int HW = g.H * g.W;
    const Tap s = make_tap(off + (size_t)b * g.dg * 2 * g.KK * g.HoWo, msk + (size_t)b * g.dg * g.KK * g.HoWo, g, seg, t, ho, wo, Pc, pv);
    // pair form: the two corners of a row are adjacent floats -> one (4-byte aligned) dwordx2 gather per row
    const float a0 = s.a0 * s.m, a1 = s.a1 * s.m, b0 = s.b0 * s.m, b1 = s.b1 * s.m;
    const int cq = (g.cpg + 3) / 4;
    const int c_lo = wave * cq, c_hi = min(g.cpg, c_lo + cq);
    const float *ip = in + ((size_t)b * g.C + (size_t)grp * g.cpg + c_lo) * HW;
    float *cp = col + ((size_t)b * g.C * g.KK + ((size_t)grp * g.cpg + c_lo) * g.KK + t) * g.HoWo + Pc;
    const size_t cstep = (size_t)g.KK * g.HoWo;
    int cc = c_lo;
    auto chunk = [&](auto n_tag) {                              // N channels: all 2N gathers in flight, then N stores
        constexpr int N = decltype(n_tag)::value;
        f32x2 vt[N], vb[N];
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const float *pl = ip + (size_t)u * HW;
            vt[u] = ld2(pl + s.pt);
            vb[u] = ld2(pl + s.pb);
        }
        if (pv) {
#pragma unroll
            for (int u = 0; u < N; ++u) cp[(size_t)u * cstep] = a0 * vt[u].x + a1 * vt[u].y + b0 * vb[u].x + b1 * vb[u].y;
        }
        ip += (size_t)N * HW;
        cp += N * cstep;
    };
    for (; cc + 8 <= c_hi; cc += 8) chunk(IntC<8>{});
    for (; cc + 4 <= c_hi; cc += 4) chunk(IntC<4>{});
    for (; cc < c_hi; ++cc) {
        const f32x2 vt = ld2(ip + s.pt), vb = ld2(ip + s.pb);
        if (pv) *cp = a0 * vt.x + a1 * vt.y + b0 * vb.x + b1 * vb.y;
        ip += HW;
        cp += cstep;
    }
}

// grad_input from T through the inverse lists: thread = input cell (lane), wave = 16 consecutive channels.
// grid = (ceil(HW/64), ceil(C/64), B).  Plain stores: every cell of grad_input is written.
constexpr int DN_CH = 8;         // channels per thread (cpg % 16 == 0 is required by the coordinate kernel, so this divides cpg)

__global__ __launch_bounds__(256) void dcn_dense_col2im(const float *__restrict__ T, InvLists inv, float *__restrict__ gin, Geom g)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int HW = g.H * g.W;
    const int q = blockIdx.x * 64 + lane, b = blockIdx.z;
    const int c0 = (blockIdx.y * 4 + wave) * DN_CH;
    if (c0 >= g.C) return;                                     // wave-uniform
    const bool qv = q < HW;
    const int Qc = qv ? q : HW - 1;
    const int grp = c0 / g.cpg;                                // cpg % DN_CH == 0 (host check): one group per wave
    const int S = g.dg * g.KK;
    float acc[DN_CH];
#pragma unroll
    for (int u = 0; u < DN_CH; ++u) acc[u] = 0.f;
    for (int t = 0; t < g.KK; ++t) {
        const int seg = grp * g.KK + t;
        int cnt = qv ? (int)inv.cnt[((size_t)b * S + seg) * HW + Qc] : 0;
        if (cnt == INV_OVERFLOW) cnt = 0;                      // the coordinate kernel scatters this cell's samples
        int maxc = cnt;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) maxc = max(maxc, __shfl_xor(maxc, o));
        if (maxc == 0) continue;
        const int mu = __builtin_amdgcn_readfirstlane(maxc);
        unsigned ei[INV_CAP];                                  // byte offset of the listed pixel's row in Tt (uniform base + 32-bit offset)
        float ew[INV_CAP];
        const size_t base = ((size_t)b * S + seg) * INV_CAP * HW + Qc;
#pragma unroll
        for (int e = 0; e < INV_CAP; ++e) {
            int ri = 0;
            float rw = 0.f;
            if (e < mu) {                                      // scalar branch; slots past cnt hold stale words, masked below
                ri = inv.idx[base + (size_t)e * HW];
                rw = inv.w[base + (size_t)e * HW];
            }
            ei[e] = e < cnt ? (unsigned)ri * (unsigned)g.Kp * 4u : 0u;
            ew[e] = e < cnt ? rw : 0.f;
        }
        const float *Tp = T + (size_t)b * g.HoWo * g.Kp + (size_t)seg * g.cpgp + (c0 - grp * g.cpg);
        auto run = [&](auto ne_tag) {
            constexpr int NE = decltype(ne_tag)::value;
            // two entries (eight 16-byte gathers) in flight at a time: more would cost the occupancy that hides their latency
#pragma unroll
            for (int e0 = 0; e0 < NE; e0 += 2) {
                f32x4 v[2][DN_CH / 4];
#pragma unroll
                for (int e = 0; e < 2; ++e)
#pragma unroll
                    for (int u4 = 0; u4 < DN_CH / 4; ++u4)
                        v[e][u4] = *reinterpret_cast<const f32x4 *>((const char *)Tp + ei[e0 + e] + 16 * u4);
#pragma unroll
                for (int e = 0; e < 2; ++e)
#pragma unroll
                    for (int u = 0; u < DN_CH; ++u) acc[u] += ew[e0 + e] * v[e][u >> 2][u & 3];
            }
        };
        if (mu <= 2) run(IntC<2>{});
        else if (mu <= 4) run(IntC<4>{});
        else if (mu <= 6) run(IntC<6>{});
        else if (mu <= 8) run(IntC<8>{});
        else run(IntC<INV_CAP>{});
    }
    if (qv) {
        float *gp = gin + ((size_t)b * g.C + c0) * HW + q;
#pragma unroll
        for (int u = 0; u < DN_CH; ++u)
            if (c0 + u < g.C) gp[(size_t)u * HW] = acc[u];
    }
}

// grad_offset / grad_mask from T; thread = output pixel (lane), blockIdx.y = (group, tap), the four waves split the
// group's channels and meet in LDS.  Samples the inverse lists do not hold are scattered into grad_input here (after
// dcn_dense_col2im's plain stores, same stream).
__global__ __launch_bounds__(256) void dcn_dense_coord_grad(const float *__restrict__ in, const float *__restrict__ off,
                                                            const float *__restrict__ msk, const float *__restrict__ T,
                                                            float *__restrict__ goff, float *__restrict__ gmsk,
                                                            float *__restrict__ gin, Geom g, InvLists inv)
{
    __shared__ float red[3][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int P = blockIdx.x * 64 + lane, seg = blockIdx.y, b = blockIdx.z;
    const bool pv = P < g.HoWo;
    const int Pc = pv ? P : g.HoWo - 1;
    const int ho = Pc / g.Wo, wo = Pc - ho * g.Wo;
    const int grp = seg / g.KK, t = seg - grp * g.KK;
    const int HW = g.H * g.W;
    const int S = g.dg * g.KK;
    const Tap s = make_tap(off + (size_t)b * S * 2 * g.HoWo, msk + (size_t)b * S * g.HoWo, g, seg, t, ho, wo, Pc, pv);
    const float rlim = (float)inv_radius(inv.absmax_bits);
    const bool far = !(fabsf(s.oh) <= rlim && fabsf(s.ow) <= rlim);
    bool o1 = false, o2 = false, o3 = false, o4 = false;
    if (inv.absmax_bits[2] != 0u) {                            // uniform, normally false
        const unsigned char *cnt_p = inv.cnt + ((size_t)b * S + seg) * HW;
        o1 = cnt_p[s.i1] == INV_OVERFLOW; o2 = cnt_p[s.i2] == INV_OVERFLOW;
        o3 = cnt_p[s.i3] == INV_OVERFLOW; o4 = cnt_p[s.i4] == INV_OVERFLOW;
    }
    const bool a1 = pv && s.c1 && (far || o1), a2 = pv && s.c2 && (far || o2);
    const bool a3 = pv && s.c3 && (far || o3), a4 = pv && s.c4 && (far || o4);
    const bool scatter = __any(a1 | a2 | a3 | a4);

    const int cq = g.cpg / 4;                                  // cpg % 16 == 0 (host check): four-channel pieces stay aligned
    const int c_lo = wave * cq, c_hi = c_lo + cq;
    const float *ip = in + ((size_t)b * g.C + (size_t)grp * g.cpg + c_lo) * HW;
    float *gp = gin + ((size_t)b * g.C + (size_t)grp * g.cpg + c_lo) * HW;
    const float *tp = T + ((size_t)b * g.HoWo + Pc) * g.Kp + (size_t)seg * g.cpgp + c_lo;
    float s_m = 0.f, s_h = 0.f, s_w = 0.f;
    auto one = [&](float d, const f32x2 &top, const f32x2 &bot, float *gpc) {
        // un-map the pairs onto the four corners (finish_tap: shift = +1 at the left image edge, -1 at the right one)
        const float v1 = s.c1 ? (s.shift == -1 ? top.y : top.x) : 0.f, v2 = s.c2 ? (s.shift == 1 ? top.x : top.y) : 0.f;
        const float v3 = s.c3 ? (s.shift == -1 ? bot.y : bot.x) : 0.f, v4 = s.c4 ? (s.shift == 1 ? bot.x : bot.y) : 0.f;
        s_m += d * (s.w1 * v1 + s.w2 * v2 + s.w3 * v3 + s.w4 * v4);
        const float dm = d * s.m;
        // d/dh and d/dw of the bilinear sample (cuda/dcn_v2_im2col_cuda.cu:82-123)
        s_h += dm * (s.hw * (v3 - v1) + s.lw * (v4 - v2));
        s_w += dm * (s.hh * (v2 - v1) + s.lh * (v4 - v3));
        if (scatter) {
            if (a1) atomicAdd(gpc + s.i1, dm * s.w1);
            if (a2) atomicAdd(gpc + s.i2, dm * s.w2);
            if (a3) atomicAdd(gpc + s.i3, dm * s.w3);
            if (a4) atomicAdd(gpc + s.i4, dm * s.w4);
        }
    };
    auto chunk = [&](auto n_tag) {                              // N (4 or 8) channels: 2N corner gathers + N/4 T loads in flight
        constexpr int N = decltype(n_tag)::value;
        f32x2 vt[N], vb[N];
        f32x4 d[N / 4];
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const float *pl = ip + (size_t)u * HW;
            vt[u] = ld2(pl + s.pt);
            vb[u] = ld2(pl + s.pb);
        }
#pragma unroll
        for (int q = 0; q < N / 4; ++q) d[q] = *reinterpret_cast<const f32x4 *>(tp + 4 * q);
#pragma unroll
        for (int u = 0; u < N; ++u) one(pv ? d[u >> 2][u & 3] : 0.f, vt[u], vb[u], gp + (size_t)u * HW);
        ip += (size_t)N * HW;
        gp += (size_t)N * HW;
        tp += N;
    };
    int cc = c_lo;
    for (; cc + 8 <= c_hi; cc += 8) chunk(IntC<8>{});
    for (; cc < c_hi; cc += 4) chunk(IntC<4>{});
    red[0][wave][lane] = s_m;
    red[1][wave][lane] = s_h;
    red[2][wave][lane] = s_w;
    __syncthreads();
    if (wave == 0 && pv) {
        const float m_ = (red[0][0][lane] + red[0][1][lane]) + (red[0][2][lane] + red[0][3][lane]);
        const float h_ = (red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane]);
        const float w_ = (red[2][0][lane] + red[2][1][lane]) + (red[2][2][lane] + red[2][3][lane]);
        goff[((size_t)b * S + seg) * 2 * g.HoWo + P] = h_;
        goff[((size_t)b * S + seg) * 2 * g.HoWo + g.HoWo + P] = w_;
        gmsk[((size_t)b * S + seg) * g.HoWo + P] = m_;
    }
}

// out[z][i] = sum_s part[z][s][i] (+ bias[i / N]); fixed order -> deterministic
__global__ void dcn_dense_reduce(const float *__restrict__ part, float *__restrict__ out, const float *__restrict__ bias,
                                 int n, int S, int N)
{
    const int z = blockIdx.y;
    const float *p = part + (size_t)z * S * n;
    float *o = out + (size_t)z * n;
    for (int i = (blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += gridDim.x * blockDim.x * 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (i + 3 < n) {
            for (int s = 0; s < S; ++s) acc += *reinterpret_cast<const f32x4 *>(p + (size_t)s * n + i);
            if (bias) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] += bias[(i + j) / N];
            }
            *reinterpret_cast<f32x4 *>(o + i) = acc;
        } else {
            for (int j = 0; i + j < n; ++j) {
                float a = 0.f;
                for (int s = 0; s < S; ++s) a += p[(size_t)s * n + i + j];
                o[i + j] = a + (bias ? bias[(i + j) / N] : 0.f);
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
inline void dense_im2col(hipStream_t stream, const float *input, const float *offset, const float *mask, float *col, const Geom &g)
{
    hipLaunchKernelGGL(dcn_dense_im2col, dim3((g.HoWo + 63) / 64, g.dg * g.KK, g.B), dim3(256), 0, stream, input, offset, mask, col, g);
}

// split: the three products on the bf16 matrix cores with split operands (DCD_PREC_BF16X3, sgemm_bf16x3.inc); sampling, the
// column buffer and every reduction stay fp32
// prec: DCD_PREC_F32 / DCD_PREC_BF16X3 / DCD_PREC_BF16 (one product of bf16-rounded operands)
inline void dense_gemm(hipStream_t stream, int prec, bool ak, bool bk, const SgemmArgs &a, int Z)
{
    if (prec != DCD_PREC_F32) sgemm_bf16x3(stream, ak, bk, a, Z, prec == DCD_PREC_BF16);
    else sgemm_f32(stream, ak, bk, a, Z);
}

inline void dense_forward(hipStream_t stream, const float *input, const float *weight, const float *bias, const float *offset,
                          const float *mask, float *output, const Geom &g, const DcnWorkspace &m, void *workspace, int split)
{
    const DensePlan &p = m.dense;
    const int K9 = g.C * g.KK;
    float *col = m.dense_col.in<float>(workspace), *part = m.dense_part.in<float>(workspace);
    dense_im2col(stream, input, offset, mask, col, g);
    SgemmArgs a;
    a.A = weight; a.B = col; a.M = g.Co; a.N = g.HoWo; a.K = K9; a.lda = K9; a.ldb = g.HoWo; a.ldc = g.HoWo;
    a.strideA = 0; a.strideB = (long long)K9 * g.HoWo;
    a.nsplit = p.fwd_split; a.kchunk = p.fwd_kchunk; a.ct = 0; a.b_off = nullptr;
    if (p.fwd_split == 1) {
        a.C = output; a.bias = bias; a.strideC = (long long)g.Co * g.HoWo; a.strideCs = 0;
        dense_gemm(stream, split, true, false, a, g.B);
    } else {
        const int n = g.Co * g.HoWo;
        a.C = part; a.bias = nullptr; a.strideC = (long long)p.fwd_split * n; a.strideCs = n;
        dense_gemm(stream, split, true, false, a, g.B);
        hipLaunchKernelGGL(dcn_dense_reduce, dim3((n / 4 + 255) / 256 < 256 ? (n / 4 + 255) / 256 : 256, g.B), dim3(256), 0, stream,
                           part, output, bias, n, p.fwd_split, g.HoWo);
    }
}

// after: dcn_prep_weights (Wb), zero_ranges (grad_bias), dcn_offset_absmax, dcn_build_inverse (unpacked lists)
inline void dense_backward(hipStream_t stream, const float *input, const float *wb, const float *offset, const float *mask,
                           const float *grad_output, float *grad_input, float *grad_offset, float *grad_mask, float *grad_weight,
                           const Geom &g, const InvLists &inv, const DcnWorkspace &m, void *workspace, int split)
{
    const DensePlan &p = m.dense;
    const int K9 = g.C * g.KK, HW = g.H * g.W;
    float *col = m.dense_col.in<float>(workspace), *part = m.dense_part.in<float>(workspace);
    SgemmArgs a;
    // Tt[b][p][kp] = sum_o Wb[o][kp] dY[b][o][p]
    a.A = wb; a.B = grad_output; a.C = col; a.bias = nullptr; a.M = g.Kp; a.N = g.HoWo; a.K = g.Co;
    a.lda = g.Kp; a.ldb = g.HoWo; a.ldc = g.Kp; a.ct = 1; a.b_off = nullptr;
    a.strideA = 0; a.strideB = (long long)g.Co * g.HoWo; a.strideC = (long long)g.Kp * g.HoWo; a.strideCs = 0;
    a.nsplit = 1; a.kchunk = (g.Co + SG_K - 1) / SG_K * SG_K;
    dense_gemm(stream, split, false, false, a, g.B);
    hipLaunchKernelGGL(dcn_dense_col2im, dim3((HW + 63) / 64, (g.C + 4 * DN_CH - 1) / (4 * DN_CH), g.B), dim3(256), 0, stream,
                       col, inv, grad_input, g);
    hipLaunchKernelGGL(dcn_dense_coord_grad, dim3((g.HoWo + 63) / 64, g.dg * g.KK, g.B), dim3(256), 0, stream, input, offset, mask,
                       col, grad_offset, grad_mask, grad_input, g, inv);
    // dW = sum_b dY[b] col[b]^T
    dense_im2col(stream, input, offset, mask, col, g);
    const int n = g.Co * K9;
    a.A = grad_output; a.B = col; a.C = part; a.bias = nullptr; a.M = g.Co; a.N = K9; a.K = g.HoWo;
    a.lda = g.HoWo; a.ldb = g.HoWo; a.ldc = K9;
    a.strideA = (long long)g.Co * g.HoWo; a.strideB = (long long)K9 * g.HoWo;
    a.strideC = (long long)p.dw_split * n; a.strideCs = n;
    a.nsplit = p.dw_split; a.kchunk = p.dw_kchunk; a.ct = 0;
    dense_gemm(stream, split, true, true, a, g.B);
    hipLaunchKernelGGL(dcn_dense_reduce, dim3((n / 4 + 255) / 256 < 512 ? (n / 4 + 255) / 256 : 512, 1), dim3(256), 0, stream,
                       part, grad_weight, (const float *)nullptr, n, g.B * p.dw_split, 1);
}

}  // namespace
