// GMW inference (GMW/main.py:524-548 `validate`, GMW/model/model.py:154-199): from the two extractors' features of every edge to the
// refined depth and location of the object, without the 2628 x 2628 distance matrix the training route builds -- refinement reads
// only its diagonal.
//
//   gmw_edge_weights   per edge k: n4 = max(||f4[:, k]||, 1e-12), n6 likewise (F.normalize), d_k = sqrt(max(sum_c (f4/n4 - f6/n6)^2,
//                      1e-30)), w_k = 1 / d_k.  The DIFFERENCE form: `pairwise_l2_dist` expands to ||a||^2 + ||b||^2 - 2 a.b, which
//                      on unit vectors cancels exactly where a trained model puts its mass (matched edges, small d).
//                      Lanes run along the points (contiguous), 16-byte loads when K % 4 == 0; one wave per 256 (64) points, so an
//                      object is ceil(K / 256) workgroups and eight objects already give 88.  Two passes over the C rows of the
//                      wave's own columns (norms, then differences): the second is served by the caches where the tile still
//                      lies there, by memory otherwise -- at most 2 x (2 C K 4) bytes per object.
//   gmw_softmax_depth  one workgroup per object: gathers w and the edge depths at good_idx into LDS (the first 4096; later ones are
//                      gathered again), softmax with the maximum subtracted (two identical columns give w = 1e15 and a one-hot, not
//                      a NaN), z = sum softmax * depth, and the location rule: y -= h/2, scale by z / raw_z, y += h/2.
//   gmw_pack_records   decoded candidates -> GMW's inputs (dcd_gmw_pack_records): one workgroup per record.  The record's 5 nk
//                      key-point floats go to LDS once; lanes run along the pairs p, so each of the 4 + 6 channel rows of
//                      e4 (cap, 4, P) / e6 (cap, 6, P) is written contiguously -- 16-byte stores, four pairs per lane, when P % 4 == 0
//                      and the bases are 16-byte aligned (P = 2628 is), 4-byte stores otherwise.  (i, j) of pair p come from the two
//                      index tables (`GMW.pair_i` / `pair_j`, read as int32, 16 bytes at a time on the wide path), not from p in closed
//                      form: the tables ARE the order `edge_expand` uses, and 21 KB of them stay in L2 for every record.  A table entry
//                      outside [0, nk) gives 0, a source row outside [0, n_rows) a zero record with nothing read.  Pure data movement,
//                      no atomics: every output is bit-equal to `edge_expand(x[src]).transpose(-2, -1).contiguous()` and the row slices.
// Every sum runs in a fixed order (a lane's own loop, xor-shuffles, then the waves in index order): no atomics, and an object's
// result depends neither on its place in the batch nor on B.  An index outside [0, K) makes that object's depth and location NaN.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dcd_hip.h"

namespace {

constexpr int GMW_WAVE = 64;
constexpr int GMW_LDS_EDGES = 4096;

template <int V> struct GmwVec;
template <> struct GmwVec<1> {
    float v[1];
    __device__ __forceinline__ void load(const float *p) { v[0] = *p; }
};
template <> struct GmwVec<4> {
    float v[4];
    __device__ __forceinline__ void load(const float *p)
    {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
};

template <int V>
__global__ __launch_bounds__(GMW_WAVE) void gmw_edge_weights(const float *__restrict__ f4, const float *__restrict__ f6, int C, int K,
                                                             int tiles, float *__restrict__ weights)
{
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int k0 = (tile * GMW_WAVE + threadIdx.x) * V;
    if (k0 >= K) return;                                    // V == 4 only with K % 4 == 0: k0 + 3 < K
    const size_t base = (size_t)b * C * K + k0;
    const float *a = f4 + base, *q = f6 + base;
    float s4[V], s6[V], d[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s4[j] = s6[j] = d[j] = 0.f;
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
        GmwVec<V> x, y;
        x.load(a + (size_t)c * K);
        y.load(q + (size_t)c * K);
#pragma unroll
        for (int j = 0; j < V; ++j) { s4[j] += x.v[j] * x.v[j]; s6[j] += y.v[j] * y.v[j]; }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) { s4[j] = fmaxf(sqrtf(s4[j]), 1e-12f); s6[j] = fmaxf(sqrtf(s6[j]), 1e-12f); }
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
        GmwVec<V> x, y;
        x.load(a + (size_t)c * K);
        y.load(q + (size_t)c * K);
#pragma unroll
        for (int j = 0; j < V; ++j) { const float t = x.v[j] / s4[j] - y.v[j] / s6[j]; d[j] += t * t; }
    }
    float *w = weights + (size_t)b * K + k0;
#pragma unroll
    for (int j = 0; j < V; ++j) w[j] = 1.f / sqrtf(fmaxf(d[j], 1e-30f));
}

__device__ __forceinline__ float gmw_wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ float gmw_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(256) void gmw_softmax_depth(const float *__restrict__ weights, const float *__restrict__ depths,
                                                         const long long *__restrict__ good_idx, int num_k, int K,
                                                         const float *__restrict__ raw_location, const float *__restrict__ dim,
                                                         float *__restrict__ pred_depth, float *__restrict__ pred_location)
{
    __shared__ float sw[GMW_LDS_EDGES], sz[GMW_LDS_EDGES];
    __shared__ float red[3][4];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const long long *idx = good_idx + (size_t)b * num_k;
    const float *w = weights + (size_t)b * K, *z = depths + (size_t)b * K;
    float m = -INFINITY;
    int bad = 0;
    for (int i = tid; i < num_k; i += 256) {
        const long long j = idx[i];
        if (j < 0 || j >= K) { bad = 1; continue; }
        const float v = w[j];
        if (i < GMW_LDS_EDGES) { sw[i] = v; sz[i] = z[j]; }        // read back by this thread only
        m = fmaxf(m, v);
    }
    bad = __syncthreads_or(bad);
    m = gmw_wave_max(m);
    if ((tid & 63) == 0) red[0][wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    float se = 0.f, sez = 0.f;
    if (!bad)
        for (int i = tid; i < num_k; i += 256) {
            float v, zz;
            if (i < GMW_LDS_EDGES) { v = sw[i]; zz = sz[i]; }
            else { const long long j = idx[i]; v = w[j]; zz = z[j]; }
            const float e = expf(v - m);
            se += e;
            sez += e * zz;
        }
    se = gmw_wave_sum(se);
    sez = gmw_wave_sum(sez);
    if ((tid & 63) == 0) { red[1][wave] = se; red[2][wave] = sez; }
    __syncthreads();
    if (tid == 0) {
        se = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        sez = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
        const float depth = bad ? NAN : sez / se;
        const float *loc = raw_location + (size_t)b * 3;
        const float half_h = dim[(size_t)b * 3] / 2.f;
        const float scale = depth / loc[2];
        pred_depth[b] = depth;
        float *out = pred_location + (size_t)b * 3;
        out[0] = scale * loc[0];
        out[1] = scale * (loc[1] - half_h) + half_h;
        out[2] = scale * loc[2];
    }
}

constexpr int GMW_PACK_THREADS = 256;
constexpr int GMW_PACK_MAX_NK = 128;

__device__ __forceinline__ float gmw_pick(const float *s, int idx, int stride, int c, int nk)
{
    return (unsigned)idx < (unsigned)nk ? s[idx * stride + c] : 0.f;
}

template <int V>
__global__ __launch_bounds__(GMW_PACK_THREADS) void gmw_pack_records(const float *__restrict__ rows, const float *__restrict__ k2,
                                                                      const float *__restrict__ k3, int n_rows, int nk,
                                                                      const int *__restrict__ src, int dst0, int P,
                                                                      const int *__restrict__ pair_i, const int *__restrict__ pair_j,
                                                                      float *__restrict__ e4, float *__restrict__ e6,
                                                                      float *__restrict__ k2_out, float *__restrict__ k3_out,
                                                                      float *__restrict__ rot, float *__restrict__ loc,
                                                                      float *__restrict__ dim)
{
    __shared__ float s2[GMW_PACK_MAX_NK * 2], s3[GMW_PACK_MAX_NK * 3];
    const int tid = threadIdx.x;
    const size_t rec = (size_t)dst0 + blockIdx.x;
    const int row = src[blockIdx.x];
    const bool ok = row >= 0 && row < n_rows;                          // uniform over the workgroup
    const float *a2 = k2 + (size_t)(ok ? row : 0) * nk * 2, *a3 = k3 + (size_t)(ok ? row : 0) * nk * 3;
    for (int t = tid; t < nk * 2; t += GMW_PACK_THREADS) {
        const float v = ok ? a2[t] : 0.f;
        s2[t] = v;
        k2_out[rec * nk * 2 + t] = v;
    }
    for (int t = tid; t < nk * 3; t += GMW_PACK_THREADS) {
        const float v = ok ? a3[t] : 0.f;
        s3[t] = v;
        k3_out[rec * nk * 3 + t] = v;
    }
    if (tid < 7) {                                                     // rows: [cls, alpha, box (4), h w l, x y z, ry, score]
        const float v = ok ? rows[(size_t)row * 14 + 6 + tid] : 0.f;
        if (tid < 3) dim[rec * 3 + tid] = v;
        else if (tid < 6) loc[rec * 3 + (tid - 3)] = v;
        else rot[rec] = v;
    }
    __syncthreads();
    float *o4 = e4 + rec * 4 * (size_t)P, *o6 = e6 + rec * 6 * (size_t)P;
    for (int p = tid * V; p < P; p += GMW_PACK_THREADS * V) {          // V == 4 only with P % 4 == 0: p + 3 < P
        int pi[V], pj[V];
        if constexpr (V == 4) {
            const int4 ti = *reinterpret_cast<const int4 *>(pair_i + p), tj = *reinterpret_cast<const int4 *>(pair_j + p);
            pi[0] = ti.x; pi[1] = ti.y; pi[2] = ti.z; pi[3] = ti.w;
            pj[0] = tj.x; pj[1] = tj.y; pj[2] = tj.z; pj[3] = tj.w;
        } else {
            pi[0] = pair_i[p];
            pj[0] = pair_j[p];
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float lo[V], hi[V];
#pragma unroll
            for (int v = 0; v < V; ++v) { lo[v] = gmw_pick(s2, pi[v], 2, c, nk); hi[v] = gmw_pick(s2, pj[v], 2, c, nk); }
            if constexpr (V == 4) {
                *reinterpret_cast<float4 *>(o4 + (size_t)c * P + p) = make_float4(lo[0], lo[1], lo[2], lo[3]);
                *reinterpret_cast<float4 *>(o4 + (size_t)(c + 2) * P + p) = make_float4(hi[0], hi[1], hi[2], hi[3]);
            } else {
                o4[(size_t)c * P + p] = lo[0];
                o4[(size_t)(c + 2) * P + p] = hi[0];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float lo[V], hi[V];
#pragma unroll
            for (int v = 0; v < V; ++v) { lo[v] = gmw_pick(s3, pi[v], 3, c, nk); hi[v] = gmw_pick(s3, pj[v], 3, c, nk); }
            if constexpr (V == 4) {
                *reinterpret_cast<float4 *>(o6 + (size_t)c * P + p) = make_float4(lo[0], lo[1], lo[2], lo[3]);
                *reinterpret_cast<float4 *>(o6 + (size_t)(c + 3) * P + p) = make_float4(hi[0], hi[1], hi[2], hi[3]);
            } else {
                o6[(size_t)c * P + p] = lo[0];
                o6[(size_t)(c + 3) * P + p] = hi[0];
            }
        }
    }
}

}  // namespace

extern "C" {

int dcd_gmw_refine(void *stream_, const float *f4, const float *f6, const float *depths, const long long *good_idx, int num_k,
                   const float *raw_location, const float *dim, int B, int C, int K, float *weights, float *pred_depth,
                   float *pred_location)
{
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (B < 1 || C < 1 || K < 1 || num_k < 1 || num_k > K) return DCD_ERR_BAD_ARG;
    if (!f4 || !f6 || !depths || !good_idx || !raw_location || !dim || !weights || !pred_depth || !pred_location) return DCD_ERR_BAD_ARG;
    const bool vec = (K & 3) == 0 && (((uintptr_t)f4 | (uintptr_t)f6) & 15) == 0;
    const int per_tile = GMW_WAVE * (vec ? 4 : 1);
    const int tiles = (K + per_tile - 1) / per_tile;
    if ((int64_t)tiles * B > INT32_MAX) return DCD_ERR_BAD_ARG;
    if (vec)
        hipLaunchKernelGGL(gmw_edge_weights<4>, dim3((unsigned)(tiles * B)), dim3(GMW_WAVE), 0, stream, f4, f6, C, K, tiles, weights);
    else
        hipLaunchKernelGGL(gmw_edge_weights<1>, dim3((unsigned)(tiles * B)), dim3(GMW_WAVE), 0, stream, f4, f6, C, K, tiles, weights);
    if (hipGetLastError() != hipSuccess) return DCD_ERR_LAUNCH;
    hipLaunchKernelGGL(gmw_softmax_depth, dim3((unsigned)B), dim3(256), 0, stream, weights, depths, good_idx, num_k, K, raw_location,
                       dim, pred_depth, pred_location);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}

int dcd_gmw_pack_records(void *stream_, const float *rows, const float *k2, const float *k3, int n_rows, int nk, const int *src, int n,
                         int dst0, int cap, const int *pair_i, const int *pair_j, float *e4, float *e6, float *k2_out, float *k3_out,
                         float *rot, float *loc, float *dim)
{
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (n < 0 || n_rows < 0 || dst0 < 0 || cap < 0 || (int64_t)dst0 + n > cap || nk < 2 || nk > GMW_PACK_MAX_NK) return DCD_ERR_BAD_ARG;
    if (!rows || !k2 || !k3 || !src || !pair_i || !pair_j || !e4 || !e6 || !k2_out || !k3_out || !rot || !loc || !dim) return DCD_ERR_BAD_ARG;
    if (n == 0) return DCD_OK;
    const int P = nk * (nk - 1) / 2;
    const bool vec = (P & 3) == 0 && (((uintptr_t)e4 | (uintptr_t)e6 | (uintptr_t)pair_i | (uintptr_t)pair_j) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(gmw_pack_records<4>, dim3((unsigned)n), dim3(GMW_PACK_THREADS), 0, stream, rows, k2, k3, n_rows, nk, src, dst0, P,
                           pair_i, pair_j, e4, e6, k2_out, k3_out, rot, loc, dim);
    else
        hipLaunchKernelGGL(gmw_pack_records<1>, dim3((unsigned)n), dim3(GMW_PACK_THREADS), 0, stream, rows, k2, k3, n_rows, nk, src, dst0, P,
                           pair_i, pair_j, e4, e6, k2_out, k3_out, rot, loc, dim);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}

}  // extern "C"
