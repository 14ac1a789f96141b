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

}  // extern "C"
