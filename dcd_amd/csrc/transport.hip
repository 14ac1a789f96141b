// transport.hip -- the Sinkhorn forward of the transport layer (dcd_amd/gmw/optimal_transport.py) without the host.
//
// The stock loop asks the host before every iteration whether any entry of the row scaling u of ANY object moved by more than the
// tolerance (`torch.all(torch.isclose(...))`, up to 100 device-to-host reads per forward).  Here ONE call enqueues everything and
// the question is answered on the device:
//
//   moved[t]   one int per iteration, cleared by a launch (zero_fill.h).  moved[0] is raised by the first kernel when some
//              |r - 1| exceeds the tolerance (u = r, previous = 1 before the first iteration); the kernel that updates u in
//              iteration t raises moved[t + 1] with an integer atomic when an entry moved by more than the tolerance.
//   the two kernels of iteration t return at once when moved[t] is 0.  Their own moved[t + 1] then stays 0, so every later launch
//   returns too: after the stop the remaining launches are empty.  No kernel waits for another workgroup -- no grid barrier, no
//   spinning, no cooperative launch; the only ordering is the stream's kernel-after-kernel order.
//
// Launches of one call:
//   zero_fill            moved[0 .. max_iterations]
//   sinkhorn_gibbs       K = exp(-lambda min(M, max_distance)) written INTO P's buffer, u = r, moved[0], and the strips' partial
//                        column sums of K^T u
//   sinkhorn_columns     v = c / (sum of the strips' partials, in strip order)
//   per iteration t:     sinkhorn_sweep    u_i = r_i / (K_i . v), moved[t + 1], and -- from the same registers -- the strip's
//                                          partial column sums sum_i K_ij u_i
//                        sinkhorn_columns  v = c / K^T u
//   sinkhorn_scale       P = (u K) v in place (the association of the stock path), iterations = number of updates of u that ran
//
// A workgroup of 256 threads owns a strip of 8 rows.  Lane t owns the columns 4 (256 k + t) .. + 3 of every row, k = 0, 1, ...;
// up to n = 4096 the strip stays in registers between the row products and the column sums (8 x 16 floats per lane), so the matrix
// is read once per iteration; wider rows are read a second time, from the cache.  The column assignment is the same whether a
// lane fetches its four columns as one 16-byte access (n % 4 == 0 and M, P 16-byte aligned) or as four 4-byte accesses, and the
// choice is a kernel argument in front of one copy of the arithmetic, so both give the same bits.  Every sum runs in a fixed
// order: a lane adds its columns in order, the 64 lanes of a wave combine in a butterfly, the four waves are added in wave order;
// column sums add the 8 rows of a strip in row order and then the strips in strip order.  No floating-point atomics; nothing depends on an object's place in the batch except the shared stop.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dcd_hip.h"
#include "zero_fill.h"

namespace {

constexpr int SK_THREADS = 256;
constexpr int SK_ROWS = 8;                               // rows of a strip
constexpr int SK_SPAN = SK_THREADS * 4;                  // columns one pass of the workgroup covers
constexpr int SK_HOLD = 4;                               // passes whose values stay in registers (n <= 4096)
constexpr int SK_MAX_ITERATIONS = 4096;                  // moved[] is sized for this many

struct SkLayout {
    size_t u, v, part, moved, total;                     // byte offsets into the workspace
    int n4, strips;
};

inline SkLayout sk_layout(int batch, int m, int n)
{
    SkLayout l;
    l.n4 = (n + 3) / 4 * 4;                              // v and the partials: rows padded to 16 bytes, the padding holds zeros
    l.strips = (m + SK_ROWS - 1) / SK_ROWS;
    size_t o = 0;
    l.v = o;     o += (size_t)batch * l.n4 * sizeof(float);
    l.part = o;  o += (size_t)batch * l.strips * l.n4 * sizeof(float);
    l.u = o;     o += ((size_t)batch * m + 3) / 4 * 4 * sizeof(float);
    l.moved = o; o += (size_t)(SK_MAX_ITERATIONS + 4) * sizeof(int);
    l.total = o;
    return l;
}

// `vec` is uniform over the launch and a kernel ARGUMENT, not a template parameter: both routes then feed ONE copy of the
// arithmetic, so the compiler cannot contract or schedule it differently for the two and the bits agree by construction.
__device__ inline float4 sk_load(const float *__restrict__ row, int col, int n, int vec)
{
    if (vec) return *(const float4 *)(row + col);        // n % 4 == 0: col < n implies col + 3 < n
    float4 k;
    k.x = row[col];
    k.y = col + 1 < n ? row[col + 1] : 0.f;
    k.z = col + 2 < n ? row[col + 2] : 0.f;
    k.w = col + 3 < n ? row[col + 3] : 0.f;
    return k;
}

__device__ inline void sk_store(float *__restrict__ row, int col, int n, int vec, float4 k)
{
    if (vec) {
        *(float4 *)(row + col) = k;
        return;
    }
    row[col] = k.x;
    if (col + 1 < n) row[col + 1] = k.y;
    if (col + 2 < n) row[col + 2] = k.z;
    if (col + 3 < n) row[col + 3] = k.w;
}

// |a - b| <= tol is `torch.isclose(a, b, atol=tol, rtol=0)` for finite values; equal infinities are close, a NaN never is
__device__ inline bool sk_moved(float a, float b, float tol) { return !(fabsf(a - b) <= tol) && a != b; }

// the sums of SK_ROWS per-lane values over the workgroup, in a fixed order; every lane gets every sum
__device__ inline void sk_row_sums(float (&acc)[SK_ROWS], float (*lds)[SK_THREADS / 64])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < SK_ROWS; ++r) {
        float s = acc[r];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) lds[r][wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SK_ROWS; ++r) acc[r] = ((lds[r][0] + lds[r][1]) + lds[r][2]) + lds[r][3];
}

// K into P's buffer, u = r, moved[0], partial column sums of K^T r.  grid (strips, batch)
__global__ __launch_bounds__(SK_THREADS) void sinkhorn_gibbs(const float *__restrict__ M, const float *__restrict__ r, float *__restrict__ K,
                                                             float *__restrict__ u, float *__restrict__ part, int *__restrict__ moved,
                                                             int m, int n, int n4, int vec, float lambda, float max_distance, float tol)
{
    const int b = blockIdx.y, strip = blockIdx.x, row0 = strip * SK_ROWS;
    const int rows = min(SK_ROWS, m - row0);
    const size_t base = ((size_t)b * m + row0) * n;
    float rv[SK_ROWS];
#pragma unroll
    for (int i = 0; i < SK_ROWS; ++i) rv[i] = i < rows ? r[(size_t)b * m + row0 + i] : 0.f;
    if (threadIdx.x < rows) {
        const float ri = r[(size_t)b * m + row0 + threadIdx.x];
        u[(size_t)b * m + row0 + threadIdx.x] = ri;
        if (sk_moved(ri, 1.f, tol)) atomicOr(moved, 1);
    }
    float *prow = part + ((size_t)b * gridDim.x + strip) * n4;
    for (int col = threadIdx.x * 4; col < n4; col += SK_SPAN) {
        float4 s = {0.f, 0.f, 0.f, 0.f};
        if (col < n) {
#pragma unroll
            for (int i = 0; i < SK_ROWS; ++i) {
                if (i < rows) {
                    float4 d = sk_load(M + base + (size_t)i * n, col, n, vec), k;
                    k.x = expf(-lambda * (d.x > max_distance ? max_distance : d.x));
                    k.y = expf(-lambda * (d.y > max_distance ? max_distance : d.y));
                    k.z = expf(-lambda * (d.z > max_distance ? max_distance : d.z));
                    k.w = expf(-lambda * (d.w > max_distance ? max_distance : d.w));
                    sk_store(K + base + (size_t)i * n, col, n, vec, k);
                    s.x += k.x * rv[i];
                    s.y += k.y * rv[i];
                    s.z += k.z * rv[i];
                    s.w += k.w * rv[i];
                }
            }
            if (col + 1 >= n) s.y = 0.f;
            if (col + 2 >= n) s.z = 0.f;
            if (col + 3 >= n) s.w = 0.f;
        }
        *(float4 *)(prow + col) = s;
    }
}

// v = c / (the strips' partials added in strip order); the padding of v's rows is zero.  grid (ceil(n4 / 256), batch)
__global__ __launch_bounds__(SK_THREADS) void sinkhorn_columns(const float *__restrict__ part, const float *__restrict__ c, float *__restrict__ v,
                                                               const int *__restrict__ gate, int strips, int n, int n4)
{
    if (gate && *gate == 0) return;
    const int b = blockIdx.y, col = blockIdx.x * SK_THREADS + threadIdx.x;
    if (col >= n4) return;
    float out = 0.f;
    if (col < n) {
        const float *p = part + (size_t)b * strips * n4 + col;
        float s = 0.f;
#pragma unroll 8
        for (int k = 0; k < strips; ++k) s += p[(size_t)k * n4];
        out = c[(size_t)b * n + col] / s;
    }
    v[(size_t)b * n4 + col] = out;
}

// One update of u for a strip, and the strip's partial column sums of K^T u.  NC > 0: the strip's NC passes stay in registers;
// NC == 0: any n, the matrix is read twice.  grid (strips, batch)
template <int NC>
__global__ __launch_bounds__(SK_THREADS) void sinkhorn_sweep(const float *__restrict__ K, const float *__restrict__ r, const float *__restrict__ v,
                                                             float *__restrict__ u, float *__restrict__ part, int *__restrict__ moved, int m, int n,
                                                             int n4, int vec, float tol)
{
    if (moved[0] == 0) return;                            // moved points at this iteration's flag
    __shared__ float lds[SK_ROWS][SK_THREADS / 64];
    const int b = blockIdx.y, strip = blockIdx.x, row0 = strip * SK_ROWS;
    const int rows = min(SK_ROWS, m - row0);
    const float *krow = K + ((size_t)b * m + row0) * n;
    const float *vrow = v + (size_t)b * n4;
    constexpr int NH = NC > 0 ? NC : 1;
    float4 hold[SK_ROWS][NH];
    float acc[SK_ROWS];
#pragma unroll
    for (int i = 0; i < SK_ROWS; ++i) acc[i] = 0.f;
    if (NC > 0) {
#pragma unroll
        for (int k = 0; k < NH; ++k) {
            const int col = k * SK_SPAN + threadIdx.x * 4;
            const bool in = col < n;
            const float4 vv = in ? *(const float4 *)(vrow + col) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int i = 0; i < SK_ROWS; ++i) {
                float4 kk = {0.f, 0.f, 0.f, 0.f};
                if (in && i < rows) kk = sk_load(krow + (size_t)i * n, col, n, vec);
                hold[i][k] = kk;
                acc[i] += kk.x * vv.x;
                acc[i] += kk.y * vv.y;
                acc[i] += kk.z * vv.z;
                acc[i] += kk.w * vv.w;
            }
        }
    } else {
        for (int col = threadIdx.x * 4; col < n; col += SK_SPAN) {
            const float4 vv = *(const float4 *)(vrow + col);
#pragma unroll
            for (int i = 0; i < SK_ROWS; ++i) {
                float4 kk = {0.f, 0.f, 0.f, 0.f};
                if (i < rows) kk = sk_load(krow + (size_t)i * n, col, n, vec);
                acc[i] += kk.x * vv.x;
                acc[i] += kk.y * vv.y;
                acc[i] += kk.z * vv.z;
                acc[i] += kk.w * vv.w;
            }
        }
    }
    sk_row_sums(acc, lds);
    float un[SK_ROWS];
#pragma unroll
    for (int i = 0; i < SK_ROWS; ++i) un[i] = i < rows ? r[(size_t)b * m + row0 + i] / acc[i] : 0.f;
    if (threadIdx.x < SK_ROWS) {
        float mine = 0.f;
#pragma unroll
        for (int i = 0; i < SK_ROWS; ++i)
            if (i == (int)threadIdx.x) mine = un[i];
        if ((int)threadIdx.x < rows) {
            float *up = u + (size_t)b * m + row0 + threadIdx.x;
            if (sk_moved(mine, *up, tol)) atomicOr(moved + 1, 1);
            *up = mine;
        }
    }
    float *prow = part + ((size_t)b * gridDim.x + strip) * n4;
    if (NC > 0) {
#pragma unroll
        for (int k = 0; k < NH; ++k) {
            const int col = k * SK_SPAN + threadIdx.x * 4;
            if (col < n4) {
                float4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < SK_ROWS; ++i) {
                    s.x += hold[i][k].x * un[i];
                    s.y += hold[i][k].y * un[i];
                    s.z += hold[i][k].z * un[i];
                    s.w += hold[i][k].w * un[i];
                }
                *(float4 *)(prow + col) = s;
            }
        }
    } else {
        for (int col = threadIdx.x * 4; col < n4; col += SK_SPAN) {
            float4 s = {0.f, 0.f, 0.f, 0.f};
            if (col < n) {
#pragma unroll
                for (int i = 0; i < SK_ROWS; ++i) {
                    float4 kk = {0.f, 0.f, 0.f, 0.f};
                    if (i < rows) kk = sk_load(krow + (size_t)i * n, col, n, vec);
                    s.x += kk.x * un[i];
                    s.y += kk.y * un[i];
                    s.z += kk.z * un[i];
                    s.w += kk.w * un[i];
                }
            }
            *(float4 *)(prow + col) = s;
        }
    }
}

// P = (u K) v in place; iterations = the number of raised flags among moved[0 .. max_iterations).  grid (strips, batch)
__global__ __launch_bounds__(SK_THREADS) void sinkhorn_scale(float *__restrict__ P, const float *__restrict__ u, const float *__restrict__ v,
                                                             const int *__restrict__ moved, int max_iterations, int *__restrict__ iterations,
                                                             int m, int n, int n4, int vec)
{
    const int b = blockIdx.y, row0 = blockIdx.x * SK_ROWS;
    const int rows = min(SK_ROWS, m - row0);
    if (blockIdx.x == 0 && b == 0 && threadIdx.x == 0 && iterations) {
        int t = 0;
        while (t < max_iterations && moved[t] != 0) ++t;
        *iterations = t;
    }
    float *prow = P + ((size_t)b * m + row0) * n;
    float uv[SK_ROWS];
#pragma unroll
    for (int i = 0; i < SK_ROWS; ++i) uv[i] = i < rows ? u[(size_t)b * m + row0 + i] : 0.f;
    for (int col = threadIdx.x * 4; col < n; col += SK_SPAN) {
        const float4 vv = *(const float4 *)(v + (size_t)b * n4 + col);
#pragma unroll
        for (int i = 0; i < SK_ROWS; ++i) {
            if (i < rows) {
                float4 k = sk_load(prow + (size_t)i * n, col, n, vec);
                k.x = (uv[i] * k.x) * vv.x;
                k.y = (uv[i] * k.y) * vv.y;
                k.z = (uv[i] * k.z) * vv.z;
                k.w = (uv[i] * k.w) * vv.w;
                sk_store(prow + (size_t)i * n, col, n, vec, k);
            }
        }
    }
}

void sk_launch_sweep(hipStream_t stream, dim3 grid, int passes, const float *K, const float *r, const float *v, float *u, float *part,
                     int *moved, int m, int n, int n4, int vec, float tol)
{
#define SK_SWEEP(NC) hipLaunchKernelGGL((sinkhorn_sweep<NC>), grid, dim3(SK_THREADS), 0, stream, K, r, v, u, part, moved, m, n, n4, vec, tol)
    switch (passes) {
    case 1: SK_SWEEP(1); break;
    case 2: SK_SWEEP(2); break;
    case 3: SK_SWEEP(3); break;
    case 4: SK_SWEEP(4); break;
    default: SK_SWEEP(0); break;
    }
#undef SK_SWEEP
}

}  // namespace

extern "C" {

size_t dcd_sinkhorn_workspace_bytes(int batch, int m, int n)
{
    if (batch < 1 || m < 1 || n < 1) return 0;
    return sk_layout(batch, m, n).total;
}

int dcd_sinkhorn(void *stream_, const float *M, const float *r, const float *c, float *P, int batch, int m, int n, float lambda,
                 float max_distance, float tolerance, int max_iterations, int *iterations, void *workspace, size_t workspace_bytes)
{
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (!M || !r || !c || !P || !workspace || M == P) return DCD_ERR_BAD_ARG;
    if (batch < 1 || batch > 65535 || m < 1 || n < 1 || max_iterations < 0 || max_iterations > SK_MAX_ITERATIONS) return DCD_ERR_BAD_ARG;
    if ((int64_t)m * n >= ((int64_t)1 << 31) || n > (1 << 30)) return DCD_ERR_BAD_ARG;
    if ((((uintptr_t)M | (uintptr_t)P | (uintptr_t)r | (uintptr_t)c | (uintptr_t)iterations) & 3) != 0) return DCD_ERR_BAD_ARG;
    if (((uintptr_t)workspace & 15) != 0) return DCD_ERR_BAD_ARG;
    const SkLayout l = sk_layout(batch, m, n);
    if (workspace_bytes < l.total) return DCD_ERR_WORKSPACE;
    char *ws = (char *)workspace;
    float *u = (float *)(ws + l.u), *v = (float *)(ws + l.v), *part = (float *)(ws + l.part);
    int *moved = (int *)(ws + l.moved);
    const int vec = n % 4 == 0 && (((uintptr_t)M | (uintptr_t)P) & 15) == 0;
    const int passes = n <= SK_HOLD * SK_SPAN ? (n + SK_SPAN - 1) / SK_SPAN : 0;
    const dim3 strips((unsigned)l.strips, (unsigned)batch), block(SK_THREADS);
    const dim3 columns((unsigned)((l.n4 + SK_THREADS - 1) / SK_THREADS), (unsigned)batch);

    if (!dcd_zero_fill(stream, (float *)moved, (size_t)max_iterations + 1)) return DCD_ERR_LAUNCH;     // an all-zero int is 0.f
    hipLaunchKernelGGL(sinkhorn_gibbs, strips, block, 0, stream, M, r, P, u, part, moved, m, n, l.n4, vec, lambda, max_distance, tolerance);
    hipLaunchKernelGGL(sinkhorn_columns, columns, block, 0, stream, part, c, v, (const int *)nullptr, l.strips, n, l.n4);
    for (int t = 0; t < max_iterations; ++t) {
        sk_launch_sweep(stream, strips, passes, P, r, v, u, part, moved + t, m, n, l.n4, vec, tolerance);
        hipLaunchKernelGGL(sinkhorn_columns, columns, block, 0, stream, part, c, v, (const int *)(moved + t), l.strips, n, l.n4);
    }
    hipLaunchKernelGGL(sinkhorn_scale, strips, block, 0, stream, P, u, v, moved, max_iterations, iterations, m, n, l.n4, vec);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}

}  // extern "C"
