// tta.hip -- the merge of a frame's detections with those of its mirrored view, for every image of a batch in one launch
// (include/dcd_hip.h, dcd_tta_merge_detections).  The arithmetic and the rules are csrc/tta_math.h and csrc/nms_math.h.
//
// One workgroup of TTA_THREADS threads (eight waves) per image, K <= 128 candidates per view:
//   1. view A's rows and view M's rows, un-mirrored on the way in, go to LDS with their aux rows; the prefix n of A's candidates
//      is counted from the raw scores (one ballot per wave);
//   2. thread t < n counts the candidates visited before its own (O(n^2), scores read from LDS as broadcasts): order[rank] = t;
//   3. the n x K match table -- the overlap of A candidate a with M row m where the two may match, else TTA_NO_MATCH -- one
//      element per thread and pass, in LDS (64 KB at K = 128: dynamic LDS, raised past the default limit by lds_limit.h);
//   4. the greedy scan by wave 0 alone: the A candidate is wave-uniform, a lane holds M rows lane and lane + 64 and whether
//      they are taken, and six xor-shuffles give every lane the same arg-max (the larger overlap, a tie to the lower M rank);
//   5. thread t fuses row t with its mate, or scales its scores, in place in LDS;
//   6. the stable rank of the output raw scores (O(K^2)), and the copy, one row per wave pass.
// No atomics, nothing is read back, nothing depends on the order waves run in: two calls give the same bits.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/dcd_hip.h"
#include "lds_limit.h"
#include "tta_math.h"

namespace {

constexpr int WAVE = 64;
constexpr int TTA_THREADS = 512;
constexpr int TTA_WAVES = TTA_THREADS / WAVE;
static_assert(TTA_MAXK == 2 * WAVE, "two ballots span a view's candidates, a lane of the scan holds two M rows");

// dynamic LDS, in floats: A's rows, M's rows, the match table
__host__ __device__ constexpr int tta_lds_floats(int K) { return 2 * K * NMS_ROW + K * K; }

__global__ __launch_bounds__(TTA_THREADS) void tta_merge(const float *__restrict__ rows, const float *__restrict__ aux,
                                                         const float *__restrict__ kpts2d, const float *__restrict__ kpts3d,
                                                         const int *__restrict__ widths, int B, int K, int nk, int mode,
                                                         double match_thresh, double det_threshold, float unmatched_scale,
                                                         float *__restrict__ rows_out, float *__restrict__ aux_out,
                                                         float *__restrict__ kpts2d_out, float *__restrict__ kpts3d_out,
                                                         int *__restrict__ src_out, int *__restrict__ mate_out,
                                                         float *__restrict__ overlaps_out)
{
    extern __shared__ float s_dyn[];
    float *s_a = s_dyn, *s_m = s_dyn + K * NMS_ROW, *s_match = s_dyn + 2 * K * NMS_ROW;
    __shared__ float s_aux_a[TTA_MAXK * NMS_AUX], s_aux_m[TTA_MAXK * NMS_AUX];
    __shared__ int s_order[TTA_MAXK], s_mate[TTA_MAXK], s_dst[TTA_MAXK];
    __shared__ int s_first[2];

    const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const size_t row_a = (size_t)blockIdx.x * K, row_m = ((size_t)B + blockIdx.x) * K;   // the image's first row in each view

    // 1. both views to LDS, M un-mirrored; the prefix of A counted
    for (int i = tid; i < K * NMS_ROW; i += TTA_THREADS) s_a[i] = rows[row_a * NMS_ROW + i];
    for (int i = tid; i < K * NMS_AUX; i += TTA_THREADS) {
        s_aux_a[i] = aux[row_a * NMS_AUX + i];
        s_aux_m[i] = aux[row_m * NMS_AUX + i];
    }
    if (tid < K) {
        float m[NMS_ROW], u[NMS_ROW];
        for (int i = 0; i < NMS_ROW; ++i) m[i] = rows[(row_m + tid) * NMS_ROW + i];
        tta_unmirror(m, widths[blockIdx.x], u);
        for (int i = 0; i < NMS_ROW; ++i) s_m[tid * NMS_ROW + i] = u[i];
        s_mate[tid] = -1;
    }
    if (wave < 2) {
        const bool ok = tid < K && nms_is_candidate(aux[(row_a + tid) * NMS_AUX], det_threshold);
        const unsigned long long below = __ballot(!ok);
        if (lane == 0) s_first[wave] = below ? __ffsll((long long)below) - 1 : WAVE;
    }
    __syncthreads();
    const int n = s_first[0] < WAVE ? s_first[0] : WAVE + s_first[1];    // (a lane at or past K counts as below: n <= K)

    // 2. the visit order of A's candidates
    if (tid < n) {
        const float st = s_a[tid * NMS_ROW + 13];
        int my_rank = 0;
        for (int j = 0; j < n; ++j) my_rank += nms_before(s_a[j * NMS_ROW + 13], j, st, tid) ? 1 : 0;
        s_order[my_rank] = tid;
    }

    // 3. the match table, and the overlaps for whoever asked
    float *ovl = overlaps_out ? overlaps_out + (size_t)blockIdx.x * K * K : nullptr;
    if (ovl)
        for (int i = n * K + tid; i < K * K; i += TTA_THREADS) ovl[i] = 0.f;
    for (int i = tid; i < n * K; i += TTA_THREADS) {
        const int ia = i / K, im = i % K;
        const float *a = s_a + ia * NMS_ROW, *m = s_m + im * NMS_ROW;
        const bool eligible = tta_eligible(s_aux_m[im * NMS_AUX]);
        float value = TTA_NO_MATCH, shown = 0.f;
        if (eligible && (ovl || nms_same_class(a, m))) {
            const double o = nms_overlap(mode, a, m);
            value = tta_match_value(o, match_thresh, eligible, a, m);
            shown = (float)o;
        }
        s_match[i] = value;
        if (ovl) ovl[i] = shown;
    }
    __syncthreads();

    // 4. the greedy scan
    if (wave == 0) {
        bool taken0 = false, taken1 = false;
        for (int r = 0; r < n; ++r) {
            const int ia = s_order[r];
            const float v0 = (lane < K && !taken0) ? s_match[ia * K + lane] : TTA_NO_MATCH;
            const float v1 = (lane + WAVE < K && !taken1) ? s_match[ia * K + lane + WAVE] : TTA_NO_MATCH;
            float best = v0;
            int at = lane;
            if (tta_better(v1, lane + WAVE, best, at)) { best = v1; at = lane + WAVE; }
            for (int step = 1; step < WAVE; step *= 2) {
                const float other = __shfl_xor(best, step, WAVE);
                const int other_at = __shfl_xor(at, step, WAVE);
                if (tta_better(other, other_at, best, at)) { best = other; at = other_at; }
            }
            if (best > TTA_NO_MATCH) {
                if (at == lane) taken0 = true;
                if (at == lane + WAVE) taken1 = true;
                if (lane == 0) s_mate[ia] = at;
            }
        }
    }
    __syncthreads();

    // 5. the output row of every A row, in place
    if (tid < n) {
        float *a = s_a + tid * NMS_ROW, *xa = s_aux_a + tid * NMS_AUX;
        const int mate = s_mate[tid];
        if (mate >= 0) {
            float row[NMS_ROW], x[NMS_AUX];
            tta_fuse(a, xa, s_m + mate * NMS_ROW, s_aux_m + mate * NMS_AUX, row, x);
            for (int i = 0; i < NMS_ROW; ++i) a[i] = row[i];
            for (int i = 0; i < NMS_AUX; ++i) xa[i] = x[i];
        } else {
            a[13] *= unmatched_scale;
            xa[0] *= unmatched_scale;
        }
    }
    __syncthreads();

    // 6. the stable order of the output raw scores, and the copy: row t of view A's block to row dst[t]
    if (tid < K) {
        const float st = s_aux_a[tid * NMS_AUX];
        int my_rank = 0;
        for (int j = 0; j < K; ++j) my_rank += nms_before(s_aux_a[j * NMS_AUX], j, st, tid) ? 1 : 0;
        s_dst[tid] = my_rank;
    }
    __syncthreads();
    const int n2 = 2 * nk, n3 = 3 * nk;
    for (int t = wave; t < K; t += TTA_WAVES) {
        const size_t src = row_a + t, dst = row_a + s_dst[t];
        if (lane < NMS_ROW) rows_out[dst * NMS_ROW + lane] = s_a[t * NMS_ROW + lane];
        if (lane < NMS_AUX) aux_out[dst * NMS_AUX + lane] = s_aux_a[t * NMS_AUX + lane];
        if (lane == 0) {
            src_out[dst] = t;
            mate_out[dst] = s_mate[t];
        }
        if (kpts2d_out) {
            for (int i = lane; i < n2; i += WAVE) kpts2d_out[dst * n2 + i] = kpts2d[src * n2 + i];
            for (int i = lane; i < n3; i += WAVE) kpts3d_out[dst * n3 + i] = kpts3d[src * n3 + i];
        }
    }
}

LdsLimit g_tta_lds;

}  // namespace

extern "C" int dcd_tta_merge_detections(void *stream_, const float *rows, const float *aux, const float *kpts2d, const float *kpts3d,
                                        const int *widths, int B, int K, int nk, int mode, double match_thresh, double det_threshold,
                                        double unmatched_scale, float *rows_out, float *aux_out, float *kpts2d_out, float *kpts3d_out,
                                        int *src_out, int *mate_out, float *overlaps_out)
{
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (!rows || !aux || !widths || !rows_out || !aux_out || !src_out || !mate_out || rows_out == rows || aux_out == aux)
        return DCD_ERR_BAD_ARG;
    if (B < 1 || K < 1 || K > TTA_MAXK || 2 * (int64_t)B * K > INT_MAX) return DCD_ERR_BAD_ARG;
    if (mode != DCD_NMS_2D && mode != DCD_NMS_BEV && mode != DCD_NMS_3D) return DCD_ERR_BAD_ARG;
    if (!(match_thresh >= 0.0 && match_thresh < 1.0) || det_threshold != det_threshold) return DCD_ERR_BAD_ARG;
    if (!(unmatched_scale >= 0.0 && unmatched_scale <= 1.0)) return DCD_ERR_BAD_ARG;
    const bool kpts = kpts2d || kpts3d || kpts2d_out || kpts3d_out;
    if (kpts && (!kpts2d || !kpts3d || !kpts2d_out || !kpts3d_out || kpts2d_out == kpts2d || kpts3d_out == kpts3d || nk < 1 || nk > 128))
        return DCD_ERR_BAD_ARG;
    const int lds = tta_lds_floats(K) * (int)sizeof(float);
    if (!g_tta_lds.raise(tta_lds_floats(TTA_MAXK) * (int)sizeof(float), tta_merge)) return DCD_ERR_LAUNCH;
    hipLaunchKernelGGL(tta_merge, dim3((unsigned)B), dim3(TTA_THREADS), lds, stream, rows, aux, kpts2d, kpts3d, widths, B, K,
                       kpts ? nk : 0, mode, match_thresh, det_threshold, (float)unmatched_scale, rows_out, aux_out, kpts2d_out,
                       kpts3d_out, src_out, mate_out, overlaps_out);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}
