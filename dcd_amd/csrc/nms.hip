// nms.hip -- greedy box NMS among the decoded candidates of every image of a batch, in one launch (include/dcd_hip.h,
// dcd_nms_detections).  The arithmetic and the rules are csrc/nms_math.h.
//
// One workgroup of NMS_THREADS threads (eight waves) per image, K <= 128 candidates:
//   1. the image's rows go to LDS; the prefix n of candidates is counted from the raw scores (one ballot per wave);
//   2. thread t < n counts the candidates visited before its own (O(n^2), scores read from LDS as broadcasts): order[rank] = t;
//   3. the upper triangle of the n x n suppression matrix, in visit order: a wave takes row r (the kept box, wave-uniform) and
//      its lanes the columns c > r, 64 at a time; one ballot is 64 bits of the row, stored by lane 0 -- no atomics, and a chunk
//      that lies on or under the diagonal is skipped by the whole wave;
//   4. the greedy scan over the bit rows, by every thread alike (uniform LDS reads, at most 128 steps of four words);
//   5. the stable compaction: survivors, then the suppressed, then the rows under the threshold, from two ballots and the
//      counts of the lanes below;
//   6. the copy, one row per wave pass.
// LDS as compiled for gfx950: 27 168 bytes per workgroup -- 7 KB of rows, 2 KB of bits, 1.5 KB of indices declared here, and
// 16 KB that the compiler takes for the clip's polygon arrays (32 bytes per thread; the `m < 8` guards of clipped_area keep
// every index into them in range); 80 VGPRs and 48 bytes of scratch per lane.  Nothing is read back, nothing depends on the order waves run in: two
// calls give the same bits.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/dcd_hip.h"
#include "nms_math.h"

namespace {

constexpr int WAVE = 64;
constexpr int NMS_THREADS = 512;
constexpr int NMS_WAVES = NMS_THREADS / WAVE;
static_assert(NMS_MAXK == 2 * WAVE, "two ballots span an image's candidates");
static_assert(NMS_MAXK * NMS_WORDS == NMS_THREADS, "one thread per word clears the bit matrix");

__global__ __launch_bounds__(NMS_THREADS) void nms_detections(const float *__restrict__ rows, const float *__restrict__ aux,
                                                              const float *__restrict__ kpts2d, const float *__restrict__ kpts3d,
                                                              int K, int nk, int mode, double thresh, double det_threshold,
                                                              int class_agnostic, float *__restrict__ rows_out,
                                                              float *__restrict__ aux_out, float *__restrict__ kpts2d_out,
                                                              float *__restrict__ kpts3d_out, float *__restrict__ overlaps_out)
{
    __shared__ float s_row[NMS_MAXK * NMS_ROW];
    __shared__ uint32_t s_bits[NMS_MAXK * NMS_WORDS];
    __shared__ int s_order[NMS_MAXK], s_dst[NMS_MAXK], s_suppressed[NMS_MAXK];
    __shared__ int s_first[2], s_count[2][2];

    const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const size_t row0 = (size_t)blockIdx.x * K;                          // the image's first row

    // 1. rows to LDS, the bit matrix cleared, the prefix counted
    for (int i = tid; i < K * NMS_ROW; i += NMS_THREADS) s_row[i] = rows[row0 * NMS_ROW + i];
    s_bits[tid] = 0;
    if (wave < 2) {
        const bool ok = tid < K && nms_is_candidate(aux[(row0 + tid) * NMS_AUX], det_threshold);
        const unsigned long long below = __ballot(!ok);
        if (lane == 0) s_first[wave] = below ? __ffsll((long long)below) - 1 : WAVE;
    }
    __syncthreads();
    const int n = s_first[0] < WAVE ? s_first[0] : WAVE + s_first[1];    // (a lane at or past K counts as below: n <= K)

    // 2. the visit order
    int my_rank = 0;
    if (tid < n) {
        const float st = s_row[tid * NMS_ROW + 13];
        for (int j = 0; j < n; ++j) my_rank += nms_before(s_row[j * NMS_ROW + 13], j, st, tid) ? 1 : 0;
        s_order[my_rank] = tid;
    }
    __syncthreads();

    // 3. the suppression bits of the upper triangle, and the overlaps for whoever asked
    float *ovl = overlaps_out ? overlaps_out + (size_t)blockIdx.x * K * K : nullptr;
    if (ovl) {
        for (int i = tid; i < K * K; i += NMS_THREADS) {
            const int a = i / K, b = i % K;
            if (a >= n || b >= n || a == b) ovl[i] = 0.f;               // (every other element is one side of a pair below)
        }
    }
    for (int r = wave; r + 1 < n; r += NMS_WAVES) {
        const int iq = s_order[r];
        const float *q = s_row + iq * NMS_ROW;
        for (int chunk = r / WAVE; chunk * WAVE < n; ++chunk) {         // (chunk 0 of a row r >= 63 holds no column > r)
            const int c = chunk * WAVE + lane;
            bool hit = false;
            if (c > r && c < n) {
                const int ib = s_order[c];
                const float *b = s_row + ib * NMS_ROW;
                if (ovl || class_agnostic || nms_same_class(q, b)) {
                    const double o = nms_overlap(mode, q, b);
                    hit = nms_suppresses(o, thresh, class_agnostic != 0, q, b);
                    if (ovl) {
                        ovl[iq * K + ib] = (float)o;
                        ovl[ib * K + iq] = (float)o;
                    }
                }
            }
            const unsigned long long m = __ballot(hit);
            if (lane == 0) {
                s_bits[r * NMS_WORDS + 2 * chunk] = (uint32_t)m;
                s_bits[r * NMS_WORDS + 2 * chunk + 1] = (uint32_t)(m >> 32);
            }
        }
    }
    __syncthreads();

    // 4. the greedy scan
    uint32_t removed[NMS_WORDS];
    nms_greedy(s_bits, n, removed);

    // 5. where every row goes
    bool survives = false, suppressed = false;
    int before_s = 0, before_p = 0;
    if (wave < 2) {
        suppressed = tid < n && nms_bit(removed, my_rank);
        survives = tid < n && !suppressed;
        const unsigned long long ms = __ballot(survives), mp = __ballot(suppressed), lower = (1ull << lane) - 1;
        before_s = __popcll(ms & lower);
        before_p = __popcll(mp & lower);
        if (lane == 0) {
            s_count[wave][0] = __popcll(ms);
            s_count[wave][1] = __popcll(mp);
        }
    }
    __syncthreads();
    if (tid < K) {
        const int n_keep = s_count[0][0] + s_count[1][0];
        const int off_s = wave ? s_count[0][0] : 0, off_p = wave ? s_count[0][1] : 0;
        s_dst[tid] = survives ? off_s + before_s : suppressed ? n_keep + off_p + before_p : tid;
        s_suppressed[tid] = suppressed ? 1 : 0;
    }
    __syncthreads();

    // 6. the copy: row t of the block to row dst[t] (a permutation of 0 .. K - 1)
    const int n2 = 2 * nk, n3 = 3 * nk;
    for (int t = wave; t < K; t += NMS_WAVES) {
        const size_t src = row0 + t, dst = row0 + s_dst[t];
        if (lane < NMS_ROW) rows_out[dst * NMS_ROW + lane] = s_row[t * NMS_ROW + lane];
        if (lane < NMS_AUX) {
            const float v = aux[src * NMS_AUX + lane];
            aux_out[dst * NMS_AUX + lane] = (lane == 0 && s_suppressed[t]) ? -INFINITY : v;
        }
        if (kpts2d_out) {
            for (int i = lane; i < n2; i += WAVE) kpts2d_out[dst * n2 + i] = kpts2d[src * n2 + i];
            for (int i = lane; i < n3; i += WAVE) kpts3d_out[dst * n3 + i] = kpts3d[src * n3 + i];
        }
    }
}

}  // namespace

extern "C" int dcd_nms_detections(void *stream_, const float *rows, const float *aux, const float *kpts2d, const float *kpts3d, int B,
                                  int K, int nk, int mode, double thresh, double det_threshold, int class_agnostic, float *rows_out,
                                  float *aux_out, float *kpts2d_out, float *kpts3d_out, float *overlaps_out)
{
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (!rows || !aux || !rows_out || !aux_out || rows_out == rows || aux_out == aux) return DCD_ERR_BAD_ARG;
    if (B < 1 || K < 1 || K > NMS_MAXK || (int64_t)B * K > INT_MAX) return DCD_ERR_BAD_ARG;
    if (mode != DCD_NMS_2D && mode != DCD_NMS_BEV && mode != DCD_NMS_3D) return DCD_ERR_BAD_ARG;
    if (!(thresh >= 0.0 && thresh < 1.0) || det_threshold != det_threshold) return DCD_ERR_BAD_ARG;
    const bool kpts = kpts2d || kpts3d || kpts2d_out || kpts3d_out;
    if (kpts && (!kpts2d || !kpts3d || !kpts2d_out || !kpts3d_out || kpts2d_out == kpts2d || kpts3d_out == kpts3d || nk < 1 || nk > 128))
        return DCD_ERR_BAD_ARG;
    hipLaunchKernelGGL(nms_detections, dim3((unsigned)B), dim3(NMS_THREADS), 0, stream, rows, aux, kpts2d, kpts3d, K, kpts ? nk : 0,
                       mode, thresh, det_threshold, class_agnostic, rows_out, aux_out, kpts2d_out, kpts3d_out, overlaps_out);
    return hipGetLastError() == hipSuccess ? DCD_OK : DCD_ERR_LAUNCH;
}
