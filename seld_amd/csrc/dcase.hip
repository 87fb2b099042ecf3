// dcase.hip — the segment-based, location-aware DCASE score and the answer rows, on the device.
//
//   seld_dcase_update   SELDMetrics_.update_seld_scores (SELD_evaluation_metrics.py:63-154) with the distance of
//                       distance_between_cartesian_coordinates (:171-188), on model-format predictions (one DOA per class and frame) and
//                       packed ground truth.  The reference walks nested dicts read back from a csv file, one file at a time on the host.
//   seld_dcase_sweep    the counters seld_dcase_update would leave for base_thresh with one class's entry replaced by one candidate, for
//                       every (class, candidate) at once and bit for bit: the inner loop of a per-class threshold search
//                       (search_best.py:145, whose loop the reference left commented out).
//   seld_answer_rows    the tf.where + gather of utils.write_answer (utils.py:249-264): an ordered stream compaction.
//
// state layout (doubles): [0]TP [1]FP [2]FN [3]S [4]D [5]I [6]Nref [7]total_DE [8]DE_TP [9]DE_FP [10]DE_FN
//
// All three are staged and free of atomics: the same inputs give the same bits.  The host half (argument checks, segment table) is
// dcase_host.h.  The tables reach the device through one copy per call, which the call waits for before it returns.
#include "common.h"
#include "dcase_host.h"
#include "../../include/seld_hip.h"

namespace {

#define DC_TP 0
#define DC_FP 1
#define DC_FN 2
#define DC_S 3
#define DC_D 4
#define DC_I 5
#define DC_NREF 6
#define DC_TOTAL_DE 7
#define DC_DE_TP 8
#define DC_DE_FP 9
#define DC_DE_FN 10

// distance_between_cartesian_coordinates (:171-188) in fp64, operation by operation
__device__ inline double dcase_angle(double x1, double y1, double z1, double x2, double y2, double z2) {
    const double n1 = sqrt(x1 * x1 + y1 * y1 + z1 * z1 + 1e-10);
    const double n2 = sqrt(x2 * x2 + y2 * y2 + z2 * z2 + 1e-10);
    x1 /= n1; y1 /= n1; z1 /= n1;
    x2 /= n2; y2 /= n2; z2 /= n2;
    double d = x1 * x2 + y1 * y2 + z1 * z2;
    d = fmin(fmax(d, -1.0), 1.0);
    return acos(d) * 180.0 / 3.14159265358979323846;
}

// one thread per segment: all classes, all frames of the segment -> items[segment][11]
__global__ __launch_bounds__(64) void seld_dcase_items_kernel(const float* __restrict__ sed, const float* __restrict__ doa,
                                                              const float* __restrict__ thr, const double* __restrict__ gt_xyz,
                                                              const uint8_t* __restrict__ gt_slot, const int32_t* __restrict__ gt_n,
                                                              const int32_t* __restrict__ seg, int n_seg, int nc, int K, double doa_threshold,
                                                              double* __restrict__ items) {
    const int it = blockIdx.x * 64 + threadIdx.x;
    if (it >= n_seg) return;
    const int t0 = seg[2 * it], len = seg[2 * it + 1];
    double acc[SELD_DCASE_STATE];
#pragma unroll
    for (int i = 0; i < SELD_DCASE_STATE; ++i) acc[i] = 0.0;
    int loc_fp = 0, loc_fn = 0;
    for (int c = 0; c < nc; ++c) {
        const float th = thr[c];
        int nref = 0;
        bool gt_any = false, pred_any = false;
        for (int f = 0; f < len; ++f) {
            const size_t r = (size_t)(t0 + f) * nc + c;
            const int n = min(max(gt_n[r], 0), K);
            nref = max(nref, n);
            gt_any |= n > 0;
            pred_any |= sed[r] > th;
        }
        acc[DC_NREF] += nref;
        if (gt_any && pred_any) {
            double sum[SELD_DCASE_MAX_SLOTS];
            int cnt[SELD_DCASE_MAX_SLOTS];
#pragma unroll
            for (int s = 0; s < SELD_DCASE_MAX_SLOTS; ++s) { sum[s] = 0.0; cnt[s] = 0; }
            int common = 0;
            for (int f = 0; f < len; ++f) {
                const size_t t = (size_t)(t0 + f), r = t * nc + c;
                const int n = min(max(gt_n[r], 0), K);
                if (n == 0 || !(sed[r] > th)) continue;
                ++common;
                const float* dp = doa + t * 3 * nc + c;
                const double px = dp[0], py = dp[nc], pz = dp[2 * nc];
                // one prediction: the assignment on an n x 1 cost matrix is the arg-min (the first one on a tie)
                double best = 0.0;
                int best_slot = 0;
                for (int e = 0; e < n; ++e) {
                    const double* g = gt_xyz + (r * K + e) * 3;
                    const double d = dcase_angle(g[0], g[1], g[2], px, py, pz);
                    if (e == 0 || d < best) { best = d; best_slot = gt_slot[r * K + e]; }
                }
                best_slot = min(best_slot, SELD_DCASE_MAX_SLOTS - 1);
#pragma unroll
                for (int s = 0; s < SELD_DCASE_MAX_SLOTS; ++s)
                    if (s == best_slot) { sum[s] += best; cnt[s] += 1; }
            }
            if (common == 0) {          // predicted and reference frames never coincide
                loc_fn += 1; acc[DC_FN] += 1.0; acc[DC_DE_FN] += 1.0;
            } else {
#pragma unroll
                for (int s = 0; s < SELD_DCASE_MAX_SLOTS; ++s) {
                    if (cnt[s] == 0) continue;
                    const double avg = sum[s] / (double)cnt[s];
                    acc[DC_TOTAL_DE] += avg;
                    acc[DC_DE_TP] += 1.0;
                    if (avg <= doa_threshold) acc[DC_TP] += 1.0;
                    else { loc_fp += 1; acc[DC_FP] += 1.0; }
                }
            }
        } else if (gt_any) {
            loc_fn += 1; acc[DC_FN] += 1.0; acc[DC_DE_FN] += 1.0;
        } else if (pred_any) {
            loc_fp += 1; acc[DC_FP] += 1.0; acc[DC_DE_FP] += 1.0;
        }
    }
    acc[DC_S] = (double)min(loc_fp, loc_fn);
    acc[DC_D] = (double)max(0, loc_fn - loc_fp);
    acc[DC_I] = (double)max(0, loc_fp - loc_fn);
    double* out = items + (size_t)it * SELD_DCASE_STATE;
#pragma unroll
    for (int i = 0; i < SELD_DCASE_STATE; ++i) out[i] = acc[i];
}

// state[col] += sum_rows items[row][col]   (one block per column, fixed order; seld_metrics_reduce_kernel in doubles)
__global__ __launch_bounds__(256) void seld_dcase_reduce_kernel(const double* __restrict__ items, int rows, double* __restrict__ state) {
    __shared__ double red[256];
    const int col = blockIdx.x;
    double s = 0.0;
    for (int r = threadIdx.x; r < rows; r += 256) s += items[(size_t)r * SELD_DCASE_STATE + col];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) state[col] += red[0];
}

// ---- the threshold sweep: the counters of base_thresh with one class's entry replaced by one candidate, for every (class, candidate)
//
// A record per (threshold index j, class, segment), j < M the candidates and j = M the base entry of that class; segments run fastest, so
// both kernels touch neighbouring addresses from neighbouring lanes.  `packed` holds one byte per count (none exceeds the 8 slots):
//   0 TP  1 FP  2 FN  3 DE_TP  4 DE_FP  5 DE_FN  6 Nref  7 the mask of the slots whose track average was written to `avgs`
// loc_FP and loc_FN of seld_dcase_items_kernel always move with FP and FN, so they are not stored.
#define SW_SLOTS SELD_DCASE_SWEEP_SLOTS
#define SW_NO_SLOT 0xFF

__device__ inline size_t sw_rec(int j, int c, int nc, int n_seg, int sg) { return ((size_t)j * nc + c) * n_seg + sg; }
__device__ inline size_t sw_avg(int j, int c, int s, int nc, int n_seg, int sg) { return (((size_t)j * nc + c) * SW_SLOTS + s) * n_seg + sg; }

// one thread per (class, segment).  One walk over the frames finds each frame's arg-min distance and slot (they do not depend on a
// threshold; frames no threshold of this class activates are skipped); the M + 1 thresholds then re-walk the values kept in LDS, adding
// per slot in frame order as seld_dcase_items_kernel does.
__global__ __launch_bounds__(64) void seld_dcase_sweep_items_kernel(const float* __restrict__ sed, const float* __restrict__ doa,
                                                                    const float* __restrict__ base, const float* __restrict__ cand,
                                                                    const double* __restrict__ gt_xyz, const uint8_t* __restrict__ gt_slot,
                                                                    const int32_t* __restrict__ gt_n, const int32_t* __restrict__ seg, int n_seg,
                                                                    int nc, int K, int M, double doa_threshold,
                                                                    unsigned long long* __restrict__ packed, double* __restrict__ avgs) {
    __shared__ double s_best[SELD_DCASE_MAX_BLOCK][64];      // [frame][thread]: a thread reads only what it wrote
    __shared__ float s_sed[SELD_DCASE_MAX_BLOCK][64];
    __shared__ uint8_t s_slot[SELD_DCASE_MAX_BLOCK][64];
    const int tid = threadIdx.x;
    const long long it = (long long)blockIdx.x * 64 + tid;
    if (it >= (long long)n_seg * nc) return;
    const int c = (int)(it / n_seg), sg = (int)(it - (long long)c * n_seg);
    const int t0 = seg[2 * sg], len = seg[2 * sg + 1];
    float th_min = base[c];
    for (int k = 0; k < M; ++k) th_min = fminf(th_min, cand[k]);
    int nref = 0;
    bool gt_any = false;
    for (int f = 0; f < len; ++f) {
        const size_t t = (size_t)(t0 + f), r = t * nc + c;
        const int n = min(max(gt_n[r], 0), K);
        const float v = sed[r];
        nref = max(nref, n);
        gt_any |= n > 0;
        s_sed[f][tid] = v;
        int best_slot = SW_NO_SLOT;
        if (n > 0 && v > th_min) {
            const float* dp = doa + t * 3 * nc + c;
            const double px = dp[0], py = dp[nc], pz = dp[2 * nc];
            double best = 0.0;
            for (int e = 0; e < n; ++e) {
                const double* g = gt_xyz + (r * K + e) * 3;
                const double d = dcase_angle(g[0], g[1], g[2], px, py, pz);
                if (e == 0 || d < best) { best = d; best_slot = gt_slot[r * K + e]; }
            }
            best_slot = min(best_slot, SW_SLOTS - 1);
            s_best[f][tid] = best;
        }
        s_slot[f][tid] = (uint8_t)best_slot;
    }
    for (int j = 0; j <= M; ++j) {
        const float th = j < M ? cand[j] : base[c];
        double sum[SW_SLOTS];
        int cnt[SW_SLOTS];
#pragma unroll
        for (int s = 0; s < SW_SLOTS; ++s) { sum[s] = 0.0; cnt[s] = 0; }
        bool pred_any = false;
        int common = 0;
        for (int f = 0; f < len; ++f) {
            if (!(s_sed[f][tid] > th)) continue;
            pred_any = true;
            const int slot = s_slot[f][tid];
            if (slot == SW_NO_SLOT) continue;          // no reference entry in this frame
            ++common;
            const double best = s_best[f][tid];
#pragma unroll
            for (int s = 0; s < SW_SLOTS; ++s)
                if (s == slot) { sum[s] += best; cnt[s] += 1; }
        }
        unsigned long long tp = 0, fp = 0, fn = 0, de_tp = 0, de_fp = 0, de_fn = 0, mask = 0;
        if (gt_any && pred_any) {
            if (common == 0) {
                fn = 1; de_fn = 1;
            } else {
#pragma unroll
                for (int s = 0; s < SW_SLOTS; ++s) {
                    if (cnt[s] == 0) continue;
                    const double avg = sum[s] / (double)cnt[s];
                    avgs[sw_avg(j, c, s, nc, n_seg, sg)] = avg;
                    mask |= 1ull << s;
                    de_tp += 1;
                    if (avg <= doa_threshold) tp += 1;
                    else fp += 1;
                }
            }
        } else if (gt_any) {
            fn = 1; de_fn = 1;
        } else if (pred_any) {
            fp = 1; de_fp = 1;
        }
        packed[sw_rec(j, c, nc, n_seg, sg)] = tp | fp << 8 | fn << 16 | de_tp << 24 | de_fp << 32 | de_fn << 40 |
                                             (unsigned long long)nref << 48 | mask << 56;
    }
}

// one block per table row: each segment's counters are put together on load (the candidate's record for the row's class, the base records
// for the others; total_DE adds the track averages classes ascending, slots ascending, from 0.0), then summed over the segments in
// seld_dcase_reduce_kernel's order: strided partial sums, the same tree.  The row is written, where that kernel adds to a state.
__global__ __launch_bounds__(256) void seld_dcase_sweep_reduce_kernel(const unsigned long long* __restrict__ packed,
                                                                      const double* __restrict__ avgs, int n_seg, int nc, int M,
                                                                      double* __restrict__ table) {
    __shared__ double red[SELD_DCASE_STATE][256];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int cc = row < nc * M ? row / M : -1, kk = row < nc * M ? row - cc * M : 0;
    double acc[SELD_DCASE_STATE];
#pragma unroll
    for (int i = 0; i < SELD_DCASE_STATE; ++i) acc[i] = 0.0;
    for (int r = tid; r < n_seg; r += 256) {
        int cnt[7] = {0, 0, 0, 0, 0, 0, 0};
        double de = 0.0;
        for (int c = 0; c < nc; ++c) {
            const int j = c == cc ? kk : M;
            const unsigned long long w = packed[sw_rec(j, c, nc, n_seg, r)];
#pragma unroll
            for (int i = 0; i < 7; ++i) cnt[i] += (int)(w >> (8 * i) & 0xFF);
            const unsigned mask = (unsigned)(w >> 56);
#pragma unroll
            for (int s = 0; s < SW_SLOTS; ++s)
                if (mask >> s & 1u) de += avgs[sw_avg(j, c, s, nc, n_seg, r)];
        }
        const int loc_fp = cnt[1], loc_fn = cnt[2];
        acc[DC_TP] += (double)cnt[0];
        acc[DC_FP] += (double)cnt[1];
        acc[DC_FN] += (double)cnt[2];
        acc[DC_S] += (double)min(loc_fp, loc_fn);
        acc[DC_D] += (double)max(0, loc_fn - loc_fp);
        acc[DC_I] += (double)max(0, loc_fp - loc_fn);
        acc[DC_NREF] += (double)cnt[6];
        acc[DC_TOTAL_DE] += de;
        acc[DC_DE_TP] += (double)cnt[3];
        acc[DC_DE_FP] += (double)cnt[4];
        acc[DC_DE_FN] += (double)cnt[5];
    }
#pragma unroll
    for (int i = 0; i < SELD_DCASE_STATE; ++i) red[i][tid] = acc[i];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int i = 0; i < SELD_DCASE_STATE; ++i) red[i][tid] += red[i][tid + w];
        }
        __syncthreads();
    }
    if (tid < SELD_DCASE_STATE) table[(size_t)row * SELD_DCASE_STATE + tid] = red[tid][0];      // no sum is -0.0: 0.0 + x has x's bits
}

// ---- answer rows: count per 256-element chunk, exclusive scan of the counts, ordered write
#define AR_CHUNK 256

__device__ inline bool ar_active(const float* __restrict__ sed, const float* __restrict__ thr, int i, int total, int nc) {
    return i < total && sed[i] > thr[i % nc];
}

__global__ __launch_bounds__(AR_CHUNK) void seld_answer_count_kernel(const float* __restrict__ sed, const float* __restrict__ thr, int total, int nc,
                                                                     int32_t* __restrict__ chunk_cnt) {
    __shared__ int wcnt[AR_CHUNK / 64];
    const int i = blockIdx.x * AR_CHUNK + threadIdx.x;
    const unsigned long long b = __ballot(ar_active(sed, thr, i, total, nc));
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) chunk_cnt[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// one block: counts -> exclusive offsets in place, tile by tile with a running carry; the total goes to row_off[n_files]
__global__ __launch_bounds__(256) void seld_answer_scan_kernel(int32_t* __restrict__ chunk_cnt, int n_chunks, int32_t* __restrict__ row_total) {
    __shared__ int sh[256];
    int carry = 0;
    for (int base = 0; base < n_chunks; base += 256) {
        const int j = base + threadIdx.x;
        const int v = j < n_chunks ? chunk_cnt[j] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int a = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            sh[threadIdx.x] += a;
            __syncthreads();
        }
        if (j < n_chunks) chunk_cnt[j] = carry + sh[threadIdx.x] - v;
        carry += sh[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) *row_total = carry;
}

__global__ __launch_bounds__(AR_CHUNK) void seld_answer_write_kernel(const float* __restrict__ sed, const float* __restrict__ doa,
                                                                     const float* __restrict__ thr, const int32_t* __restrict__ file_off, int n_files,
                                                                     int total, int nc, const int32_t* __restrict__ chunk_off,
                                                                     int32_t* __restrict__ row_fc, float* __restrict__ row_xyz,
                                                                     int32_t* __restrict__ row_off) {
    __shared__ int wcnt[AR_CHUNK / 64];
    const int i = blockIdx.x * AR_CHUNK + threadIdx.x;
    const bool on = ar_active(sed, thr, i, total, nc);
    const unsigned long long b = __ballot(on);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wcnt[wave] = __popcll(b);
    __syncthreads();
    if (i >= total) return;
    int rank = chunk_off[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += wcnt[w];
    const int t = i / nc, c = i - t * nc;
    int lo = 0, hi = n_files;              // the file of frame t: file_off[lo] <= t < file_off[lo + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (file_off[mid] <= t) lo = mid; else hi = mid;
    }
    if (c == 0 && t == file_off[lo]) row_off[lo] = rank;      // rows written before this file's first element
    if (!on) return;
    row_fc[2 * (size_t)rank] = t - file_off[lo];
    row_fc[2 * (size_t)rank + 1] = c;
    const float* dp = doa + (size_t)t * 3 * nc + c;
    float* o = row_xyz + 3 * (size_t)rank;
    o[0] = dp[0];
    o[1] = dp[nc];
    o[2] = dp[2 * nc];
}

inline int64_t align8(int64_t n) { return (n + 7) & ~(int64_t)7; }

}  // namespace

extern "C" {

int seld_dcase_state_size(void) { return SELD_DCASE_STATE; }

int64_t seld_dcase_update_scratch_bytes(int64_t N, int n_files, int block_size) {
    if (N < 1 || n_files < 1 || block_size < 1 || block_size > SELD_DCASE_MAX_BLOCK) return -1;
    const int64_t ms = dcase_host::max_segments(N, n_files, block_size);
    return ms * SELD_DCASE_STATE * (int64_t)sizeof(double) + align8(ms * 2 * (int64_t)sizeof(int32_t));
}

int seld_dcase_update(const float* sed, const float* doa, const float* sed_thresh, const double* gt_xyz, const uint8_t* gt_slot,
                      const int32_t* gt_n, const int32_t* file_off, int n_files, int n_classes, int K, int block_size, double doa_threshold,
                      double* state, void* scratch, void* stream) {
    if (!sed || !doa || !sed_thresh || !gt_xyz || !gt_slot || !gt_n || !file_off || !state || !scratch) return SELD_ERR_INVALID;
    if (n_files < 1 || n_classes < 1 || K < 1 || K > SELD_DCASE_MAX_SLOTS || block_size < 1 || block_size > SELD_DCASE_MAX_BLOCK)
        return SELD_ERR_INVALID;
    const int64_t N = dcase_host::total_frames(file_off, n_files);
    if (N < 1 || N * n_classes > INT32_MAX) return SELD_ERR_INVALID;
    std::vector<int32_t> table;
    dcase_host::build_segments(file_off, n_files, block_size, table);
    const int n_seg = (int)(table.size() / 2);
    const int64_t ms = dcase_host::max_segments(N, n_files, block_size);
    double* items = (double*)scratch;
    int32_t* seg = (int32_t*)((char*)scratch + ms * SELD_DCASE_STATE * (int64_t)sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    if (hipMemcpyAsync(seg, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess) return SELD_ERR_HIP;
    if (hipStreamSynchronize(st) != hipSuccess) return SELD_ERR_HIP;      // `table` dies with this call
    hipLaunchKernelGGL(seld_dcase_items_kernel, dim3((n_seg + 63) / 64), dim3(64), 0, st, sed, doa, sed_thresh, gt_xyz, gt_slot, gt_n, seg, n_seg,
                       n_classes, K, doa_threshold, items);
    hipLaunchKernelGGL(seld_dcase_reduce_kernel, dim3(SELD_DCASE_STATE), dim3(256), 0, st, items, n_seg, state);
    return hipGetLastError() == hipSuccess ? SELD_OK : SELD_ERR_HIP;
}

int64_t seld_dcase_sweep_scratch_bytes(int64_t N, int n_files, int n_classes, int n_cand, int block_size) {
    if (N < 1 || n_files < 1 || n_classes < 1 || block_size < 1 || block_size > SELD_DCASE_MAX_BLOCK || N * n_classes > INT32_MAX) return -1;
    if (n_cand < 1 || n_cand > SELD_DCASE_MAX_CAND) return -1;
    const int64_t ms = dcase_host::max_segments(N, n_files, block_size);
    return align8(ms * 2 * (int64_t)sizeof(int32_t)) + dcase_host::sweep_record_bytes(ms, n_classes, n_cand);
}

int seld_dcase_sweep(const float* sed, const float* doa, const float* base_thresh, const float* cand, const double* gt_xyz,
                     const uint8_t* gt_slot, const int32_t* gt_n, const int32_t* file_off, int n_files, int n_classes, int K, int n_cand,
                     int block_size, double doa_threshold, double* table, void* scratch, void* stream) {
    if (!sed || !doa || !base_thresh || !gt_xyz || !gt_slot || !gt_n || !file_off || !scratch) return SELD_ERR_INVALID;
    if (!dcase_host::sweep_args_ok(n_cand, SELD_DCASE_MAX_CAND, cand, table)) return SELD_ERR_INVALID;
    if (n_files < 1 || n_classes < 1 || K < 1 || K > SELD_DCASE_MAX_SLOTS || block_size < 1 || block_size > SELD_DCASE_MAX_BLOCK)
        return SELD_ERR_INVALID;
    const int64_t N = dcase_host::total_frames(file_off, n_files);
    if (N < 1 || N * n_classes > INT32_MAX) return SELD_ERR_INVALID;
    std::vector<int32_t> segs;
    dcase_host::build_segments(file_off, n_files, block_size, segs);
    const int n_seg = (int)(segs.size() / 2);
    const int64_t ms = dcase_host::max_segments(N, n_files, block_size);
    int32_t* seg = (int32_t*)scratch;
    unsigned long long* packed = (unsigned long long*)((char*)scratch + align8(ms * 2 * (int64_t)sizeof(int32_t)));
    double* avgs = (double*)(packed + (size_t)n_seg * n_classes * (n_cand + 1));
    hipStream_t st = (hipStream_t)stream;
    if (hipMemcpyAsync(seg, segs.data(), segs.size() * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess) return SELD_ERR_HIP;
    if (hipStreamSynchronize(st) != hipSuccess) return SELD_ERR_HIP;      // `segs` dies with this call
    const int64_t threads = (int64_t)n_seg * n_classes;
    hipLaunchKernelGGL(seld_dcase_sweep_items_kernel, dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, st, sed, doa, base_thresh, cand, gt_xyz,
                       gt_slot, gt_n, seg, n_seg, n_classes, K, n_cand, doa_threshold, packed, avgs);
    hipLaunchKernelGGL(seld_dcase_sweep_reduce_kernel, dim3(n_classes * n_cand + 1), dim3(256), 0, st, packed, avgs, n_seg, n_classes, n_cand,
                       table);
    return hipGetLastError() == hipSuccess ? SELD_OK : SELD_ERR_HIP;
}

int64_t seld_answer_rows_scratch_bytes(int64_t N, int n_files, int n_classes) {
    if (N < 1 || n_files < 1 || n_classes < 1 || N * n_classes > INT32_MAX) return -1;
    const int64_t chunks = (N * n_classes + AR_CHUNK - 1) / AR_CHUNK;
    return align8(((int64_t)n_files + 1 + chunks) * (int64_t)sizeof(int32_t));
}

int seld_answer_rows(const float* sed, const float* doa, const float* sed_thresh, const int32_t* file_off, int n_files, int n_classes,
                     int32_t* row_fc, float* row_xyz, int32_t* row_off, void* scratch, void* stream) {
    if (!sed || !doa || !sed_thresh || !file_off || !row_fc || !row_xyz || !row_off || !scratch) return SELD_ERR_INVALID;
    if (n_files < 1 || n_classes < 1) return SELD_ERR_INVALID;
    const int64_t N = dcase_host::total_frames(file_off, n_files);
    if (N < 1 || N * n_classes > INT32_MAX) return SELD_ERR_INVALID;
    const int total = (int)(N * n_classes);
    const int chunks = (total + AR_CHUNK - 1) / AR_CHUNK;
    int32_t* d_off = (int32_t*)scratch;
    int32_t* chunk_cnt = d_off + n_files + 1;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemcpyAsync(d_off, file_off, ((size_t)n_files + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess) return SELD_ERR_HIP;
    if (hipStreamSynchronize(st) != hipSuccess) return SELD_ERR_HIP;      // the caller's file_off may go once this call returns
    hipLaunchKernelGGL(seld_answer_count_kernel, dim3(chunks), dim3(AR_CHUNK), 0, st, sed, sed_thresh, total, n_classes, chunk_cnt);
    hipLaunchKernelGGL(seld_answer_scan_kernel, dim3(1), dim3(256), 0, st, chunk_cnt, chunks, row_off + n_files);
    hipLaunchKernelGGL(seld_answer_write_kernel, dim3(chunks), dim3(AR_CHUNK), 0, st, sed, doa, sed_thresh, d_off, n_files, total, n_classes,
                       chunk_cnt, row_fc, row_xyz, row_off);
    return hipGetLastError() == hipSuccess ? SELD_OK : SELD_ERR_HIP;
}

}  // extern "C"
