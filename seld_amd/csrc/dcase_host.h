// dcase_host.h — the host half of dcase.hip: argument checks and the segment table.  Plain C++ with no HIP in it, so a stand-alone program
// can call it on the CPU.
#pragma once
#include <cstdint>
#include <vector>

#define SELD_DCASE_STATE 11
#define SELD_DCASE_MAX_BLOCK 32
#define SELD_DCASE_SWEEP_SLOTS 8          // SELD_DCASE_MAX_SLOTS: track averages kept per (segment, class, threshold)

namespace dcase_host {

// seld_dcase_sweep's own arguments: 1..max_cand candidates (SELD_DCASE_MAX_CAND), a candidate list and a table to write
inline bool sweep_args_ok(int n_cand, int max_cand, const void* cand, const void* table) {
    return n_cand >= 1 && n_cand <= max_cand && cand != nullptr && table != nullptr;
}

// bytes of the sweep's per-(segment, class, threshold) records for `segs` segments: one packed counter word and the track averages
inline int64_t sweep_record_bytes(int64_t segs, int n_classes, int n_cand) {
    return segs * n_classes * (int64_t)(n_cand + 1) * (1 + SELD_DCASE_SWEEP_SLOTS) * 8;
}

// file_off[0] == 0 and strictly ascending (every file has a frame); -> N = file_off[n_files], or -1
inline int64_t total_frames(const int32_t* file_off, int n_files) {
    if (!file_off || n_files < 1 || file_off[0] != 0) return -1;
    for (int f = 0; f < n_files; ++f)
        if (file_off[f + 1] <= file_off[f]) return -1;
    return file_off[n_files];
}

// at most this many segments whatever the offsets are: every file ends on at most one ragged segment
inline int64_t max_segments(int64_t N, int n_files, int block_size) { return N / block_size + n_files; }

// (first frame, frame count) of every segment, file by file: a segment never spans two files, a file's last one may be ragged
inline void build_segments(const int32_t* file_off, int n_files, int block_size, std::vector<int32_t>& table) {
    table.clear();
    for (int f = 0; f < n_files; ++f)
        for (int32_t t = file_off[f]; t < file_off[f + 1]; t += block_size) {
            table.push_back(t);
            table.push_back(file_off[f + 1] - t < block_size ? file_off[f + 1] - t : block_size);
        }
}

}  // namespace dcase_host
