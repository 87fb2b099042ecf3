// dcase_host.h — the host half of dcase.hip: argument checks and the segment table.  Plain C++ with no HIP in it, so a stand-alone program
// can call it on the CPU.
#pragma once
#include <cstdint>
#include <vector>

#define SELD_DCASE_STATE 11
#define SELD_DCASE_MAX_BLOCK 32

namespace dcase_host {

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
