// conv1_pp_sched.h — the tile schedule of the ping-pong first-block forward (conv_pool_sb.hip, conv_first_fwd_pool_sbpp_kernel), in plain C++ so that
// a host program can walk it (tests/test_conv1_pingpong_cpu.py): which tile a wave group works on in which iteration, and how many barriers it takes.
//
// The 4-wave kernel runs vgrid = min(ntiles, 512) persistent workgroups; workgroup v walks tiles v, v + vgrid, ... .  The ping-pong kernel runs
// ceil(vgrid / 2) workgroups of two wave groups; group g of block b IS virtual workgroup v of that grid (same tiles, same order, same partial row).
// Every wave of a block must meet the same number of s_barrier: the trip count depends on (ntiles, vgrid) alone, a group without a tile in an
// iteration (or with no virtual workgroup at all: odd vgrid) skips the work and keeps the barriers.
#pragma once
#if defined(__HIPCC__)
#define C1PP_HD __host__ __device__
#else
#define C1PP_HD
#endif

#define C1PP_MAX_VIRTUAL 512

struct Conv1PpSched {
    int ntiles;      // B * ceil(H / 10)
    int vgrid;       // virtual workgroups = statistics partial rows
    int nblocks;     // launched workgroups: ceil(vgrid / 2)
    int trips;       // loop iterations of EVERY group: ceil(ntiles / vgrid)
};

C1PP_HD inline Conv1PpSched conv1_pp_sched(int B, int H) {
    Conv1PpSched s;
    s.ntiles = B * ((H + 9) / 10);
    s.vgrid = s.ntiles < C1PP_MAX_VIRTUAL ? s.ntiles : C1PP_MAX_VIRTUAL;
    s.nblocks = (s.vgrid + 1) / 2;
    s.trips = (s.ntiles + s.vgrid - 1) / s.vgrid;
    return s;
}
// the two groups of a block walk neighbouring tiles.  May be == vgrid (odd vgrid, last block): never active.
C1PP_HD inline int conv1_pp_virtual(int block, int group) { return 2 * block + group; }
C1PP_HD inline int conv1_pp_tile(const Conv1PpSched& s, int v, int iter) { return v + iter * s.vgrid; }
C1PP_HD inline bool conv1_pp_active(const Conv1PpSched& s, int v, int iter) { return v < s.vgrid && conv1_pp_tile(s, v, iter) < s.ntiles; }
// s_barrier count of a group's main loop: group 1 runs one phase behind group 0, so it takes one barrier before its loop and group 0 one after
C1PP_HD inline int conv1_pp_pre_barriers(int group) { return group ? 1 : 0; }
C1PP_HD inline int conv1_pp_post_barriers(int group) { return group ? 0 : 1; }
