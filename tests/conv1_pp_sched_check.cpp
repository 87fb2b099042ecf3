// Host walk of the ping-pong first-block forward's schedule (seld_amd/csrc/conv1_pp_sched.h, the header the kernel includes), built and run by
// test_conv1_pingpong_cpu.py.  usage: conv1_pp_sched_check B H [B H ...]
// For every shape it replays the control flow of conv_first_fwd_pool_sbpp_kernel's main loop per (block, wave group):
//   pre barriers; for each trip: [work if active] barrier [work if active] barrier; post barriers
// and checks that (1) every tile is visited exactly once, by the virtual workgroup and in the order of the 4-wave kernel (tile = v + i * vgrid,
// i ascending, no gap in a stream), (2) both groups of every block take the same number of barriers, (3) the matrix segments of the two groups
// of a block never share a barrier interval, (4) every virtual workgroup of the 4-wave grid is played by exactly one (block, group).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "conv1_pp_sched.h"

static int fail(const char* what, int B, int H, int a, int b) {
    std::fprintf(stderr, "FAIL %s: B=%d H=%d (%d, %d)\n", what, B, H, a, b);
    return 1;
}

static int check(int B, int H) {
    const Conv1PpSched s = conv1_pp_sched(B, H);
    if (s.ntiles != B * ((H + 9) / 10) || s.vgrid != (s.ntiles < 512 ? s.ntiles : 512) || s.nblocks * 2 < s.vgrid || s.trips < 1)
        return fail("geometry", B, H, s.vgrid, s.nblocks);
    std::vector<int> visits(s.ntiles, 0), played(s.vgrid, 0);
    for (int block = 0; block < s.nblocks; ++block) {
        int barriers[2];
        std::vector<int> mfma_interval[2];      // barrier intervals (index = barriers taken so far) in which the group runs a matrix segment
        for (int g = 0; g < 2; ++g) {
            const int v = conv1_pp_virtual(block, g);
            if (v < 0) return fail("virtual workgroup", B, H, block, g);
            if (v < s.vgrid) ++played[v];
            int n = conv1_pp_pre_barriers(g);
            bool was_active = true;
            for (int it = 0; it < s.trips; ++it) {
                const bool act = conv1_pp_active(s, v, it);
                if (act && !was_active) return fail("gap in a tile stream", B, H, v, it);
                was_active = act;
                if (act) {
                    const int tile = conv1_pp_tile(s, v, it);
                    if (tile < 0 || tile >= s.ntiles || tile != v + it * s.vgrid) return fail("tile", B, H, v, it);
                    ++visits[tile];
                    mfma_interval[g].push_back(n);
                }
                n += 2;
            }
            barriers[g] = n + conv1_pp_post_barriers(g);
        }
        if (barriers[0] != barriers[1] || barriers[0] != 2 * s.trips + 1) return fail("barrier count", B, H, barriers[0], barriers[1]);
        for (int a : mfma_interval[0])
            for (int b : mfma_interval[1])
                if (a == b) return fail("matrix segments in one interval", B, H, block, a);
    }
    for (int t = 0; t < s.ntiles; ++t)
        if (visits[t] != 1) return fail("tile visits", B, H, t, visits[t]);
    for (int v = 0; v < s.vgrid; ++v)
        if (played[v] != 1) return fail("virtual workgroup played", B, H, v, played[v]);
    // a virtual workgroup past the trip count's reach would lose tiles
    if ((long long)s.trips * s.vgrid < s.ntiles) return fail("trips", B, H, s.trips, s.vgrid);
    std::printf("ok B=%d H=%d: %d tiles, %d virtual workgroups, %d blocks, %d trips, %d barriers per wave\n", B, H, s.ntiles, s.vgrid,
                s.nblocks, s.trips, 2 * s.trips + 1);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3 || (argc & 1) == 0) return 2;
    for (int i = 1; i + 1 < argc; i += 2)
        if (check(std::atoi(argv[i]), std::atoi(argv[i + 1]))) return 1;
    return 0;
}
