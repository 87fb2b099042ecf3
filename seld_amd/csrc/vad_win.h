// vad_win.h — the irregular frame window of the VAD path (preprocess_window's sorted offsets) as a launch argument: vad.hip's
// seld_vad_windows / _unwindow and vad_feat.hip's seld_vad_gather take the same host table and refuse the same ones.
#pragma once
#include "common.h"

namespace {

struct WinTable {
    int n, width;      // entries, offs[n - 1]
    int offs[SELD_VAD_MAX_WINDOW];
};

inline int win_table(const int32_t* offs, int Wn, WinTable& tb) {
    if (!offs || Wn < 1) return SELD_ERR_INVALID;
    if (Wn > SELD_VAD_MAX_WINDOW) return SELD_ERR_UNSUPPORTED;
    if (offs[0] != 0) return SELD_ERR_INVALID;
    for (int i = 0; i < Wn; ++i) {
        if (i && offs[i] < offs[i - 1]) return SELD_ERR_INVALID;
        tb.offs[i] = offs[i];
    }
    for (int i = Wn; i < SELD_VAD_MAX_WINDOW; ++i) tb.offs[i] = 0;
    tb.n = Wn, tb.width = offs[Wn - 1];
    return SELD_OK;
}

}  // namespace
