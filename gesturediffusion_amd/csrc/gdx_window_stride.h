// How far the window of gdx_parallel_loop (gdx.h) advances after one iteration: the rule, on the host.  Plain C++17, no HIP, no
// handle: it compiles with the host compiler alone (tests/test_parallel_host.py does so).
#pragma once

namespace gdx {

// err [n][batch]: slot j's mean squared change of plane j + 1 per sample (gdx_window_sweep); threshold [num_steps], read at slot
// j's schedule index first_index - j.  Slot j passes when err[j][b] <= threshold for EVERY sample b; a NaN never passes (the
// comparison is false).  The stride is 1 + the number of LEADING slots that pass, capped at n: plane 1 is always final (it was
// computed from the exact anchor with the denoiser evaluated on the exact anchor), plane j + 1 is accepted when planes 1 .. j did
// not move by more than their thresholds; a pass behind a fail does not count.
inline int window_stride(const double* err, int batch, int n, const double* threshold, int first_index) {
    int lead = 0;
    for (; lead < n; ++lead) {
        const double thr = threshold[first_index - lead];
        bool pass = true;
        for (int b = 0; b < batch; ++b) pass = pass && err[(long)lead * batch + b] <= thr;
        if (!pass) break;
    }
    return lead + 1 < n ? lead + 1 : n;
}

}  // namespace gdx
