// The hops of a resampled sampling loop (RePaint, Lugmayr et al. 2022, arXiv:2201.09865, section 4.2 "Resampling"), in execution
// order: the rule of gdx_set_resample (gdx.h) in the shape of GaussianDiffusion.resample_plan / resample_coef.  A resampling rule
// belongs here; the loop asks the walk (loops.hip).  Plain C++17, no HIP, no handle.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace gdx {

// States are counted in levels: level L is the input of the reverse step at schedule index L - 1, level 0 is the sample; a loop
// starts at level N = first_index + 1.  A reverse hop takes level from -> from - 1 (the step at index `to`), a forward hop
// level from -> from + jump.
struct Hop { bool forward; int from, to; };

// the jump levels 0, jump, 2 jump, ... with level + jump < N (RePaint's range(0, t_T - jump, jump), level 0 included)
inline bool is_jump_level(int level, int N, int jump) { return level % jump == 0 && level + jump < N; }
inline int resample_levels(int N, int jump) { return N > jump ? (N - jump - 1) / jump + 1 : 0; }

// denoiser calls and executed hops of the whole walk
inline long resample_calls(int N, int jump, int repeats) { return N + (long)resample_levels(N, jump) * (repeats - 1) * jump; }
inline long resample_hops(int N, int jump, int repeats) { return resample_calls(N, jump, repeats) + (long)resample_levels(N, jump) * (repeats - 1); }

// The walk.  Every jump level has repeats - 1 jumps left.  A reverse hop descends one level; on arriving at a jump level with
// jumps left one is used up, a forward hop goes `jump` levels up, and the descent goes on.  N = 6, jump = 2, repeats = 2:
// r5 r4 r3 r2 f(2->4) r3 r2 r1 r0 f(0->2) r1 r0.  repeats = 1, or jump >= N: the plain descent.
inline std::vector<Hop> resample_walk(int N, int jump, int repeats) {
    std::vector<Hop> hops;
    if (N <= 0 || jump < 1 || repeats < 1) return hops;
    std::vector<int> left((size_t)resample_levels(N, jump), repeats - 1);
    hops.reserve((size_t)resample_hops(N, jump, repeats));
    int level = N;
    while (level > 0) {
        hops.push_back({false, level, level - 1});
        --level;
        if (is_jump_level(level, N, jump) && left[level / jump] > 0) {
            --left[level / jump];
            hops.push_back({true, level, level + jump});
            level += jump;
        }
    }
    return hops;
}

// The forward hop from -> to is x <- a x + b z with a = sqrt(r), b = sqrt(1 - r), r = abar_lvl[to] / abar_lvl[from] and abar_lvl =
// [1, alpha_bar ...] of the loop's (respaced) schedule: `to - from` steps of the forward process in one.  Computed in fp64 and
// rounded to fp32 once each.
inline void resample_coef(const double* alpha_bar, int from, int to, float* a, float* b) {
    const double hi = from == 0 ? 1.0 : alpha_bar[from - 1], r = alpha_bar[to - 1] / hi;
    *a = (float)std::sqrt(r);
    *b = (float)std::sqrt(1.0 - r);
}

}  // namespace gdx
