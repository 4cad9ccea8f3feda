// What each denoiser call of an in-library loop does, planned in one walk over the loop's calls in execution order: the rule of
// gdx_set_guidance_interval / _refresh / gdx_set_layer_cache (gdx.h) in the shape of GaussianDiffusion.guidance_plan /
// layer_cache_plan.  A guidance or caching rule belongs here; a loop asks the plan (loops.hip).  Plain C++17, no HIP, no handle.
#pragma once
#include <cstdint>
#include <vector>

namespace gdx {

// A call's mode: the loop's own three (gdx.h's GDX_COND / GDX_UNCOND / GDX_CFG; loops.hip asserts the values) and the plan's two
// answers under the guidance refresh, never a loop's own mode: a guided call that stores the difference c - u, and one that runs
// the conditional pass alone and reuses the stored difference
enum { MODE_COND = 0, MODE_UNCOND = 1, MODE_CFG = 2, MODE_CFG_REFRESH = 3, MODE_CFG_REUSE = 4 };
// A call's part in the layer cache (forward_core); LC_OFF: no cache on the handle, or a loop that takes no part
enum { LC_OFF = 0, LC_FULL = 1, LC_PARTIAL = 2 };

// what forward_core is run with for a planned mode m: a refresh is the full guided forward, a reuse the conditional pass alone
inline int forward_mode(int m) { return m == MODE_CFG_REFRESH ? MODE_CFG : m == MODE_CFG_REUSE ? MODE_COND : m; }

// the handle's settings the plan depends on: the guided model timesteps (inclusive), the refresh and the cache period (1 = off)
struct PlanRule { int64_t guide_lo, guide_hi; int guide_every, lc_every; };

// schedule index, MODE_*, LC_*, and K = the forward mode stored by the most recent full call before this one (-1: none, or LC_OFF)
struct PlannedCall { int idx, mode, lc = LC_OFF, K = -1; };

// The walk.  Guidance only while the call's model timestep lies in the interval, else the plain conditional pass.  The guided
// calls are numbered n = 0, 1, ... and n % guide_every decides between refresh and reuse; ALL calls are numbered m = 0, 1, ...
// and call m is full when m % lc_every == 0 or the stored mode K does not cover its own.  numbered = false: a sequence that
// takes part in neither (every guided call MODE_CFG, every call LC_OFF).  timestep_map is read at idx, under MODE_CFG only.
struct PlanWalk {
    PlanRule r; int mode; const int64_t* timestep_map; bool numbered;
    int n = 0, m = 0, K = -1;
    PlannedCall visit(int idx) {
        PlannedCall e{idx, mode};
        if (mode == MODE_CFG) {
            const int64_t tau = timestep_map[idx];
            if (!(r.guide_lo <= tau && tau <= r.guide_hi)) e.mode = MODE_COND;
            else if (numbered && r.guide_every > 1) e.mode = n++ % r.guide_every == 0 ? MODE_CFG_REFRESH : MODE_CFG_REUSE;
        }
        if (numbered && r.lc_every > 1) {
            const int c = forward_mode(e.mode);
            const bool covers = K == c || (K == MODE_CFG && c == MODE_COND);
            e.lc = m++ % r.lc_every == 0 || !covers ? LC_FULL : LC_PARTIAL;
            e.K = K;
            if (e.lc == LC_FULL) K = c;
        }
        return e;
    }
};

// The plan of a loop, in execution order, from the walk's first call to the last call of the block [k_base, k_end) that asked;
// k_walk: the executed step the walk started at; second: calls[1] is the second call of gdx_plms_loop's step 0
struct CallPlan {
    std::vector<PlannedCall> calls;
    int k_walk = 0, k_base = 0, k_end = 0;
    bool second = false;
    const PlannedCall& step(int k) const { return calls[k - k_walk + (second && k > k_walk)]; }   // executed step k's (first) call
    const PlannedCall& second_call() const { return calls[1]; }
    // The block's first guided call is a reuse: it needs the difference a refresh of this loop stored (PLMS's second call is
    // no candidate)
    bool begins_with_reuse() const {
        for (int k = k_base; k < k_end; ++k)
            if (step(k).mode >= MODE_CFG) return step(k).mode == MODE_CFG_REUSE;
        return false;
    }
};

// A descending loop that takes part in the refresh and the cache, as the block first_index .. last_index sees it; k_base: the
// loop's executed steps before the block; two_calls: gdx_plms_loop, whose step 0 makes a second call at the index below the first
struct CallSeq { int mode; const int64_t* timestep_map; int num_steps, first_index, k_base, last_index; bool two_calls; };

// Whether the numbering of a loop's calls matters: only then does a block need the calls before it
inline bool is_numbered(const PlanRule& r, int mode) { return (r.guide_every > 1 && mode == MODE_CFG) || r.lc_every > 1; }

// Execution order: first, then the second call if the loop has one, then first - 1, first - 2, ...  A numbered loop is walked
// from the WHOLE loop's first index, first_index + k_base (no counter lives in the handle, so a block gets the plan of the whole
// loop); false: that index lies outside the schedule.  Otherwise the walk starts at the block's own first_index and reads
// timestep_map at the block's indices only.
inline bool plan_loop(const PlanRule& r, const CallSeq& q, CallPlan* p) {
    const bool numbered = is_numbered(r, q.mode);
    if (numbered && q.first_index + q.k_base >= q.num_steps) return false;
    p->k_walk = numbered ? 0 : q.k_base;
    p->k_base = q.k_base; p->k_end = q.k_base + q.first_index - q.last_index + 1;
    p->second = q.two_calls && p->k_walk == 0;
    const int first = q.first_index + q.k_base - p->k_walk;
    PlanWalk w{r, q.mode, q.timestep_map, numbered};
    p->calls.assign(1, w.visit(first));
    if (p->second) p->calls.push_back(w.visit((first - 1 + q.num_steps) % q.num_steps));
    for (int idx = first - 1; idx >= q.last_index; --idx) p->calls.push_back(w.visit(idx));
    return true;
}

// A sequence that takes part in neither the refresh nor the cache (gdx_bpd_loop, whose steps draw independent x_t, and
// gdx_ddim_reverse_loop, whose indices ascend): `count` calls at first, first + dir, ..., each in the mode of its own timestep
inline CallPlan plan_unnumbered(const PlanRule& r, int mode, const int64_t* timestep_map, int first, int count, int dir) {
    CallPlan p;
    p.k_end = count;
    PlanWalk w{r, mode, timestep_map, false};
    for (int i = 0; i < count; ++i) p.calls.push_back(w.visit(first + i * dir));
    return p;
}

}  // namespace gdx
