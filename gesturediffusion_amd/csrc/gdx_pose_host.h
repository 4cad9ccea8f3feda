// Host side of the pose-layout kernels (sampler.hip, guidance.hip, bound.hip): what their entry points share in front
// of and behind a launch.
#pragma once
#include <string>
#include <type_traits>

#include "gdx_pose_device.h"

// 0, or -1 with `msg` ("<entry>: launch failed") recorded, from the status of the launch just made
static inline int launch_status(const char* msg) { return hipGetLastError() == hipSuccess ? 0 : gdx_set_error_(msg); }

static inline int refuse(const char* who, const char* what) { return gdx_set_error_((std::string(who) + ": " + what).c_str()); }

// May a pose-layout kernel take its VEC = true instantiation: whole groups only, and every operand it reads or writes by
// group (nullptr = absent) aligned for the group access -- 16 bytes for floats, 4 for mask bytes.
static inline bool group_aligned(const float* p) { return !((uintptr_t)p & 15); }
static inline bool group_aligned(const uint8_t* p) { return !((uintptr_t)p & 3); }
template <typename... P>
static inline bool vec_ok(long per_sample, const P*... p) { return per_sample % 4 == 0 && (group_aligned(p) && ...); }
// ... of a kernel over a StepSrc: its operands and whatever else (`more`) the kernel reads or writes by group
template <typename... P>
static inline bool vec_ok(const gdx::StepSrc& s, const P*... more) {
    return vec_ok(s.per_sample, s.x, s.x0c, s.x0u, s.mask, s.motion, s.out, s.pred, more...);
}

// One launch of a kernel that exists as a <VEC = true> / <VEC = false> pair: `vec` (from vec_ok) picks the instantiation, the
// arguments convert to the kernel's parameter types
template <typename... A>
static inline void launch_vec(bool vec, void (*k_vec)(A...), void (*k_scalar)(A...), dim3 grid, dim3 block, hipStream_t stream,
                              std::common_type_t<A>... args) {
    void (*k)(A...) = vec ? k_vec : k_scalar;
    hipLaunchKernelGGL(k, grid, block, 0, stream, args...);
}

// The kernels' StepSrc from an entry's argument struct (every step struct names these fields alike); pred: where x0 goes
template <typename A>
static inline gdx::StepSrc step_src(const A* a, float* pred) {
    gdx::StepSrc s;
    s.per_sample = (long)a->njoints * a->frames;
    s.groups = (s.per_sample + 3) / 4;
    s.coef = a->coef; s.t = a->t; s.step_index = a->step_index;
    s.x = a->x; s.x0c = a->x0_cond; s.x0u = a->x0_uncond; s.scale = a->scale;
    s.mask = a->inpaint_mask; s.motion = a->inpaint_motion; s.clip = a->clip_denoised;
    s.out = a->out; s.pred = pred;
    return s;
}

// What gdx_plms_step, gdx_dpm_step, gdx_dpm_sde_step, gdx_unipc_step and gdx_ddim_reverse_step (`who`) share in front of their launch: the
// refusals in their order -- null argument, the entry's own kind / order check, shape, CFG, mask, the entry's history check (both
// return the refusal's text or nullptr) --, then the StepSrc and the (ceil(groups / 256), B) grid.  -1: refused, 1: nothing to do,
// 0: launch.
template <typename A, typename Entry, typename Hist>
static inline int step_begin(const char* who, const A* a, float* A::*pred, Entry entry_check, Hist hist_check, gdx::StepSrc& s, dim3& grid) {
    if (!a || !a->coef || !a->x || !a->x0_cond || !a->out) return refuse(who, "null argument");
    if (const char* m = entry_check()) return refuse(who, m);
    if (a->batch < 0 || a->njoints < 0 || a->frames < 0 || a->batch > 65535) return refuse(who, "bad shape");
    if (a->x0_uncond && !a->scale) return refuse(who, "CFG needs scale");
    if (a->inpaint_mask && !a->inpaint_motion) return refuse(who, "mask without motion");
    if (const char* m = hist_check()) return refuse(who, m);
    s = step_src(a, a->*pred);
    if (a->batch == 0 || s.per_sample == 0) return 1;
    grid = dim3((unsigned)((s.groups + 255) / 256), (unsigned)a->batch);
    return 0;
}
