// libgdx.so host side: the in-library sampling loops (diffusion/gaussian_diffusion.py:598-730, 879-993 and the multistep solvers).
// What each denoiser call of a loop does is planned once per entry-point call (gdx_call_plan.h); the loops index the plan by
// position.  C ABI in include/gdx.h; the handle is in handle.hip, forward_core in forward.hip, the step kernels in sampler.hip,
// the guidance arithmetic in guidance.hip, the bound's kernels in bound.hip.
#include "gdx_host.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace gdx;

static_assert(MODE_COND == GDX_COND && MODE_UNCOND == GDX_UNCOND && MODE_CFG == GDX_CFG, "gdx_call_plan.h restates gdx.h's modes");

static PlanRule plan_rule(const gdx_model* h) { return {h->guide_lo, h->guide_hi, h->guide_every, h->lc_every}; }

// A guided loop of entry `who` on a handle in a 3-pass compose mode (gdx.h gdx_set_guidance_compose): the refresh's stored
// difference and the layer cache's stored change are written for two row groups, so either is refused, before the first launch
static int compose_conflict(const gdx_model* h, const char* who, int mode) {
    if (pag_conflict(h, who, mode)) return -1;
    if (mode != GDX_CFG || !h->three_pass()) return 0;
    if (h->guide_every > 1)
        return fail(std::string(who) + ": the guidance refresh (gdx_set_guidance_refresh, every > 1) stores one cond-uncond difference; a "
                    "3-pass guidance compose mode (gdx_set_guidance_compose) has two: set every = 1");
    if (h->lc_every > 1)
        return fail(std::string(who) + ": the layer cache (gdx_set_layer_cache, every > 1) holds two row groups; a 3-pass guidance compose "
                    "mode (gdx_set_guidance_compose) runs three: set every = 1");
    return 0;
}

// The plan of the loop that block a (steps first_index .. last_idx) of entry `who` belongs to, and the refusals a block can meet
// there, all before the call's first launch: a numbering that needs a first index outside the schedule; a first guided call that
// would reuse a difference nobody stored; a first call that is partial while the stored change is missing or of another mode
// than the plan's.
template <typename A>
static int plan_block(const gdx_model* h, const char* who, const A* a, int last_idx, bool two_calls, CallPlan* p) {
    if (compose_conflict(h, who, a->mode)) return -1;
    const CallSeq q{a->mode, a->timestep_map, a->num_steps, a->first_index, a->k_base, last_idx, two_calls};
    if (!plan_loop(plan_rule(h), q, p)) return fail(std::string(who) + ": bad step range");
    if (p->begins_with_reuse() && !h->late.gd_valid)
        return fail(std::string(who) + ": a guided call would reuse the guidance difference, but none is stored: a block-wise "
                    "call (run_steps / k_base) must continue the loop that stored the difference");
    const PlannedCall& e = p->step(a->k_base);
    if (e.lc == LC_PARTIAL && !(h->late.lc_valid && h->late.lc_mode == e.K))
        return fail(std::string(who) + ": a partial call would add the stored change of the deep layers, but none of the planned mode "
                    "is stored: a block-wise call (run_steps / k_base) must continue the loop that stored the change");
    return 0;
}

// What the step kernel of a loop step in mode m gets as (x0_uncond, scale) after denoise_step left the prediction in h->x0.
// Guided without rescale: the uncond half and the scales, the kernel blends.  Guided with the handle's phi > 0: the rescaled
// guided prediction is formed here, in place on the cond half, and the kernel is called like on an unguided step (NULL, NULL).
// Under the guidance refresh (m = MODE_CFG_REFRESH / MODE_CFG_REUSE) the difference is stored or applied first (gdx_cfg_delta on
// the handle's buffer), and the step then continues as a guided one with (c, u or u', scale).  Every in-library loop asks here.
static int guided_operands(gdx_model* h, int m, const float* scale, hipStream_t s, const float** x0_uncond, const float** sc) {
    *x0_uncond = nullptr; *sc = nullptr;
    if (m < GDX_CFG) return 0;
    // 3-pass compose mode (never under the refresh: compose_conflict): composed, and rescaled under phi > 0, in place on the cond third
    if (h->three_pass()) return compose_x0(h, scale, nullptr, h->x0, s);
    const size_t n = (size_t)h->B * h->J * h->T;
    float* u = h->x0 + n;
    if (m != GDX_CFG) {
        // guidance refresh: a refresh stores d = c - u; a reuse, whose forward left only c, forms u' = c - d in u's place
        if (ws_need(h, &h->late.gd, sizeof(float) * n, s)) return -1;
        const bool store = m == MODE_CFG_REFRESH;
        const gdx_cfg_delta_args_t g{(int64_t)n, h->x0, store ? u : h->late.gd, store ? h->late.gd : u};
        if (gdx_cfg_delta(&g, (void*)s)) return -1;
        if (store) h->late.gd_valid = true;
    }
    if (h->guide_phi > 0.0f) return rescale_x0(h, h->x0, u, scale, nullptr, h->x0, s);
    *x0_uncond = u; *sc = scale;
    return 0;
}

// timestep-embedding table (and, V2, its W_coa image) for every kept step of a loop, shared by gdx_sample_loop and gdx_bpd_loop
static int build_step_tables(gdx_model* h, int num_steps, const int64_t* timestep_map, hipStream_t s) {
    const int d = h->d;
    const bool v2 = h->cfg.arch == GDX_ARCH_MDM;
    LateWorkspace& lw = h->late;
    // timestep-embedding table for every kept step, once per loop (same t for the whole batch:
    // gaussian_diffusion.py:712), through the respacing map (respace.py:124-129)
    if (lw.temb_table_rows < num_steps) {
        // regrown: the outgrown tables stay in the pool until the next gdx_prepare.  + GDX_ROW_PAD rows behind the last of the
        // three tables: the table linears run on the persistent GEMM, which reads / stores whole tiles
        lw.temb_table_rows = 0; lw.tables_valid = lw.c2t_valid = false;          // until all three stand
        if (ws_alloc(h, (void**)&lw.temb_table, sizeof(float) * (3 * (size_t)num_steps + GDX_ROW_PAD) * d, s) ||
            (v2 && ws_alloc(h, (void**)&lw.c2t_table, sizeof(float) * ((size_t)num_steps + GDX_ROW_PAD) * d, s)) ||
            ws_alloc(h, (void**)&lw.tmap_dev, sizeof(int64_t) * num_steps, s))
            return -1;
        lw.temb_table_rows = num_steps;
    }
    float* table = lw.temb_table;
    // the tables depend on the weights and the timestep map only: a loop run in blocks (run_steps) builds them once
    const bool tables_live = lw.tables_valid && (int)lw.tmap_host.size() == num_steps &&
                             !memcmp(lw.tmap_host.data(), timestep_map, sizeof(int64_t) * num_steps) && (!v2 || lw.c2t_valid);
    if (tables_live) return 0;
    lw.tmap_host.assign(timestep_map, timestep_map + num_steps);
    HIPCHK(hipMemcpyAsync(lw.tmap_dev, lw.tmap_host.data(), sizeof(int64_t) * num_steps, hipMemcpyHostToDevice, s));
    float* scratch0 = table + (size_t)lw.temb_table_rows * d;
    float* scratch1 = scratch0 + (size_t)lw.temb_table_rows * d;
    if (time_embed(h, lw.tmap_dev, num_steps, scratch0, scratch1, table, s)) return -1;
    if (v2) {
        // timestep half of the coarse slice of project_to_lat for every kept step, once per loop (same kernel as
        // gdx_forward's per-sample rows)
        HIPCHK(launch_small_linear(table, d, h->proj_coa.w, h->proj_coa.kpad, nullptr, lw.c2t_table, d, num_steps, d, d, 0, s));
        lw.c2t_valid = true;
    }
    lw.tables_valid = true;
    return 0;
}

// The planned call e of a loop, at its schedule index of the tables build_step_tables left: x0_out (pose layout) from the state x;
// tm: the token-major variant (x / x0_out unused); state: a captured step, which reads its row number from the device (e.idx = 0)
static int denoise_step(gdx_model* h, const float* x, const PlannedCall& e, float* x0_out, hipStream_t s, const int* state = nullptr,
                        bool tm = false) {
    const size_t row = (size_t)e.idx * h->d;
    const LateWorkspace& lw = h->late;
    return forward_core(h, x, lw.temb_table + row, 0, lw.c2t_table ? lw.c2t_table + row : nullptr, forward_mode(e.mode), x0_out, s,
                        {.state = state, .tm = tm, .lc = e.lc});
}

// Executed step k's slice of a noise tape that starts at step k_base and holds `rows` samples ([rows][per]) per step
static const float* tape_slice(const float* tape, int k, int k_base, size_t rows, size_t per) {
    return tape ? tape + (ptrdiff_t)(k - k_base) * (ptrdiff_t)(rows * per) : nullptr;
}

// One forward of a loop on the state x as its plan has it (e), and the step kernel's view of its output in h->x0:
// (x0_uncond, scale).  Every in-library loop's eager step asks here; sc_in: the loop's scales.
static int denoise_guided(gdx_model* h, const PlannedCall& e, const float* sc_in, const float* x, hipStream_t s,
                          const float** x0_uncond, const float** scale) {
    return denoise_step(h, x, e, h->x0, s) || guided_operands(h, e.mode, sc_in, s, x0_uncond, scale) ? -1 : 0;
}

// calc_bpd_loop (gaussian_diffusion.py:1537-1592): per step q_sample -> denoiser -> fused bound terms, through the SAME forward
// entry (pose-layout x_t, forward_core) the step-wise protocol reaches via gdx_forward, so both give the same bits.
extern "C" int gdx_bpd_loop(gdx_handle_t h, const gdx_bpd_loop_args_t* a, void* stream) {
    if (!h) return fail("gdx_bpd_loop: null handle");
    if (!a) return fail("gdx_bpd_loop: null argument");
    if (check_ready(h, "gdx_bpd_loop") || refuse_resampling(h, "gdx_bpd_loop")) return -1;
    if (!a->coef || !a->timestep_map || !a->x_start || !a->vb || !a->xstart_mse || !a->mse)
        return fail("gdx_bpd_loop: null argument");
    if (check_mode("gdx_bpd_loop", a->mode, a->scale) || pag_conflict(h, "gdx_bpd_loop", a->mode)) return -1;
    if (a->num_steps <= 0 || a->k_base < 0 || a->k_base >= a->num_steps || a->run_steps < 0 || a->k_base + a->run_steps > a->num_steps)
        return fail("gdx_bpd_loop: bad step range");
    if (a->inpaint_mask && !a->inpaint_motion) return fail("gdx_bpd_loop: mask without motion");
    hipStream_t s = (hipStream_t)stream;
    const int B = h->B;
    LateWorkspace& lw = h->late;
    const size_t per = (size_t)h->J * h->T;
    const size_t chunks = bpd_chunks(per);
    if (ws_need(h, &lw.bpd_xt, sizeof(float) * B * per, s) || ws_need(h, &lw.bpd_part, sizeof(float) * 4 * B * chunks, s) ||
        (!a->noise_tape && ws_need(h, &lw.bpd_z, sizeof(float) * B * per, s)))
        return -1;
    if (build_step_tables(h, a->num_steps, a->timestep_map, s)) return -1;
    gdx_bpd_args_t u;
    memset(&u, 0, sizeof(u));
    u.batch = B; u.njoints = h->J; u.frames = h->T;
    u.coef = a->coef; u.x_start = a->x_start; u.x_t = lw.bpd_xt;
    u.x0_cond = h->x0;
    u.inpaint_mask = a->inpaint_mask; u.inpaint_motion = a->inpaint_motion;
    u.clip_denoised = a->clip_denoised;
    u.vb = a->vb; u.xstart_mse = a->xstart_mse; u.mse = a->mse; u.ld = a->num_steps;
    u.workspace = lw.bpd_part;
    const int k_end = a->run_steps > 0 ? a->k_base + a->run_steps : a->num_steps;
    // no guidance refresh here: the steps draw independent x_t, so every guided call is a full one
    const CallPlan plan = plan_unnumbered(plan_rule(h), a->mode, a->timestep_map, a->num_steps - 1 - a->k_base, k_end - a->k_base, -1);
    for (int k = a->k_base; k < k_end; ++k) {
        const int idx = a->num_steps - 1 - k;
        if (a->noise_tape) {
            u.noise = tape_slice(a->noise_tape, k, a->k_base, B, per);
            if (gdx_q_sample(a->x_start, u.noise, a->coef, idx, (int64_t)(B * per), lw.bpd_xt, stream)) return -1;
        } else {
            u.noise = lw.bpd_z;
            if (gdx_bpd_xt_(a->x_start, a->coef, idx, B, (long)per, a->philox_seed, a->sample_offset, (uint32_t)k, lw.bpd_z, lw.bpd_xt, stream))
                return -1;
        }
        if (denoise_guided(h, plan.calls[k - a->k_base], a->scale, lw.bpd_xt, s, &u.x0_uncond, &u.scale)) return -1;
        u.step_index = idx; u.col = k;
        if (gdx_bpd_terms(&u, stream)) return -1;
    }
    if (a->prior_bpd) {
        u.prior = 1; u.prior_log_variance = a->prior_log_variance; u.step_index = a->num_steps - 1;
        u.vb = a->prior_bpd; u.ld = 1; u.col = 0;
        if (gdx_bpd_terms(&u, stream)) return -1;
    }
    return 0;
}

// The arguments U of a loop's step kernel at index idx, as far as every pose-layout step struct names them alike: the handle's
// shape, the loop's coefficients / state (updated in place) / inpainting / clip, and the denoiser's output as denoise_guided left it
template <typename U, typename A>
static U step_args(const gdx_model* h, const A* a, int idx, const float* x0_uncond, const float* scale) {
    U u;
    memset(&u, 0, sizeof(u));
    u.batch = h->B; u.njoints = h->J; u.frames = h->T;
    u.coef = a->coef; u.step_index = idx; u.x = a->x; u.out = a->x;
    u.x0_cond = h->x0; u.x0_uncond = x0_uncond; u.scale = scale;
    u.inpaint_mask = a->inpaint_mask; u.inpaint_motion = a->inpaint_motion; u.clip_denoised = a->clip_denoised;
    return u;
}

// The scaffold of the multistep loops gdx_plms_loop, gdx_dpm_loop, gdx_dpm_sde_loop and gdx_unipc_loop (`who`), whose argument
// structs A name the fields mode .. k_base alike: per step the denoiser through forward_core on the pose-layout state (the entry
// gdx_forward uses: same bits as the step-wise protocol), then step(idx, k, x0_uncond, scale, slot, plan), the entry's own fused
// launch; slot(k) = executed step k's place in the caller's ring of `ring` buffers (0: a->order of them) at a->*hist; two_calls: step 0
// makes a second denoiser call (plan.second_call(); the entry's step issues it).  No graph replay and no token-major variant:
// these solvers run 10-50 steps.  The argument checks need no handle and come first (then null handle, then not prepared), so
// every refusal precedes the first HIP call; missing() gives the entry's history refusal or nullptr.  A new multistep sampler
// is one more caller of this function ("Where a new in-library loop goes").
template <typename A, typename Missing, typename Step>
static int multistep_loop(const char* who, gdx_model* h, const A* a, int order_lo, int order_hi, const char* order_msg,
                          float* A::*hist, Missing missing, hipStream_t s, Step step, bool two_calls = false, int ring = 0) {
    const std::string w = std::string(who) + ": ";
    if (!a || !a->coef || !a->timestep_map || !a->x) return fail(w + "null argument");
    if (check_mode(who, a->mode, a->scale)) return -1;
    if (a->num_steps <= 0 || a->first_index < 0 || a->k_base < 0 || a->run_steps < 0 || a->first_index + a->k_base >= a->num_steps ||
        a->run_steps > a->first_index + 1)
        return fail(w + "bad step range");
    if (a->order < order_lo || a->order > order_hi) return fail(w + order_msg);
    if (a->inpaint_mask && !a->inpaint_motion) return fail(w + "mask without motion");
    if (const char* m = missing()) return fail(w + m);
    if (check_ready(h, who) || refuse_resampling(h, who)) return -1;
    if (h->B > 65535) return fail(w + "batch exceeds 65535");
    const int last_idx = a->run_steps > 0 ? a->first_index - a->run_steps + 1 : 0;
    CallPlan plan;
    if (plan_block(h, who, a, last_idx, two_calls, &plan)) return -1;
    if (build_step_tables(h, a->num_steps, a->timestep_map, s)) return -1;
    const size_t n = (size_t)h->B * h->J * h->T;
    const int depth = ring > 0 ? ring : a->order;
    auto slot = [&](int k) { return a->*hist + (size_t)(k % depth) * n; };
    int k = a->k_base;
    for (int idx = a->first_index; idx >= last_idx; --idx, ++k) {
        const float *x0u, *sc;
        if (denoise_guided(h, plan.step(k), a->scale, a->x, s, &x0u, &sc) || step(idx, k, x0u, sc, slot, plan)) return -1;
    }
    return 0;
}

// plms_sample_loop (gaussian_diffusion.py:995-1190): one fused plms_step_kernel launch per step (sampler.hip); the first step
// needs the state in the reference layout twice.
extern "C" int gdx_plms_loop(gdx_handle_t h, const gdx_plms_loop_args_t* a, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    return multistep_loop(
        "gdx_plms_loop", h, a, 2, 4, "order must be 2, 3 or 4", &gdx_plms_loop_args_t::eps_hist,
        [&] { return !a->eps_hist || !a->scratch ? "missing history (eps_hist and scratch are the caller's)" : nullptr; }, s,
        [&](int idx, int k, const float* x0u, const float* sc, auto slot, const CallPlan& plan) -> int {
            auto u = step_args<gdx_plms_step_args_t>(h, a, idx, x0u, sc);
            if (k == 0) {                               // pseudo improved Euler (:1043-1052): predictor, second forward, corrector
                u.kind = 6; u.eps_out = slot(0); u.out = a->scratch; u.pred_xstart = slot(1);
                if (gdx_plms_step(&u, stream)) return -1;
                const int idx2 = (idx - 1 + a->num_steps) % a->num_steps;
                if (denoise_guided(h, plan.second_call(), a->scale, a->scratch, s, &u.x0_uncond, &u.scale)) return -1;
                u.kind = 5; u.step_index_eps = idx2; u.x_eps = a->scratch; u.eps_hist[0] = slot(0); u.pred_prev = slot(1);
                u.eps_out = nullptr; u.out = a->x; u.pred_xstart = nullptr;
                return gdx_plms_step(&u, stream);
            }
            u.kind = k + 1 < a->order ? k + 1 : a->order;
            u.eps_out = slot(k);
            for (int j = 0; j < u.kind - 1; ++j) u.eps_hist[j] = slot(k - 1 - j);
            return gdx_plms_step(&u, stream);
        },
        true);
}

// dpm_solver_sample_loop (DPM-Solver++ multistep, gdx.h): one fused dpm_step_kernel launch per step (sampler.hip)
extern "C" int gdx_dpm_loop(gdx_handle_t h, const gdx_dpm_loop_args_t* a, void* stream) {
    return multistep_loop(
        "gdx_dpm_loop", h, a, 1, 3, "order must be 1, 2 or 3", &gdx_dpm_loop_args_t::hist,
        [&] { return a->order > 1 && !a->hist ? "missing history (hist is the caller's)" : nullptr; }, (hipStream_t)stream,
        [&](int idx, int k, const float* x0u, const float* sc, auto slot, const CallPlan& plan) -> int {
            auto u = step_args<gdx_dpm_step_args_t>(h, a, idx, x0u, sc);
            u.order = std::min(a->order, std::min(k + 1, idx + 1));      // warm-up at the start, lower order at the end
            for (int j = 0; j < u.order - 1; ++j) u.hist[j] = slot(k - 1 - j);
            u.pred_out = a->order > 1 ? slot(k) : nullptr;
            return gdx_dpm_step(&u, stream);
        });
}

// dpm_solver_sde_sample_loop (SDE-DPM-Solver++ multistep, gdx.h): gdx_dpm_loop with the noisy instantiation of dpm_step_kernel,
// whose noise is slice k - k_base of the tape or Philox draw k + 1
extern "C" int gdx_dpm_sde_loop(gdx_handle_t h, const gdx_dpm_sde_loop_args_t* a, void* stream) {
    return multistep_loop(
        "gdx_dpm_sde_loop", h, a, 1, 2, "order must be 1 or 2", &gdx_dpm_sde_loop_args_t::hist,
        [&] { return a->order > 1 && !a->hist ? "missing history (hist is the caller's)" : nullptr; }, (hipStream_t)stream,
        [&](int idx, int k, const float* x0u, const float* sc, auto slot, const CallPlan& plan) -> int {
            auto u = step_args<gdx_dpm_sde_step_args_t>(h, a, idx, x0u, sc);
            u.order = std::min(a->order, std::min(k + 1, idx + 1));      // warm-up at the start, first order on the step to sigma = 0
            u.hist[0] = u.order > 1 ? slot(k - 1) : nullptr;
            u.pred_out = a->order > 1 ? slot(k) : nullptr;
            u.noise = tape_slice(a->noise_tape, k, a->k_base, h->B, (size_t)h->J * h->T);
            u.philox_seed = a->philox_seed; u.sample_offset = a->sample_offset; u.rng_step = (uint32_t)(k + 1);
            return gdx_dpm_sde_step(&u, stream);
        });
}

// unipc_sample_loop (UniPC, gdx.h): one fused unipc_step_kernel launch per step (sampler.hip) -- the corrector of the step that
// led to a->x, then the predictor of the next input; a->base holds the corrected state, the ring is one deeper than the order
extern "C" int gdx_unipc_loop(gdx_handle_t h, const gdx_unipc_loop_args_t* a, void* stream) {
    return multistep_loop(
        "gdx_unipc_loop", h, a, 1, 3, "order must be 1, 2 or 3", &gdx_unipc_loop_args_t::hist,
        [&] { return !a->hist || !a->base || !a->coef_c ? "missing history (hist, base and coef_c are the caller's)" : nullptr; },
        (hipStream_t)stream,
        [&](int idx, int k, const float* x0u, const float* sc, auto slot, const CallPlan& plan) -> int {
            auto u = step_args<gdx_unipc_step_args_t>(h, a, idx, x0u, sc);
            u.corr_order = k == 0 || idx == 0 ? 0 : std::min(a->order, k);
            u.pred_order = std::min(a->order, std::min(k + 1, idx + 1));
            if (u.corr_order) u.x = a->base;                              // else the state itself: a->x
            u.coef_c = a->coef_c; u.base_out = a->base;
            for (int j = 0; j < std::max(u.corr_order, u.pred_order - 1); ++j) u.hist[j] = slot(k - 1 - j);
            u.pred_out = slot(k);
            return gdx_unipc_step(&u, stream);
        },
        false, a ? a->order + 1 : 0);
}

// ddim_reverse_sample_loop (DDIM inversion, gdx.h): multistep_loop's per-step pair -- denoise_guided on the pose-layout state, then
// one fused launch (ddim_reverse_step_kernel, sampler.hip) with step_args -- over ASCENDING indices.  An ascending twin and not a
// direction flag on multistep_loop: nothing else of that function applies here (no order, no history ring, no k_base, no second
// call, no refusal of plan_block), and its step range and CallSeq are both written for first_index counting down.  The
// plan is the unnumbered one, as in gdx_bpd_loop: the stored difference's numbering is defined for descending loops.
extern "C" int gdx_ddim_reverse_loop(gdx_handle_t h, int32_t mode, int32_t num_steps, int32_t first_index, int32_t run_steps,
                                     const float* coef, const int64_t* timestep_map, float* x, const float* scale,
                                     const uint8_t* inpaint_mask, const float* inpaint_motion, int32_t clip_denoised, void* stream) {
    const char* who = "gdx_ddim_reverse_loop";
    const std::string w = std::string(who) + ": ";
    if (!coef || !timestep_map || !x) return fail(w + "null argument");
    if (check_mode(who, mode, scale)) return -1;
    if (num_steps <= 0 || first_index < 0 || first_index >= num_steps || run_steps < 1 || run_steps > num_steps - first_index)
        return fail(w + "bad step range");
    if (inpaint_mask && !inpaint_motion) return fail(w + "mask without motion");
    if (check_ready(h, who) || refuse_resampling(h, who) || pag_conflict(h, who, mode)) return -1;
    if (h->B > 65535) return fail(w + "batch exceeds 65535");
    if (h->guide_every > 1)
        return fail(w + "the guidance refresh (gdx_set_guidance_refresh, every > 1) does not apply to the inversion: its numbering of "
                        "guided calls is defined for descending loops; set every = 1");
    hipStream_t s = (hipStream_t)stream;
    if (build_step_tables(h, num_steps, timestep_map, s)) return -1;
    const CallPlan plan = plan_unnumbered(plan_rule(h), mode, timestep_map, first_index, run_steps, +1);
    // the loop's operands under the names step_args reads
    const struct { const float* coef; float* x; const uint8_t* inpaint_mask; const float* inpaint_motion; int32_t clip_denoised; }
        a{coef, x, inpaint_mask, inpaint_motion, clip_denoised};
    for (int idx = first_index; idx < first_index + run_steps; ++idx) {
        const float *x0u, *sc;
        if (denoise_guided(h, plan.calls[idx - first_index], scale, x, s, &x0u, &sc)) return -1;
        if (gdx_ddim_reverse_step_(step_args<gdx::DdimReverseStepArgs>(h, &a, idx, x0u, sc), stream)) return -1;
    }
    return 0;
}

// parallel_sample_loop (parallel-in-time sampling, gdx.h): per iteration ONE denoiser call on the window's W planes as a batch of
// W x B samples -- gdx_forward itself: per-sample timestep rows, the blend that selects per sample by the guidance interval, the
// rescale --, ONE gdx_window_sweep launch, the stride from the sweep's errors (gdx_window_stride.h), the slide.  The one loop
// that synchronises its stream, once per iteration: the stride depends on the data.  Nothing of multistep_loop applies (no plan:
// every call is a full one at per-sample timesteps; no history; the step count of a call is not known in advance).
extern "C" int gdx_parallel_loop(gdx_handle_t h, int32_t kind, int32_t mode, int32_t num_steps, int32_t first_index, const float* coef,
                                 const int64_t* timestep_map, const double* threshold, int32_t window, float* planes,
                                 const float* scale, const uint8_t* inpaint_mask, const float* inpaint_motion, int32_t clip_denoised,
                                 const float* noise_tape, uint64_t philox_seed, uint64_t sample_offset, int32_t* anchor,
                                 int32_t max_iterations, int32_t* strides_out, int32_t strides_capacity, int32_t* iterations_out,
                                 void* stream) {
    const char* who = "gdx_parallel_loop";
    const std::string w = std::string(who) + ": ";
    if (!coef || !timestep_map || !threshold || !planes || !anchor || !iterations_out) return fail(w + "null argument");
    if (kind != GDX_SAMPLER_P && kind != GDX_SAMPLER_DDIM) return fail(w + "kind must be GDX_SAMPLER_P or GDX_SAMPLER_DDIM");
    if (check_mode(who, mode, scale)) return -1;
    if (num_steps <= 0 || first_index < 0 || first_index >= num_steps) return fail(w + "bad step range");
    const int K = first_index + 1;
    if (*anchor < 0 || *anchor > K) return fail(w + "anchor must lie in 0 .. first_index + 1");
    if (window < 1 || window > 64) return fail(w + "window must lie in 1 .. 64");
    if (max_iterations < 0 || strides_capacity < 0 || (strides_capacity > 0 && !strides_out))
        return fail(w + "bad max_iterations / strides_out");
    if (inpaint_mask && !inpaint_motion) return fail(w + "mask without motion");
    if (!h) return fail(w + "null handle");
    if (refuse_resampling(h, who)) return -1;
    if (h->guide_every > 1)
        return fail(w + "the guidance refresh (gdx_set_guidance_refresh, every > 1) needs memory across sequential denoiser calls; "
                        "the window's calls are not sequential: set every = 1");
    if (h->lc_every > 1)
        return fail(w + "the layer cache (gdx_set_layer_cache, every > 1) needs memory across sequential denoiser calls; the "
                        "window's calls are not sequential: set every = 1");
    if (pag_conflict(h, who, mode)) return -1;
    if (mode == GDX_CFG && h->three_pass())
        return fail(w + "a 3-pass guidance compose mode (gdx_set_guidance_compose) is not supported by the parallel loop, whose "
                        "window repeats one scale per slot: use GDX_GUIDE_JOINT, _TEXT or _SEED");
    if (check_ready(h, who)) return -1;
    if (h->B % window)
        return fail(w + "the handle is prepared for " + std::to_string(h->B) + " samples, which window = " + std::to_string(window) +
                    " does not divide (prepare it for window x batch)");
    if ((long)h->B * (mode == GDX_CFG ? 2 : 1) > 65535) return fail(w + "window x batch (x 2 under guidance) exceeds 65535");
    hipStream_t s = (hipStream_t)stream;
    const int WB = h->B, B = WB / window;
    const size_t per = (size_t)h->J * h->T, plane = (size_t)B * per;
    const size_t chunks = bpd_chunks(per);
    *iterations_out = 0;
    LateWorkspace& lw = h->late;
    if (ws_need(h, &lw.pl_x0, sizeof(float) * WB * per, s) || ws_need(h, &lw.pl_scale, sizeof(float) * WB, s) ||
        ws_need(h, &lw.pl_err, sizeof(double) * WB, s) || ws_need(h, &lw.pl_part, sizeof(double) * WB * chunks, s))
        return -1;
    // the model timestep of executed step k for every k a slot can name, one row of B per step: the window at anchor a reads rows
    // a .. a + W - 1 as its W x B timesteps; rows behind the last step (ignored tail slots) run at index 0
    std::vector<int64_t> ts((size_t)(K + window) * B);
    for (int k = 0; k < K + window; ++k)
        std::fill_n(ts.begin() + (size_t)k * B, B, timestep_map[k < K ? first_index - k : 0]);
    if (lw.pl_ts_cap < ts.size()) {                                // regrown, like the step tables
        if (ws_alloc(h, (void**)&lw.pl_ts, sizeof(int64_t) * ts.size(), s)) return -1;
        lw.pl_ts_cap = ts.size(); lw.pl_ts_host.clear();
    }
    if (lw.pl_ts_host != ts) {
        HIPCHK(hipStreamSynchronize(s));                           // an earlier call may still read the rows, or this one's fill run
        HIPCHK(hipMemcpy(lw.pl_ts, ts.data(), sizeof(int64_t) * ts.size(), hipMemcpyHostToDevice));
        lw.pl_ts_host.swap(ts);
    }
    if (mode == GDX_CFG)
        for (int j = 0; j < window; ++j)
            HIPCHK(hipMemcpyAsync(lw.pl_scale + (size_t)j * B, scale, sizeof(float) * B, hipMemcpyDeviceToDevice, s));
    std::vector<double> err((size_t)window * B);
    int a = *anchor, it = 0;
    while (a < K && (max_iterations == 0 || it < max_iterations)) {
        const int n = std::min(window, K - a);
        if (gdx_forward(h, planes, lw.pl_ts + (size_t)a * B, mode, mode == GDX_CFG ? lw.pl_scale : nullptr, lw.pl_x0, stream)) return -1;
        if (gdx_window_sweep(kind, B, h->J, h->T, n, coef, first_index - a, planes, lw.pl_x0, inpaint_mask, inpaint_motion, clip_denoised,
                             noise_tape ? noise_tape + (size_t)a * plane : nullptr, philox_seed, sample_offset, (uint32_t)(a + 1),
                             lw.pl_err, lw.pl_part, stream))
            return -1;
        HIPCHK(hipMemcpyAsync(err.data(), lw.pl_err, sizeof(double) * n * B, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const int stride = window_stride(err.data(), B, n, threshold, first_index - a);
        if (gdx_window_slide_(planes, (long)plane, window, stride, stream)) return -1;
        a += stride;
        *anchor = a;
        if (it < strides_capacity) strides_out[it] = stride;
        *iterations_out = ++it;
    }
    return 0;
}

// gdx_sample_loop while resampling is on (gdx_set_resample, repeats > 1): the hops [k_base, k_base + run_steps) of the walk of
// gdx_resample_plan.h over the WHOLE loop, levels first_index + 1 .. 0.  A reverse hop is the eager step of the plain loop --
// denoise_guided on the pose-layout state, then gdx_sampler_update --, a forward hop one renoise_kernel launch; hop k of either kind
// takes tape slice k - k_base or Philox draw k + 1.  The plan is the unnumbered one: every reverse hop takes the mode of its own
// model timestep, and nothing is carried from one denoiser call to the next.  No token-major path, no graph capture.
static int resample_loop(gdx_model* h, const gdx_loop_args_t* a, hipStream_t s) {
    const std::string w = "gdx_sample_loop: resampling (gdx_set_resample, repeats > 1) ";
    if (a->kind != GDX_SAMPLER_P && a->kind != GDX_SAMPLER_DDIM) return fail(w + "runs GDX_SAMPLER_P or GDX_SAMPLER_DDIM");
    if (a->n_dump) return fail(w + "does not support dump_steps: an executed-step number names no single state of the walk");
    if (a->const_noise) return fail(w + "does not support const_noise");
    if (h->guide_every > 1)
        return fail(w + "and the guidance refresh (gdx_set_guidance_refresh, every > 1) exclude each other: a forward hop invalidates "
                        "the stored difference; set every = 1");
    if (h->lc_every > 1)
        return fail(w + "and the layer cache (gdx_set_layer_cache, every > 1) exclude each other: a forward hop invalidates the "
                        "stored change; set every = 1");
    if (a->num_steps != h->rp_steps)
        return fail(w + "was set for a schedule of " + std::to_string(h->rp_steps) + " steps, the loop has " + std::to_string(a->num_steps));
    if (a->inpaint_mask && !a->inpaint_motion) return fail("gdx_sample_loop: mask without motion");
    const std::vector<Hop> hops = resample_walk(a->first_index + 1, h->rp_jump, h->rp_repeats);
    const long n_hops = (long)hops.size();
    if (a->k_base >= n_hops || (long)a->k_base + a->run_steps > n_hops) return fail("gdx_sample_loop: bad step range");
    const long k_end = a->run_steps > 0 ? (long)a->k_base + a->run_steps : n_hops;
    if (build_step_tables(h, a->num_steps, a->timestep_map, s)) return -1;
    LateWorkspace& lw = h->late;
    if (lw.rp_tab_rows < h->rp_steps) {                            // regrown, like the step tables
        lw.rp_tab_rows = 0; lw.rp_tab_valid = false;
        if (ws_alloc(h, (void**)&lw.rp_tab, sizeof(float) * 2 * (size_t)h->rp_steps, s)) return -1;
        lw.rp_tab_rows = h->rp_steps;
    }
    if (!lw.rp_tab_valid) {
        HIPCHK(hipMemcpyAsync(lw.rp_tab, h->rp_rows.data(), sizeof(float) * h->rp_rows.size(), hipMemcpyHostToDevice, s));
        lw.rp_tab_valid = true;
    }
    const size_t per = (size_t)h->J * h->T;
    PlanWalk walk{plan_rule(h), a->mode, a->timestep_map, false};
    for (long k = a->k_base; k < k_end; ++k) {
        const Hop& hop = hops[k];
        const float* z = tape_slice(a->noise_tape, (int)k, a->k_base, h->B, per);
        if (hop.forward) {
            if (gdx_renoise_(a->x, lw.rp_tab, hop.from, h->B, (long)per, z, a->philox_seed, a->sample_offset, (uint32_t)(k + 1), (void*)s))
                return -1;
            continue;
        }
        const float *x0u, *sc;
        if (denoise_guided(h, walk.visit(hop.to), a->scale, a->x, s, &x0u, &sc)) return -1;
        gdx_update_args_t u = step_args<gdx_update_args_t>(h, a, hop.to, x0u, sc);
        u.kind = a->kind; u.noise = z;
        u.philox_seed = a->philox_seed; u.sample_offset = a->sample_offset; u.rng_step = (uint32_t)(k + 1);
        if (gdx_sampler_update(&u, (void*)s)) return -1;
    }
    return 0;
}

extern "C" int gdx_sample_loop(gdx_handle_t h, const gdx_loop_args_t* a, void* stream) {
    if (check_ready(h, "gdx_sample_loop")) return -1;
    if (!a || !a->coef || !a->timestep_map || !a->x) return fail("gdx_sample_loop: null argument");
    if (check_mode("gdx_sample_loop", a->mode, a->scale)) return -1;
    if (a->num_steps <= 0 || a->first_index >= a->num_steps || a->first_index < 0 || a->run_steps < 0 || a->k_base < 0)
        return fail("gdx_sample_loop: bad step range");
    if (a->kind == GDX_SAMPLER_DDIM && (a->const_noise || a->n_dump))
        return fail("gdx_sample_loop: ddim_sample_loop supports neither const_noise nor dump_steps");  // :903-906
    if (h->rp_repeats > 1) return resample_loop(h, a, (hipStream_t)stream);
    hipStream_t s = (hipStream_t)stream;
    const int B = h->B;
    const int last_idx = a->run_steps > 0 && a->run_steps <= a->first_index ? a->first_index - a->run_steps + 1 : 0;
    CallPlan plan;
    if (plan_block(h, "gdx_sample_loop", a, last_idx, false, &plan)) return -1;
    if (build_step_tables(h, a->num_steps, a->timestep_map, s)) return -1;

    const int64_t per = (int64_t)h->J * h->T;
    const size_t tape_rows = a->const_noise ? 1 : B;             // samples per step of the noise tape
    int dump_i = 0;
    while (dump_i < a->n_dump && a->dump_steps[dump_i] < a->k_base) ++dump_i;     // entries of earlier blocks
    // (x0_uncond, scale): guided_operands' answer for the step
    auto fill_update = [&](gdx_update_args_t& u, int idx, int k, const float* x0_uncond, const float* scale) {
        u = step_args<gdx_update_args_t>(h, a, idx, x0_uncond, scale);
        u.kind = a->kind;
        u.noise = tape_slice(a->noise_tape, k, a->k_base, tape_rows, per);
        u.const_noise = a->const_noise;
        u.philox_seed = a->philox_seed; u.sample_offset = a->sample_offset; u.rng_step = (uint32_t)(k + 1);
    };
    auto eager_step = [&](int idx, int k) -> int {
        const float *x0u, *sc;
        if (denoise_guided(h, plan.step(k), a->scale, a->x, s, &x0u, &sc)) return -1;
        gdx_update_args_t u;
        fill_update(u, idx, k, x0u, sc);
        if (gdx_sampler_update(&u, stream)) return -1;
        while (a->dump && dump_i < a->n_dump && a->dump_steps[dump_i] <= k) {      // duplicates / stale entries never stall
            if (a->dump_steps[dump_i] == k)
                HIPCHK(hipMemcpyAsync(a->dump + (size_t)dump_i * B * per, a->x, sizeof(float) * B * per,
                                      hipMemcpyDeviceToDevice, s));
            ++dump_i;
        }
        return 0;
    };

    // Optional hipGraph replay of the step (gdx_set_graph_replay): ONE step is captured and replayed; everything that
    // changes from step to step (timestep-embedding row, coefficient row, Philox draw number, noise-tape slice) is read
    // from a two-int device state that a one-thread kernel advances at the end of the step.  Measured on MI355X /
    // ROCm 7.2 (tools/small_loop.py, 1000 steps, B=4 T=60 d=512 fp16): eager 0.307 ms/step, graph replay 0.337 -- the
    // ~65 small kernels of a step are bound by their GPU-side dispatch + ramp, not by host launch time, and a graph
    // node costs slightly more than a stream launch; so it is OFF by default and kept as a switch.
    // guidance interval: the modes this call's steps take (all the loop's own mode unless it is GDX_CFG)
    const int mode0 = plan.step(a->k_base).mode;
    bool uniform = true, any_guided = false;
    for (int k = plan.k_base; k < plan.k_end; ++k) {
        const int m = plan.step(k).mode;
        uniform = uniform && m == mode0;
        any_guided = any_guided || m >= GDX_CFG;
    }
    // Token-major fast path (sampler.hip, update_tm_kernel): with nothing but the noise tape living in the reference layout
    // (no inpainting, no dumps; the tape is read in place), the state stays in the input GEMM's operand layout for the whole
    // call -- one transpose in front, none per step (2 launches and ~40 MB per step less), the last update also writes the
    // sample in the reference layout.  Bit-identical to the general path (tests: fused Philox loop == step-wise Philox loop).
    // the guidance rescale has no token-major variant: a call that rescales a step takes the general path; nor has the guidance
    // refresh, whose calls also run eagerly under graph replay (the stored difference is host-tracked state)
    const bool rescales = h->guide_phi > 0.0f && any_guided;
    const bool refreshes = h->guide_every > 1 && any_guided;
    const bool composes = h->three_pass() && any_guided;          // nor has the 3-pass compose, whose calls also run eagerly
    if (!((uintptr_t)a->noise_tape & 15) && !a->inpaint_mask && !a->n_dump && !h->graph_replay && !h->keep_taps && h->T % 4 == 0 &&
        !rescales && !refreshes && !composes) {
        // guided loop: the state holds both halves (the same x feeds both passes).  An unguided step reads and writes the cond
        // half and mirrors into the uncond half only when the NEXT step of this call is guided (every call transposes the
        // state in afresh); a call without a guided step keeps one half, like a loop that is not guided at all.
        // GDX_TM_MIRROR=always mirrors on every unguided step of such a call (the A/B of DESIGN 4f).
        static const bool mirror_always = [] { const char* e = getenv("GDX_TM_MIRROR"); return e && !strcmp(e, "always"); }();
        const int Beff = any_guided ? 2 * B : B;
        // half modes: the fp32 state keeps the half operand's row stride, and the update kernel also writes that operand
        const int ldx = h->f16 ? h->in_x.kpad16 : h->in_x.kpad;
        HIPCHK(launch_transpose_in(a->x, h->xt.f, Beff, B, h->J, h->T, ldx, s));
        if (h->f16) HIPCHK(HFN(h->bf16, launch_transpose_in_f16, a->x, h->xt.h, Beff, B, h->J, h->T, ldx, s));
        gdx::UpdateTmDev u;
        memset(&u, 0, sizeof(u));
        u.kind = a->kind; u.B = B; u.J = h->J; u.T = h->T; u.ldx = ldx; u.ldo = h->ldo;
        u.coef = a->coef; u.xt = h->xt.f; u.x0t = h->x0t;
        u.const_noise = a->const_noise; u.seed = a->philox_seed; u.sample_offset = a->sample_offset;
        u.clip = a->clip_denoised;
        u.xt16 = h->xt.h; u.half_dtype = h->cfg.compute_dtype;
        int k = a->k_base;
        for (int idx = a->first_index; idx >= last_idx; --idx, ++k) {
            const int m = plan.step(k).mode;
            if (denoise_step(h, nullptr, plan.step(k), nullptr, s, nullptr, true)) return -1;
            u.scale = m == GDX_CFG ? a->scale : nullptr;
            u.mirror = any_guided && m != GDX_CFG && (mirror_always || (idx > last_idx && plan.step(k + 1).mode == GDX_CFG));
            u.step_index = idx; u.rng_step = (uint32_t)(k + 1);
            u.out_pose = idx == last_idx ? a->x : nullptr;
            u.noise = tape_slice(a->noise_tape, k, a->k_base, tape_rows, per);
            if (gdx_sampler_update_tm_(u, stream)) return -1;
        }
        return 0;
    }
    // the graph is ONE captured step: only a call whose steps all take the same mode can replay it
    const bool want_graph = h->graph_replay && !h->prof && !h->keep_taps && !a->n_dump && a->first_index - last_idx >= 8 && uniform && !refreshes &&
                            !composes && h->lc_every == 1;                     // the layer cache's calls differ from one another: eager
    int idx = a->first_index, k = a->k_base;
    if (want_graph) {
        // step 0 eagerly: it sets every kernel attribute and acquires the late workspace, so the captured step never allocates
        if (eager_step(idx, k)) return -1;
        --idx; ++k;
        bool ok = true;
        if (!h->gstream) {
            ok = hipStreamCreateWithFlags(&h->gstream, hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&h->gev_in, hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&h->gev_out, hipEventDisableTiming) == hipSuccess &&
                 hipMalloc((void**)&h->gstate, 64) == hipSuccess;
            if (!ok) { (void)hipGetLastError(); }
        }
        if (ok && h->gexec) {                                     // the previous loop's graph: its launches must have drained
            (void)hipStreamSynchronize(h->gstream);
            (void)hipGraphExecDestroy(h->gexec); h->gexec = nullptr;
            (void)hipGraphDestroy(h->ggraph); h->ggraph = nullptr;
        }
        if (ok) {
            ok = launch_set_state(h->gstate, idx, k, s) == hipSuccess && hipEventRecord(h->gev_in, s) == hipSuccess &&
                 hipStreamWaitEvent(h->gstream, h->gev_in, 0) == hipSuccess;
        }
        if (ok && hipStreamBeginCapture(h->gstream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            const int64_t counted = h->forward_samples;          // the capture enqueues no forward: the replays are counted
            int rc = denoise_step(h, a->x, PlannedCall{0, mode0}, h->x0, h->gstream, h->gstate);
            h->forward_samples = counted;
            const float *x0u = nullptr, *sc = nullptr;           // the rescale's launches depend on no per-step state: captured as they are
            if (!rc) rc = guided_operands(h, mode0, a->scale, h->gstream, &x0u, &sc);
            if (!rc) {
                gdx_update_args_t u;
                fill_update(u, 0, 0, x0u, sc);                    // noise: step 0's slice; the kernel adds state[1] * stride
                rc = gdx_sampler_update_state_(&u, h->gstate, (long)(tape_rows * per), (void*)h->gstream);
            }
            if (!rc && launch_advance_state(h->gstate, h->gstream) != hipSuccess) rc = -1;
            hipGraph_t g = nullptr;
            const hipError_t ee = hipStreamEndCapture(h->gstream, &g);
            if (rc || ee != hipSuccess || !g) {
                if (g) (void)hipGraphDestroy(g);
                (void)hipGetLastError();
                ok = false;
            } else if (hipGraphInstantiate(&h->gexec, g, nullptr, nullptr, 0) != hipSuccess) {
                (void)hipGraphDestroy(g);
                (void)hipGetLastError();
                h->gexec = nullptr;
                ok = false;
            } else {
                h->ggraph = g;
            }
        } else {
            ok = false;
            (void)hipGetLastError();
        }
        if (ok) {
            for (; idx >= last_idx; --idx, ++k) {
                HIPCHK(hipGraphLaunch(h->gexec, h->gstream));
                h->forward_samples += mode0 == GDX_CFG ? 2 * B : B;
            }
            HIPCHK(hipEventRecord(h->gev_out, h->gstream));
            HIPCHK(hipStreamWaitEvent(s, h->gev_out, 0));
            return 0;
        }
        clear_error();                                          // capture unavailable: finish the loop eagerly
    }
    for (; idx >= last_idx; --idx, ++k)
        if (eager_step(idx, k)) return -1;
    return 0;
}
