"""The loops' planner (csrc/gdx_call_plan.h) against GaussianDiffusion.guidance_plan / layer_cache_plan, on the CPU: the header
compiles as plain C++17 without HIP, and a short probe (tests/call_plan_probe.cpp) prints its plans for the grid of
test_layer_cache_host.test_plan_against_the_restatements_counter with guidance_refresh in {1, 2, 3}, a one-step loop and a
two-call PLMS loop.  Whole plans, every split point (a block gets the plan of the whole loop), the two refusal predicates, the
unnumbered sequences and the step range that is refused only where the numbering needs it."""
import os
import subprocess

import pytest

from conftest import REPO
from test_dpm_host import diffusion
from test_guidance_interval_host import _full
from test_layer_cache_host import MID

COND, UNCOND, CFG, REFRESH, REUSE = range(5)
LC_OFF, LC_FULL, LC_PARTIAL = range(3)
I64 = (-2**63, 2**63 - 1)
INTERVALS = (None, MID, (1, 0), (0, 0), (300, 800), (500, 999))


def _probe(tmp):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if subprocess.run(
        ["sh", "-c", f"command -v {c}"], capture_output=True).returncode == 0), None)
    assert cxx, "no C++ compiler"
    exe = os.path.join(tmp, "call_plan_probe")
    built = subprocess.run([cxx, "-std=c++17", "-Werror", "-I", os.path.join(REPO, "gesturediffusion_amd", "csrc"),
                            os.path.join(REPO, "tests", "call_plan_probe.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = _probe(str(tmp_path_factory.mktemp("call_plan")))

    def run(lines):
        got = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(got) == sum(1 for ln in lines if ln[0] != "M")
        out = []
        for ln in got:
            if ln == "bad":
                out.append(None)
                continue
            begin, reuse, *calls = ln.split()
            out.append((int(begin), bool(int(reuse)), [tuple(int(v) for v in c.split(",")) for c in calls]))
        return out
    return run


def _map_line(tmap):
    return "M %d %s" % (len(tmap), " ".join(str(t) for t in tmap))


def _loop_line(iv, refresh, lc_every, mode, n, first_index, k_base, last_index, plms):
    lo, hi = iv or I64
    return f"L {lo} {hi} {refresh} {lc_every} {mode} {n} {first_index} {k_base} {last_index} {int(plms)}"


def _python_plan(df, iv, refresh, lc_every, guided, plms, skip):
    """The loop's calls in execution order as (idx, mode, lc, K), from the package's two plans alone."""
    n = df.num_timesteps
    idx = list(range(n - skip))[::-1]
    if plms:
        idx.insert(1, (idx[0] - 1) % n)
    if guided:
        word = df.guidance_plan(iv, refresh, plms=plms, skip_timesteps=skip)
        modes = [COND if w == "off" else CFG if refresh == 1 else REFRESH if w == "refresh" else REUSE for w in word]
    else:
        modes = [COND] * len(idx)
    assert len(modes) == len(idx)
    if lc_every == 1:
        return [(i, m, LC_OFF, -1) for i, m in zip(idx, modes)]
    what = df.layer_cache_plan((lc_every, 1), iv, refresh, guided=guided, plms=plms, skip_timesteps=skip)
    plan, stored = [], -1
    for i, m, w in zip(idx, modes, what):
        plan.append((i, m, LC_FULL if w == "full" else LC_PARTIAL, stored))
        if w == "full":
            stored = {REFRESH: CFG, REUSE: COND}.get(m, m)
    return plan


def _cases():
    for df in (diffusion("cosine", "ddim10"), diffusion("linear", "logsnr10"), diffusion("cosine", [20]), _full()):
        n = df.num_timesteps
        for iv in INTERVALS:
            for plms in (False, True):
                for skip in (0, 3, n - 1):                   # n - 1: a one-step loop; PLMS: two calls, both at valid indices
                    for refresh in (1, 2, 3):
                        for guided in (True, False):
                            for lc_every in (1, 2, 3):
                                yield df, iv, plms, skip, refresh, guided, lc_every


def test_plans_and_every_split_point_against_the_python_plans(ask):
    """Whole plans equal the Python plans entry for entry; for every split point k the block that starts at executed step k and
    runs to the end reads exactly the whole plan's entries from its position on; begins_with_reuse is what the Python plan says.
    The 1000-step schedule, to stay quick: the whole tail at the first four, the middle and the last two k, and two-step blocks
    at every seventh k (7 is coprime to every period of the grid, so every residue of both numberings is met)."""
    lines, want, last_map, seen, sizes = [], [], None, set(), set()
    for df, iv, plms, skip, refresh, guided, lc_every in _cases():
        tmap, n = df._timestep_map(), df.num_timesteps
        if tmap != last_map:
            lines.append(_map_line(tmap))
            last_map = tmap
        plan = _python_plan(df, iv, refresh, lc_every, guided, plms, skip)
        steps = n - skip
        sizes.add((steps, len(plan)))
        assert len(plan) == steps + (1 if plms else 0) and all(0 <= e[0] < n for e in plan)
        numbered = (guided and refresh > 1) or lc_every > 1
        for e in plan:                                       # what the cases must include
            if e[2] == LC_FULL and e[3] == COND and e[1] in (CFG, REFRESH):
                seen.add("promotion")
            if e[2] == LC_PARTIAL and e[3] == CFG and e[1] in (COND, REUSE):
                seen.add("cfg serves cond")
        pos = lambda k: k + (1 if plms and k > 0 else 0)     # noqa: E731
        for k in range(steps):
            tails = (None,) if n <= 20 or k in (0, 1, 2, 3, steps // 2, steps - 2, steps - 1) else ()
            for run in tails + ((2,) if n > 20 and k % 7 == 0 and k + 2 <= steps else ()):
                end = steps if run is None else k + run
                lines.append(_loop_line(iv, refresh, lc_every, CFG if guided else COND, n, n - 1 - skip - k, k, n - 1 - skip - (end - 1), plms))
                own = plan[pos(k):pos(end)]
                firsts = [plan[pos(j)][1] for j in range(k, end) if plan[pos(j)][1] >= CFG]      # PLMS's second call: no candidate
                # an unnumbered block is walked from its own first index: it sits at position 0 of its plan
                want.append((pos(k) if numbered or k == 0 else 0, bool(firsts) and firsts[0] == REUSE, own))
    got = ask(lines)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, [ln for ln in lines if ln[0] != "M"][i])
    assert seen == {"promotion", "cfg serves cond"}
    assert (1, 1) in sizes and (1, 2) in sizes


def test_first_call_partial_is_read_off_the_plan(ask):
    """The layer cache's refusal asks the block's first call: LC_PARTIAL with the K of the whole loop's plan, at every split."""
    df = diffusion("cosine", "ddim10")
    n = df.num_timesteps
    lines = [_map_line(df._timestep_map())]
    want = []
    for iv, refresh, lc_every, plms in ((MID, 2, 3, False), (MID, 1, 4, True), (None, 2, 3, True), ((300, 800), 1, 4, True)):
        plan = _python_plan(df, iv, refresh, lc_every, True, plms, 0)
        for k in range(n):
            lines.append(_loop_line(iv, refresh, lc_every, CFG, n, n - 1 - k, k, n - 1 - k, plms))
            want.append(plan[k + (1 if plms and k > 0 else 0)])
    got = ask(lines)
    assert [g[2][0] for g in got] == want
    assert {w[2] for w in want} == {LC_FULL, LC_PARTIAL} and {w[3] for w in want} == {-1, COND, CFG}


def test_step_range_is_refused_only_where_the_numbering_needs_it(ask):
    """first_index + k_base outside the schedule: accepted while no numbering matters, and timestep_map is then indexed at the
    block's own indices only (the map handed over ends at first_index); refused as soon as the refresh (under GDX_CFG) or the
    cache is on."""
    tmap = diffusion("cosine", "ddim10")._timestep_map()
    short = tmap[:6]                                         # indices 0 .. 5
    lines = [_map_line(short)]
    cases = [(CFG, 1, 1, True), (COND, 3, 1, True), (UNCOND, 2, 1, True), (CFG, 2, 1, False), (CFG, 1, 2, False),
             (COND, 1, 3, False), (UNCOND, 2, 2, False)]
    for mode, refresh, lc_every, _ in cases:
        lines.append(_loop_line(MID, refresh, lc_every, mode, 10, 5, 100, 2, False))
    got = ask(lines)
    for (mode, refresh, lc_every, ok), g in zip(cases, got):
        if not ok:
            assert g is None, (mode, refresh, lc_every)
            continue
        want = [(i, (CFG if MID[0] <= short[i] <= MID[1] else COND) if mode == CFG else mode, LC_OFF, -1) for i in (5, 4, 3, 2)]
        assert g == (0, False, want), (mode, refresh, lc_every)
    assert {w[1] for w in got[0][2]} == {COND, CFG}
    # in range, the same blocks are planned under every setting
    lines = [_map_line(tmap)] + [_loop_line(MID, r, lc, mode, 10, 5, 4, 2, False) for mode, r, lc, _ in cases]
    assert all(g is not None and [e[0] for e in g[2]] == [5, 4, 3, 2] for g in ask(lines))


def test_unnumbered_sequences(ask):
    """gdx_bpd_loop's and gdx_ddim_reverse_loop's form: each call in the mode of its own timestep, whatever the refresh and the
    cache say, descending and ascending, read at the calls' own indices only."""
    df = diffusion("cosine", "ddim10")
    tmap = df._timestep_map()
    lines, want = [], []
    for iv in INTERVALS:
        flags = df.guided_steps(iv)
        lo, hi = iv or I64
        for mode in (COND, UNCOND, CFG):
            for refresh, lc_every in ((1, 1), (2, 1), (1, 2), (3, 3)):
                for first, count, step in ((9, 10, -1), (6, 3, -1), (0, 10, 1), (2, 5, 1), (4, 1, 1)):
                    used = [first + i * step for i in range(count)]
                    lines.append(_map_line(tmap[:max(used) + 1]))
                    lines.append(f"U {lo} {hi} {refresh} {lc_every} {mode} {first} {count} {step}")
                    want.append((0, False, [(i, (CFG if flags[i] else COND) if mode == CFG else mode, LC_OFF, -1) for i in used]))
    assert ask(lines) == want
