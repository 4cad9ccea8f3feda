"""Every entry of include/gdx.h that takes a `stream`, run on a NON-DEFAULT stream and compared bit for bit with its run on the
default stream (tests/stream_cases.py is the case table; tests/test_streams_host.py holds it against the header).  The kernels
are deterministic -- no atomics, fixed reduction orders -- so there is no tolerance anywhere in this module.

The delayed-input protocol, per case (run_protocol):
  1. reference: a fresh handle, inputs X, the default stream; synchronise; keep every output.
  2. decoy: a second fresh handle of the same configuration, under torch.cuda.stream(side), one run with OTHER inputs (another
     tensor seed, another Philox seed); synchronise the device.  The workspace now holds values that are wrong for X, and every
     first-use allocation lies behind us.
  3. poison: every floating input buffer is filled with NaN, every output buffer too; integer inputs (timesteps, indices, masks)
     keep the decoy's valid values, so a kernel that runs early reads wrong data, never an out-of-range index.  Outputs that a
     Python wrapper allocates itself are filled with NaN and released, so that the allocator hands the same blocks out again.
  4. gated phase, all on `side` with no host synchronisation in between: a gate that keeps the stream busy, an event, the
     device-to-device copies of X into the input buffers, the call, the copies of the outputs.
  5. synchronise `side`; every output equals the reference's as int32 words (NaNs compare too).
A launch, copy or fill inside the call that went to another stream than `side` runs while the gate is still busy: it reads
NaN or the decoy's values, or its result is overwritten, and the case fails.

What keeps a case from passing vacuously: side.cuda_stream != 0; for an entry that does not synchronise, the gate's event is
still pending when the call has returned to the host, else the case FAILS ("gate too short"); for one that synchronises the
stream itself (stream_cases.SYNCS) the same is checked immediately before the call.  The gate is torch.cuda._sleep where its
length follows its argument, else a dependent chain of matmuls; it is timed once per session with a pair of events and sized per
case: at least ten times the host duration of the case's own enqueue (measured on the reference run) and at least 40 ms.  Both
numbers of a session go to the file GDX_STREAM_GATE_RECORD names (profiles/stream_gate.txt).

The module keeps two side streams alive at most (the second one for the two-handle test), besides the library's own graph stream."""
import ctypes as C
import functools
import os
import time
import types

import numpy as np
import pytest
import torch

import stream_cases as SC
from conftest import load_golden, weights_from
from gesturediffusion_amd import _lib
from gesturediffusion_amd import engine as E
from test_dpm_host import diffusion
from test_gpu_parity import TINY, build_model, dev

pytestmark = pytest.mark.gpu

B = 3
NAN = float("nan")
MIN_GATE_MS = 40.0                     # the floor asked of a gate is 20 ms; twice that, against a hiccup of the host between gate and call
MARGIN = 10.0                          # gate >= MARGIN x the host duration of the case's enqueue
MID = (300, 700)                       # ddim10's model timesteps are 0, 100, ..., 900: guided on five of the ten steps
F32, F16, BF16 = _lib.GDX_DTYPE_F32, _lib.GDX_DTYPE_F16, _lib.GDX_DTYPE_BF16
P, DDIM = _lib.GDX_SAMPLER_P, _lib.GDX_SAMPLER_DDIM
MODE = {"cond": E.GDX_COND, "uncond": E.GDX_UNCOND, "cfg": E.GDX_CFG}
STATS = {"cases": 0, "slowest": ("", 0.0, 0.0), "shortest_gate": None}


# ------------------------------------------------------------------------------------------------------ streams and the gate
@functools.lru_cache(maxsize=None)
def side_stream(i=0):
    assert i in (0, 1), "at most two side streams (the machines run with four hardware queues)"
    s = torch.cuda.Stream(device=dev())
    assert s.cuda_stream != 0, "torch.cuda.Stream() returned the default stream"
    return s


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


class Gate:
    """gate(ms): work on the current stream that takes at least `ms` milliseconds and touches no tensor of a case."""

    def __init__(self):
        d = dev()
        cycles = 20_000_000
        torch.cuda._sleep(1000)
        t1, t2 = _event_ms(lambda: torch.cuda._sleep(cycles)), _event_ms(lambda: torch.cuda._sleep(2 * cycles))
        if t1 > 1.0 and 1.5 < t2 / t1 < 2.5:
            self.kind, self.unit, self.per_ms = "torch.cuda._sleep", "cycles", 2 * cycles / t2
            self.note = f"_sleep({cycles}) {t1:.2f} ms, _sleep({2 * cycles}) {t2:.2f} ms"
        else:                                     # _sleep does not follow its argument here: a dependent chain of matmuls
            self.a = torch.randn(2048, 2048, device=d) / 2048 ** 0.5
            self.b = torch.randn(2048, 2048, device=d)
            self._chain(4)
            t = _event_ms(lambda: self._chain(40))
            self.kind, self.unit, self.per_ms = "matmul chain 2048^3", "matmuls", 40 / t
            self.note = f"_sleep gave {t1:.2f} / {t2:.2f} ms for {cycles} / {2 * cycles} cycles; 40 matmuls {t:.2f} ms"
        self.check_ms = _event_ms(lambda: self(MIN_GATE_MS))
        assert self.check_ms >= MIN_GATE_MS, f"a {MIN_GATE_MS} ms gate took {self.check_ms:.2f} ms ({self.kind}: {self.note})"

    def _chain(self, n):
        x = self.b
        for _ in range(n):
            x = self.a @ x
        self.b = x

    def __call__(self, ms):
        n = int(1.25 * ms * self.per_ms) + 1      # a quarter more than the calibration asks for
        if self.unit == "cycles":
            torch.cuda._sleep(n)
        else:
            self._chain(n)


@functools.lru_cache(maxsize=None)
def gate():
    return Gate()


@pytest.fixture(scope="module", autouse=True)
def gate_record():
    yield
    path = os.environ.get("GDX_STREAM_GATE_RECORD")
    if path and STATS["cases"]:
        g = gate()
        name, enq, used = STATS["slowest"]
        with open(path, "w") as f:
            f.write(f"gate: {g.kind}; calibration (one pair of events each): {g.note}; a {MIN_GATE_MS:.0f} ms request measured "
                    f"{g.check_ms:.2f} ms\n"
                    f"cases under the protocol: {STATS['cases']}; rule per case: gate = max({MIN_GATE_MS:.0f} ms, {MARGIN:.0f} x the "
                    f"host duration of the case's enqueue on the default-stream reference run)\n"
                    f"slowest enqueue: {enq:.3f} ms ({name}), its gate {used:.1f} ms = {used / max(enq, 1e-9):.1f} x\n"
                    f"shortest gate requested: {STATS['shortest_gate']:.1f} ms\n")


# ------------------------------------------------------------------------------------------------------------------ helpers
def bits(t):
    t = t.detach().contiguous().reshape(-1)
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.uint8)


def same_bits(a, b):
    if not isinstance(a, torch.Tensor):
        return type(a) is type(b) and a == b
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def cur():
    return C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rn(g, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=g).to(dtype).to(dev())


def ri(g, lo, hi, *shape):
    return torch.randint(lo, hi, shape, generator=g, dtype=torch.int64).to(dev())


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev())


class Case:
    """setup() -> state: a fresh handle, prepared (on the current stream; None for a handle-free entry).
    inputs(g, which) -> {name: tensor}: the call's device operands, floating ones drawn from g; which = 0 the real run, 1 the decoy.
    outputs() -> {name: tensor}: output buffers the harness owns and fills with NaN before every call.
    call(state, i, o, which) -> {name: tensor or host value}: the outputs to compare (o's buffers, tensors a wrapper allocated,
    in-place operands of i, host values)."""

    def __init__(self, setup, inputs, call, outputs=None):
        self.setup, self.inputs, self.call, self.outputs = setup, inputs, call, outputs or (lambda: {})


def clone_all(d):
    return {k: v.clone() for k, v in d.items()}


def keep(outs):
    return {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in outs.items()}


def reference(case, seed=0):
    """Step 1 on the default stream -> (X, outputs, host milliseconds of the enqueue)."""
    assert torch.cuda.current_stream(dev()).cuda_stream == 0
    state = case.setup()
    X = case.inputs(gen(1000 + seed), 0)
    i, o = clone_all(X), case.outputs()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = case.call(state, i, o, 0)
    enq = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    ref = keep(outs)
    for k, v in ref.items():
        if isinstance(v, torch.Tensor) and v.is_floating_point():
            assert not torch.isnan(v).all(), f"the reference's output {k} is all NaN"
    return X, ref, enq


def assert_equal(got, ref, what):
    assert set(got) == set(ref)
    bad = [k for k in ref if not same_bits(got[k], ref[k])]
    detail = ""
    if bad and isinstance(ref[bad[0]], torch.Tensor) and got[bad[0]].shape == ref[bad[0]].shape:
        n = int((bits(got[bad[0]]) != bits(ref[bad[0]])).sum())
        detail = f" ({bad[0]}: {n} of {bits(ref[bad[0]]).numel()} words differ, {int(torch.isnan(got[bad[0]].float()).sum())} NaN)"
    assert not bad, f"{what}: outputs {bad} differ from the default-stream run{detail}"


def run_protocol(cid, case, syncs):
    side = side_stream()
    X, ref, enq = reference(case)
    ms = max(MIN_GATE_MS, MARGIN * enq)
    STATS["cases"] += 1
    if enq > STATS["slowest"][1]:
        STATS["slowest"] = (cid, enq, ms)
    STATS["shortest_gate"] = ms if STATS["shortest_gate"] is None else min(ms, STATS["shortest_gate"])
    g = gate()
    # 2. the decoy, on the side stream
    with torch.cuda.stream(side):
        state = case.setup()
        i, o = clone_all(case.inputs(gen(2000), 1)), case.outputs()
        decoy = case.call(state, i, o, 1)
    torch.cuda.synchronize()
    tensors = [k for k, v in ref.items() if isinstance(v, torch.Tensor)]
    assert any(not same_bits(decoy[k], ref[k]) for k in tensors), "the decoy computed the reference's bits: it hides nothing"
    # 3. poison
    with torch.cuda.stream(side):
        for v in list(i.values()) + list(o.values()) + [v for v in decoy.values() if isinstance(v, torch.Tensor)]:
            if v.is_floating_point():
                v.fill_(NAN)
        del decoy
    torch.cuda.synchronize()
    # 4. the gated phase
    with torch.cuda.stream(side):
        g(ms)
        ev = torch.cuda.Event()
        ev.record(side)
        for k in i:
            i[k].copy_(X[k], non_blocking=True)
        busy_before = not ev.query()
        outs = case.call(state, i, o, 0)
        busy_after = not ev.query()
        got = keep(outs)
    if syncs:
        assert busy_before, f"gate too short: the {ms:.1f} ms gate had ended before the call (which synchronises) was made"
    else:
        assert busy_after, (f"gate too short: the {ms:.1f} ms gate had ended when the call returned "
                            f"(reference enqueue {enq:.3f} ms); the entry synchronises, or the gate must be longer")
    # 5.
    side.synchronize()
    assert_equal(got, ref, cid)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- models
@functools.lru_cache(maxsize=None)
def shape_model(name):
    from gesturediffusion_amd.utils.init import init_state_dict
    arch, d, heads, ff, T, _ = SC.FORWARD_SHAPES[name]
    cfg = dict(arch=arch, njoints=16, nfeats=1, latent_dim=d, ff_size=ff, num_layers=2, num_heads=heads, seed_poses=10)
    return build_model(arch, cfg, init_state_dict(cfg, seed=5, perturb=True)), T


@functools.lru_cache(maxsize=None)
def text_model():
    import text_restatement as tr
    cfg, sd = tr.case(load_golden("forward_text_tiny.npz"), "mdm_128_t64")[:2]
    return tr.build_text_model(cfg, sd).to(dev()), 20


@functools.lru_cache(maxsize=None)
def tiny_model(arch):
    return build_model(arch, TINY, weights_from(load_golden(f"loops_{arch}_tiny.npz")))


def model_tensors(m):
    return {k: v.detach() for k, v in {**m._engine_tensors(), **m._extra_engine_tensors(dev())}.items()}


def new_engine(m, dtype, weights=True):
    """A fresh handle of the module's configuration, its weights set on the current stream."""
    td, cd = m._text_dims()
    eng = E.Engine(m._arch, m.input_feats, m.latent_dim, m.ff_size, m.num_layers, m.num_heads, m.seed_poses,
                   cl_head=getattr(m, "cl_head", 8), window=10, compute_dtype=dtype, text_dim=td, clip_dim=cd)
    if weights:
        eng.load_tensors(model_tensors(m))
    return eng


def forward_into(eng, x, t, mode, scale, out):
    _lib.check(eng.lib.gdx_forward(eng.handle, vp(x), vp(t), mode, vp(scale), vp(out), cur()), eng.lib)
    return out


def cond_inputs(g, m, T, which, x=True):
    """x, the conditioning, valid timesteps and scales of a forward or a loop."""
    J = m.input_feats
    i = dict(seed=rn(g, B, J, 1, m.seed_poses), mfcc=rn(g, B, 26, 1, T), scale=rn(g, B) + 1.5)
    if x:
        i["x"] = rn(g, B, J, 1, T)
    if m._text_dims()[0]:
        i["text"] = rn(g, B, m._text_dims()[1])
    return i


# ----------------------------------------------------------------------------------------------------------------- forwards
def build_forward(shape, dtype, what):
    """gdx_set_condition / gdx_set_condition_text + gdx_forward on a fresh handle.  Launchers by shape (stream_cases.
    FORWARD_SHAPES): old128 launch_token0 with pe, the row-mapped input GEMM, launch_attention3 (fp32) / launch_attentionh, both
    LayerNorm launchers; v2_512 / v2_256 / v2_384 launch_small_linear for W_coa, the V2 GEMMs and the three local-attention front
    ends (16-bit, fp32 MFMA, fp32 with a 16-bit copy, scalar); d96 launch_gemm (gemm.hip); old128_T260 launch_attention (S > 256).
    Every one: launch_gather_rows, the timestep MLP, launch_transpose_in(_f16), launch_transpose_out; cfg launch_cfg_blend;
    +rescale the three launches of gdx_cfg_rescale instead of it; +taps the tap copies, launch_convert_f32 and gdx_get_tap;
    text64 the text slice of the conditioning."""
    mode_name, _, extra = what.partition("+")
    m, T = text_model() if shape == SC.TEXT else shape_model(shape)
    mode, L, d = MODE[mode_name], m.num_layers, m.latent_dim
    beff = 2 * B if mode == E.GDX_CFG else B

    def setup():
        eng = new_engine(m, dtype)
        eng.prepare(B, T)
        if extra == "taps":
            eng.keep_taps(True)
        if extra == "rescale":
            eng.set_guidance_rescale(0.7)
        return eng

    def inputs(g, which):
        i = cond_inputs(g, m, T, which)
        i["t"] = torch.tensor([[3, 500, 999], [871, 40, 260]][which], device=dev())      # valid in both runs
        return i

    def outputs():
        return {"out": nans(B, m.input_feats, 1, T)}

    def call(eng, i, o, which):
        eng.set_condition(i["seed"], i["mfcc"], text=i.get("text"), cache=False)
        outs = {"out": forward_into(eng, i["x"], i["t"], mode, i["scale"] if mode == E.GDX_CFG else None, o["out"])}
        if extra == "taps":
            for l in range(L + 2):
                outs[f"tap{l}"] = eng.tap(l, beff * (T + 1 if l <= L else T), d, dev())
        return outs
    return Case(setup, inputs, call, outputs)


# ------------------------------------------------------------------------------------------------------------------ weights
def build_weights(kind, arch, dtype):
    """set: gdx_set_weight over the whole state dict inside the gated phase (the three pack kernels of weights.hip, the
    hipMemsetAsync of the padded vectors), then a forward.  packed: gdx_export_packed of a loaded handle, gdx_import_packed into
    a second one, then a forward on it.  The decoy's weights are another draw, so an upload that ran early leaves them behind."""
    from gesturediffusion_amd.utils.init import init_state_dict
    m = tiny_model(arch)
    T = 20
    base = model_tensors(m)

    def draw(which):                     # the model's tensors, the decoy's perturbed: same names and shapes
        if not which:
            return {k: v.clone() for k, v in base.items()}
        sd = init_state_dict(dict(TINY, arch=arch), seed=77, perturb=True)
        return {k: (sd[k].to(dev()) if k in sd else v.clone()) for k, v in base.items()}

    def setup():
        if kind == "set":
            eng = new_engine(m, dtype, weights=False)
            eng.load_tensors(draw(1))    # a complete model of other values; the call sets every tensor again
            eng.prepare(B, T)
            return eng
        src = []
        for which in (0, 1):
            e = new_engine(m, dtype, weights=False)
            e.load_tensors(draw(which))
            src.append(e)
        dst = new_engine(m, dtype, weights=False)
        dst.load_tensors(draw(1))        # so that gdx_prepare finds a complete model; the import replaces it
        dst.prepare(B, T)
        return src, dst

    def inputs(g, which):
        i = cond_inputs(g, m, T, which)
        i["t"] = torch.tensor([[3, 500, 999], [871, 40, 260]][which], device=dev())
        if kind == "set":
            i.update({"w." + k: v for k, v in draw(which).items()})
        return i

    def outputs():
        return {"out": nans(B, m.input_feats, 1, T)}

    def call(st, i, o, which):
        if kind == "set":
            eng = st
            eng.load_tensors({k[2:]: v for k, v in i.items() if k.startswith("w.")})
        else:
            src, eng = st
            eng.import_packed(src[which].export_packed(dev()), dev())
        eng.set_condition(i["seed"], i["mfcc"], cache=False)
        return {"out": forward_into(eng, i["x"], i["t"], E.GDX_CFG, i["scale"], o["out"])}
    return Case(setup, inputs, call, outputs)


# ------------------------------------------------------------------------------------------------------ pose-layout kernels
@functools.lru_cache(maxsize=None)
def df_ddim():
    return diffusion("cosine", "ddim10")


@functools.lru_cache(maxsize=None)
def df_dpm():
    return diffusion("linear", "logsnr10")


def build_pose(name, variant, sh):
    """One stand-alone launch (three for gdx_cfg_rescale, two for gdx_window_sweep and gdx_bpd_terms) on [3, J, 1, T]; "v": J 16,
    T 20, aligned operands, the 128-bit instantiation; "s": J 37, T 23, the scalar one.  They are separate launch lines."""
    d = dev()
    J, T = (SC.POSTPROCESS_SHAPES if name == "postprocess" else SC.POSE_SHAPES)[sh]
    shp = (B, J, 1, T)
    df = df_ddim()
    pose = lambda g: rn(g, *shp)                                   # noqa: E731
    guided = lambda g: dict(x=pose(g), oc=pose(g), ou=pose(g), scale=rn(g, B) + 1.5)     # noqa: E731
    masked = lambda g: dict(mask=(torch.rand(shp, generator=g) < 0.3).to(d), motion=0.5 * pose(g))     # noqa: E731
    tsteps = lambda which: torch.tensor([[2, 5, 8], [7, 3, 4]][which], device=d)          # noqa: E731
    buf = lambda *names: (lambda: {n: nans(*shp) for n in names})  # noqa: E731
    cfgkw = lambda i: dict(x0_uncond=i["ou"], scale=i["scale"])    # noqa: E731
    maskkw = lambda i: dict(inpaint_mask=i["mask"], inpaint_motion=i["motion"])           # noqa: E731
    outputs = None

    if name == "sampler_update" and variant == "p_cfg_mask_clip":
        coef = df.coef_table(P, d, 0.0)
        inputs = lambda g, w: {**guided(g), **masked(g)}           # noqa: E731
        outputs = buf("out", "pred")
        call = lambda st, i, o, w: {"out": E.sampler_update(P, coef, i["x"], i["oc"], o["out"], step_index=4, **cfgkw(i), **maskkw(i),   # noqa: E731
                                                           philox_seed=99 + w, sample_offset=2, rng_step=3, pred_xstart=o["pred"],
                                                           clip_denoised=True), "pred": o["pred"]}
    elif name == "sampler_update":
        coef, cc = df.coef_table(DDIM, d, 0.5), df._cond_coef(d)
        inputs = lambda g, w: dict(x=pose(g), oc=pose(g), noise=pose(g), grad=pose(g), t=tsteps(w))    # noqa: E731
        outputs = buf("out", "pred")
        call = lambda st, i, o, w: {"out": E.sampler_update(DDIM, coef, i["x"], i["oc"], o["out"], t=i["t"], noise=i["noise"],   # noqa: E731
                                                           pred_xstart=o["pred"], cond_grad=i["grad"], cond_coef=cc), "pred": o["pred"]}
    elif name == "plms_update":
        kind = int(variant[4:])
        coef, cc = df.coef_table(DDIM, d, 0.0), df._cond_coef(d)
        inputs = lambda g, w: dict(x=pose(g), pred=pose(g), e0=pose(g), t=tsteps(w))      # noqa: E731
        outputs = buf("out")
        call = lambda st, i, o, w: {"out": E.plms_update(kind, coef, i["t"], i["x"], i["pred"],   # noqa: E731
                                                        eps=(i["e0"], cc) if kind == 7 else (i["e0"],), out=o["out"])}
    elif name == "plms_step":
        kind = int(variant[4:])
        coef = df.coef_table(DDIM, d, 0.0)
        nh = {1: 0, 2: 1, 3: 2, 4: 3, 5: 1, 6: 0}[kind]
        inputs = lambda g, w: {**guided(g), **masked(g), "x_eps": pose(g), "pred_prev": pose(g),   # noqa: E731
                               **{f"h{j}": pose(g) for j in range(nh)}}
        outputs = buf("out", "eps", "pred")
        call = lambda st, i, o, w: {"out": E.plms_step(   # noqa: E731
            kind, coef, i["x"], i["oc"], o["out"], eps_out=o["eps"], eps_hist=[i[f"h{j}"] for j in range(nh)], step_index=5, **cfgkw(i),
            **maskkw(i), clip_denoised=kind % 2 == 0, pred_xstart=o["pred"], x_eps=i["x_eps"] if kind == 5 else None,
            step_index_eps=4, pred_prev=i["pred_prev"] if kind == 5 else None), "eps": o["eps"], "pred": o["pred"]}
    elif name in ("dpm_step", "dpm_sde_step"):
        sde = name == "dpm_sde_step"
        order = {"order1": 1, "order2": 2, "order3": 3, "tape": 2, "philox": 1}[variant]
        coef = df_dpm().dpm_sde_coef_table(d, 1.0) if sde else df_dpm().dpm_coef_table(d)
        inputs = lambda g, w: {**guided(g), **masked(g), "noise": pose(g), "t": tsteps(w), **{f"h{j}": pose(g) for j in range(order - 1)}}   # noqa: E731
        outputs = buf("out", "pred")

        def call(st, i, o, w):
            kw = dict(hist=[i[f"h{j}"] for j in range(order - 1)], t=i["t"], **cfgkw(i), **maskkw(i), clip_denoised=True, pred_out=o["pred"])
            if sde:
                E.dpm_sde_step(order, coef, i["x"], i["oc"], o["out"], noise=i["noise"] if variant == "tape" else None,
                               philox_seed=31 + w, sample_offset=4, rng_step=6, **kw)
            else:
                E.dpm_step(order, coef, i["x"], i["oc"], o["out"], **kw)
            return dict(o)
    elif name == "unipc_step":
        coef, coef_c = df_dpm().unipc_coef_tables(d)
        qc, qp = (0, 1) if variant == "predictor" else (2, 2)
        inputs = lambda g, w: {**guided(g), "h0": pose(g), "h1": pose(g)}    # noqa: E731
        outputs = buf("out", "base", "pred")
        call = lambda st, i, o, w: (E.unipc_step(qc, qp, coef, coef_c, i["x"], i["oc"], o["out"], o["base"], hist=[i["h0"], i["h1"]][:qc],   # noqa: E731
                                                 step_index=5, **cfgkw(i), pred_out=o["pred"]), dict(o))[1]
    elif name == "ddim_reverse_step":
        coef = df.coef_table(DDIM, d, "reverse")
        inputs = lambda g, w: {**guided(g), **masked(g), "t": tsteps(w)}     # noqa: E731
        outputs = buf("out", "pred", "eps")
        call = lambda st, i, o, w: (E.ddim_reverse_step(coef, i["x"], i["oc"], o["out"], t=i["t"], **cfgkw(i), **maskkw(i),   # noqa: E731
                                                        pred_out=o["pred"], eps_out=o["eps"]), dict(o))[1]
    elif name in ("q_sample", "q_sample_t"):
        coef = df.coef_table(P, d, 0.0)
        inputs = lambda g, w: dict(x=pose(g), noise=pose(g), t=tsteps(w))    # noqa: E731
        call = lambda st, i, o, w: {"out": E.q_sample(i["x"], i["noise"], coef, 4) if name == "q_sample"   # noqa: E731
                                    else E.q_sample_t(i["x"], i["noise"], coef, i["t"])}
    elif name == "masked_l2":
        inputs = lambda g, w: dict(a=pose(g), b=pose(g), mask=(torch.arange(T) < [T - 3, T // 2][w]).view(1, 1, 1, T).repeat(B, 1, 1, 1).to(d))   # noqa: E731
        call = lambda st, i, o, w: {"out": E.masked_l2(i["a"], i["b"], i["mask"])}     # noqa: E731
    elif name == "randn":
        inputs = lambda g, w: {}                                   # noqa: E731
        call = lambda st, i, o, w: {"out": E.randn(shp, d, 1234 + w, sample_offset=3, rng_step=2)}   # noqa: E731
    elif name == "postprocess":
        inputs = lambda g, w: dict(x=pose(g), mean=rn(g, J, dtype=torch.float64), std=rn(g, J, dtype=torch.float64).abs() + 0.5)   # noqa: E731
        call = lambda st, i, o, w: dict(zip(("pos", "rot"), E.postprocess(i["x"], i["mean"], i["std"])))   # noqa: E731
    elif name == "cfg_rescale":
        me = types.SimpleNamespace(lib=_lib.load())
        inputs = lambda g, w: dict(c=pose(g), u=pose(g), scale=rn(g, B) + 1.5, t=torch.tensor([[100, 500, 600], [300, 900, 700]][w], device=d))   # noqa: E731
        outputs = buf("out")
        call = lambda st, i, o, w: dict(zip(("out", "factor"), E.Engine.cfg_rescale(   # noqa: E731
            me, i["c"], i["u"], i["scale"], 0.7, t=i["t"], interval=MID, out=o["out"])))
    elif name == "cfg_delta":
        inputs = lambda g, w: dict(a=pose(g), b=pose(g))           # noqa: E731
        outputs = buf("out")
        call = lambda st, i, o, w: {"out": E.cfg_delta(i["a"], i["b"], out=o["out"])}   # noqa: E731
    elif name == "bpd_terms":
        coef = df.bpd_table(d)
        step = {"prior": 9, "middle": 5, "step0": 0}[variant]
        inputs = lambda g, w: {**guided(g), "x_start": 0.5 * pose(g), "noise": pose(g)}   # noqa: E731

        def call(st, i, o, w):
            if variant == "prior":
                return {"prior": E.bpd_prior(coef, i["x_start"], step, df._prior_log_variance())}
            vb, xm, mse, pred = E.bpd_terms(coef, i["x_start"], i["x"], i["oc"], noise=i["noise"], step_index=step, **cfgkw(i))
            return dict(vb=vb, xstart_mse=xm, mse=mse, pred=pred)
    elif name == "window_sweep":
        coef = df.coef_table(P, d, 0.0)
        inputs = lambda g, w: {**masked(g), "planes": rn(g, 4, *shp), "x0": 1.5 * rn(g, 3, *shp)}     # noqa: E731
        call = lambda st, i, o, w: {"err": E.window_sweep(P, coef, 6, i["planes"], i["x0"], **maskkw(i), clip_denoised=True,   # noqa: E731
                                                          philox_seed=55 + w, sample_offset=1, rng_step=3), "planes": i["planes"]}
    elif name == "layer_delta":
        op, dt = variant.split("_")
        tin, tout = {"fp32": (torch.float32,) * 2, "fp16": (torch.float16,) * 2, "bf16": (torch.float32, torch.bfloat16)}[dt]
        Tn, w_ = 20, 128
        if op == "store":
            inputs = lambda g, w: dict(inp=rn(g, B, Tn + 1, w_, dtype=tin), outc=rn(g, B, Tn, w_, dtype=tout))      # noqa: E731
            outputs = lambda: {"delta": nans(B, Tn, w_)}           # noqa: E731
            call = lambda st, i, o, w: {"delta": E.layer_delta(0, i["inp"], i["outc"], o["delta"])}     # noqa: E731
        else:
            inputs = lambda g, w: dict(inp=rn(g, B, Tn + 1, w_, dtype=tin), delta=rn(g, B, Tn, w_))     # noqa: E731
            outputs = lambda: {"outc": nans(B, Tn, w_, dtype=tout)}     # noqa: E731
            call = lambda st, i, o, w: {"outc": E.layer_delta(1, i["inp"], o["outc"], i["delta"])}      # noqa: E731
    else:
        raise KeyError(name)
    return Case(lambda: None, inputs, call, outputs)


# -------------------------------------------------------------------------------------------------------------------- loops
def build_loop(entry, variant, arch, dtype):
    """An in-library loop of ten steps on a fresh handle: gdx_set_condition and the loop inside the gated phase.  T = 20 (12 for
    MDM_Old) without inpainting takes gdx_sample_loop's token-major path, T = 10 the pose-layout one; every other loop is
    pose-layout only."""
    d = dev()
    m = tiny_model(arch)
    tm_T = 20 if arch == "mdm" else 12
    pose_T = 10
    df = df_dpm() if entry in ("dpm", "dpm_sde", "unipc") else df_ddim()
    tmap, n = df._timestep_map(), df.num_timesteps
    assert n == 10
    T = pose_T
    if (entry, variant) in (("sample", "token_major"), ("sample", "layer_cache_tm"), ("sample", "refresh"), ("sample", "rescale")) \
            or entry in ("plms", "dpm", "unipc", "bpd"):
        T = tm_T
    window = 4 if entry == "parallel" else 1
    shp = (B, 16, 1, T)

    def setup():
        eng = new_engine(m, dtype)
        eng.prepare(window * B, T)
        if variant == "interval":
            eng.set_guidance_interval(MID)
        if variant == "rescale":
            eng.set_guidance_rescale(0.7)
        if variant == "graph_replay":
            eng.set_graph_replay(True)
        return eng

    def inputs(g, which):
        i = cond_inputs(g, m, T, which)
        i["x"] = rn(g, *shp)
        if variant in ("inpaint_dump", "graph_replay", "tape"):
            i["tape"] = rn(g, n, *shp)
        if variant == "inpaint_dump":
            i.update(mask=(torch.rand(shp, generator=g) < 0.3).to(d), motion=0.5 * rn(g, *shp))
        if entry in ("plms", "dpm", "dpm_sde", "unipc"):
            i["hist"] = torch.zeros(3, *shp, device=d)
            i["aux"] = torch.zeros(shp, device=d)
        return i

    def outputs():
        if variant == "inpaint_dump":
            return {"dump": nans(3, *shp)}
        if entry == "bpd":
            return {k: nans(B, n) for k in ("vb", "xstart_mse", "mse")} | {"prior": nans(B)}
        return {}

    def call(eng, i, o, which):
        rep = lambda t: t.repeat(window, *([1] * (t.dim() - 1)))   # noqa: E731  (window-major, Engine.prepare_window)
        eng.set_condition(rep(i["seed"]), rep(i["mfcc"]), cache=False)
        eng.set_guidance_refresh(2 if variant == "refresh" else 1)           # host side; clears what an earlier loop stored
        eng.set_layer_cache(*((2, 1) if variant.startswith("layer_cache") else (1, 0)))
        x, kw, seed = i["x"], dict(scale=i["scale"]), 7 + which
        if entry == "sample" and variant == "inpaint_dump":
            eng.sample_loop(x, P, E.GDX_CFG, df.coef_table(P, d, 0.0), tmap, n - 1, inpaint_mask=i["mask"], inpaint_motion=i["motion"],
                            noise_tape=i["tape"], dump=o["dump"], dump_steps=[0, 3, 9], **kw)     # the DDIM kind takes no dump
            return {"x": x, "dump": o["dump"]}
        if entry == "sample" and variant == "graph_replay":
            eng.sample_loop(x, DDIM, E.GDX_CFG, df.coef_table(DDIM, d, 0.5), tmap, n - 1, noise_tape=i["tape"], **kw)
        elif entry == "sample":
            eng.sample_loop(x, P, E.GDX_CFG, df.coef_table(P, d, 0.0), tmap, n - 1, philox_seed=seed, sample_offset=which, **kw)
        elif entry == "plms":
            eng.plms_loop(x, E.GDX_CFG, 2, df.coef_table(DDIM, d, 0.0), tmap, n - 1, i["hist"], i["aux"], **kw)
        elif entry == "dpm":
            eng.dpm_loop(x, E.GDX_CFG, 2, df.dpm_coef_table(d), tmap, n - 1, i["hist"], **kw)
        elif entry == "dpm_sde":
            eng.dpm_sde_loop(x, E.GDX_CFG, 2, df.dpm_sde_coef_table(d, 1.0), tmap, n - 1, i["hist"], noise_tape=i.get("tape"),
                             philox_seed=seed, **kw)
        elif entry == "unipc":
            coef, coef_c = df.unipc_coef_tables(d)
            eng.unipc_loop(x, E.GDX_CFG, 2, coef, coef_c, tmap, n - 1, i["hist"], i["aux"], **kw)
        elif entry == "ddim_reverse":
            eng.ddim_reverse_loop(x, E.GDX_CFG, df.coef_table(DDIM, d, "reverse"), tmap, 0, n, **kw)
        elif entry == "bpd":
            eng.bpd_loop(x, E.GDX_CFG, df.bpd_table(d), tmap, o["vb"], o["xstart_mse"], o["mse"], philox_seed=seed,
                         prior_bpd=o["prior"], prior_log_variance=df._prior_log_variance(), **kw)
            return dict(o)
        elif entry == "parallel":
            planes = x.unsqueeze(0).repeat(window + 1, 1, 1, 1, 1)
            thr = df.parallel_threshold(0.0 if variant == "tol0" else 1e-2)
            anchor, strides = eng.parallel_loop(planes, P, E.GDX_CFG, df.coef_table(P, d, 0.0), tmap, thr, n - 1, philox_seed=seed, **kw)
            assert anchor == n
            return {"planes": planes, "iterations": len(strides), "strides": tuple(strides)}
        outs = {"x": x}
        if "hist" in i:
            outs.update(hist=i["hist"], aux=i["aux"])
        return outs
    return Case(setup, inputs, call, outputs)


def build_torch_tape(arch, dtype):
    """p_sample_loop(rng="torch"): the noise of a gdx_sample_loop block is drawn by torch's generator on the current stream into a
    tape the kernels read.  A fresh module per handle (the module owns its engine)."""
    T = 20
    shp = (B, 16, 1, T)

    def setup():
        from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
        m = build_model(arch, TINY, weights_from(load_golden(f"loops_{arch}_tiny.npz")))
        m.compute_dtype = dtype
        return ClassifierFreeSampleModel(m)

    def call(model, i, o, which):
        torch.manual_seed(5 + which)
        y = {"seed": i["seed"], "mfcc": i["mfcc"], "scale": i["scale"]}
        return {"x": df_ddim().p_sample_loop(model, shp, clip_denoised=False, model_kwargs={"y": y}, rng="torch")}
    return Case(setup, lambda g, w: cond_inputs(g, tiny_model(arch), T, w, x=False), call)


def build_guards(arch, dtype):
    """gdx_check_guards after a forward on a guarded workspace: it synchronises the stream and reads the canaries back."""
    m, T = tiny_model(arch), 20

    def setup():
        eng = new_engine(m, dtype)
        eng.set_guards(True)
        eng.prepare(B, T)
        return eng

    def inputs(g, which):
        return {**cond_inputs(g, m, T, which), "t": torch.tensor([[3, 500, 999], [871, 40, 260]][which], device=dev())}

    def call(eng, i, o, which):
        eng.set_condition(i["seed"], i["mfcc"], cache=False)
        forward_into(eng, i["x"], i["t"], E.GDX_CFG, i["scale"], o["out"])
        bad, first = eng.check_guards(dev())
        return {"out": o["out"], "bad_bytes": bad, "first_bad_zone": first}
    return Case(setup, inputs, call, lambda: {"out": nans(B, 16, 1, T)})


def build_mfcc(n):
    """gdx_mfcc on n samples (shorter than one frame): framing, the DFT and mel GEMMs, the cepstrum kernel."""
    from gesturediffusion_amd.data_loaders.mfcc import MfccExtractor
    rng = np.random.default_rng(n)
    mean, std = rng.normal(size=26), rng.uniform(0.5, 3.0, size=26)
    return Case(lambda: MfccExtractor(dev(), mfcc_mean=mean, mfcc_std=std), lambda g, w: {"signal": 0.3 * rn(g, n)},
                lambda ex, i, o, w: {"mfcc": ex(i["signal"])})


# -------------------------------------------------------------------------------------------------------- test entry points
def build_entry(name):
    """One small call of a test entry point of csrc/testapi.hip: its Scratch helpers stage, convert and copy back on the caller's
    stream, and every one of them synchronises it."""
    lib = _lib.load()
    d = dev()

    def run(fn, *args):
        _lib.check(fn(*args, cur()), lib)

    if name in ("linear_full", "linear_half"):
        M, N, K = 70, 128, 64
        inputs = lambda g, w: dict(A=rn(g, M, K), W=rn(g, N, K) / 8, bias=rn(g, N))      # noqa: E731
        if name == "linear_full":
            outputs = lambda: {"C": nans(M, N)}                   # noqa: E731
            call = lambda st, i, o, w: (run(lib.gdx_linear_full, vp(i["A"]), vp(i["W"]), vp(i["bias"]), None, 0, None, 0, vp(o["C"]), M,   # noqa: E731
                                            M, N, K, 1, 0, 1, 0, 0, 0, 0, None), dict(o))[1]
        else:
            outputs = lambda: {"C32": nans(M, N), "C16": nans(M, N)}     # noqa: E731
            call = lambda st, i, o, w: (run(lib.gdx_linear_half, vp(i["A"]), vp(i["W"]), vp(i["bias"]), None, 0, None, 0, vp(o["C32"]),   # noqa: E731
                                            vp(o["C16"]), M, M, N, K, 1, 0, 1, F16, 0, 0, None), dict(o))[1]
    elif name == "layernorm":
        R, w_ = 50, 128
        inputs = lambda g, w: dict(x=rn(g, R, w_), res=rn(g, R, w_), gamma=rn(g, w_), beta=rn(g, w_))   # noqa: E731
        outputs = lambda: {"out32": nans(R, w_), "out16": nans(R, w_)}   # noqa: E731
        call = lambda st, i, o, w: (run(lib.gdx_layernorm, vp(i["x"]), vp(i["res"]), vp(i["gamma"]), vp(i["beta"]), vp(o["out32"]),   # noqa: E731
                                        vp(o["out16"]), R, R, w_, 0, 0, BF16), dict(o))[1]
    elif name == "local_attention":
        Bn, T, w_, heads, win = 2, 20, 256, 8, 10
        rows = Bn * (T + 1)
        inputs = lambda g, w: dict(x=rn(g, Bn, T, w_), cos=torch.cos(rn(g, T + 1, w_ // heads // 2)), sin=torch.sin(rn(g, T + 1, w_ // heads // 2)))   # noqa: E731
        outputs = lambda: {"enc": nans(rows, w_)}                 # noqa: E731
        call = lambda st, i, o, w: (run(lib.gdx_local_attention, vp(i["x"]), vp(i["cos"]), vp(i["sin"]), vp(o["enc"]), None, rows, Bn, T,   # noqa: E731
                                        w_, heads, win, F32, None), dict(o))[1]
    elif name == "transpose_in":
        inputs = lambda g, w: dict(x=rn(g, 2, 16, 20))            # noqa: E731
        outputs = lambda: {"xt": nans(80, 32)}                    # noqa: E731
        call = lambda st, i, o, w: (run(lib.gdx_transpose_in, vp(i["x"]), vp(o["xt"]), 80, 4, 2, 16, 20, 32, F16), dict(o))[1]   # noqa: E731
    elif name == "transpose_out":
        inputs = lambda g, w: dict(yt=rn(g, 60, 32))              # noqa: E731
        outputs = lambda: {"y": nans(48, 20)}                     # noqa: E731
        call = lambda st, i, o, w: (run(lib.gdx_transpose_out, vp(i["yt"]), vp(o["y"]), 48, 3, 16, 20, 32), dict(o))[1]   # noqa: E731
    elif name == "small_linear":
        inputs = lambda g, w: dict(A=rn(g, 5, 64), W=rn(g, 96, 64) / 8, bias=rn(g, 96))  # noqa: E731
        outputs = lambda: {"out": nans(5, 96)}                    # noqa: E731
        call = lambda st, i, o, w: (run(lib.gdx_small_linear, vp(i["A"]), 64, vp(i["W"]), 64, vp(i["bias"]), vp(o["out"]), 5, 96, 5, 96, 64, 1),   # noqa: E731
                                    dict(o))[1]
    elif name == "gather_rows":
        inputs = lambda g, w: dict(table=rn(g, 50, 128), idx=ri(gen(40 + w), 0, 50, 7))  # noqa: E731
        outputs = lambda: {"out": nans(7, 128)}                   # noqa: E731
        call = lambda st, i, o, w: (run(lib.gdx_gather_rows, vp(i["table"]), vp(i["idx"]), vp(o["out"]), 7, 7, 128, 50), dict(o))[1]   # noqa: E731
    elif name == "mfcc_project":
        inputs = lambda g, w: dict(mfcc=rn(g, 2, 26, 20), W=rn(g, 128, 32) / 5, bias=rn(g, 128), pe=rn(g, 21, 128))   # noqa: E731
        outputs = lambda: {"out": nans(84, 128)}                  # noqa: E731
        call = lambda st, i, o, w: (run(lib.gdx_mfcc_project, vp(i["mfcc"]), vp(i["W"]), 32, vp(i["bias"]), vp(i["pe"]), vp(o["out"]), 84,   # noqa: E731
                                        4, 2, 26, 20, 128, 21, 1), dict(o))[1]
    elif name == "token0":
        inputs = lambda g, w: dict(temb=rn(g, 2, 128), seed=rn(g, 4, 128), pe0=rn(g, 128))     # noqa: E731
        outputs = lambda: {"enc": nans(64, 128), "enc16": nans(64, 128)}     # noqa: E731
        call = lambda st, i, o, w: (run(lib.gdx_token0, vp(i["temb"]), 128, vp(i["seed"]), vp(i["pe0"]), vp(o["enc"]), vp(o["enc16"]), 64,   # noqa: E731
                                        None, None, None, 0, None, 4, 2, 21, 128, F16), dict(o))[1]
    elif name in ("attention_half", "attention_f32_rows", "attention_f16", "attention_f32"):
        Bn, S, w_ = 2, 21, 128
        H = 2 if name == "attention_f32_rows" else 4               # head width 64: attention3.hip; 32: attention.hip / attentionh
        pad = 64 if name in ("attention_half", "attention_f32_rows") else 0
        inputs = lambda g, w: dict(qkv=rn(g, Bn * S + pad, 3 * w_))   # noqa: E731
        outputs = lambda: {"ctx": nans(Bn * S, w_)}               # noqa: E731
        if name == "attention_half":
            call = lambda st, i, o, w: (run(lib.gdx_attention_half, vp(i["qkv"]), Bn * S + pad, vp(o["ctx"]), Bn * S, Bn, S, H, w_, F16, 0,   # noqa: E731
                                            0, None), dict(o))[1]
        elif name == "attention_f32_rows":
            call = lambda st, i, o, w: (run(lib.gdx_attention_f32_rows, vp(i["qkv"]), Bn * S + pad, vp(o["ctx"]), Bn * S, Bn, S, H, w_, 0,   # noqa: E731
                                            0, None), dict(o))[1]
        elif name == "attention_f16":
            call = lambda st, i, o, w: (run(lib.gdx_attention_f16, vp(i["qkv"]), vp(o["ctx"]), Bn, S, H, w_), dict(o))[1]   # noqa: E731
        else:
            call = lambda st, i, o, w: (run(lib.gdx_attention_f32, vp(i["qkv"]), vp(o["ctx"]), Bn, S, H, w_, 0), dict(o))[1]   # noqa: E731
    else:
        raise KeyError(name)
    return Case(lambda: None, inputs, call, outputs)


# -------------------------------------------------------------------------------------------------------- the Python protocol
def build_python(what, arch):
    """p_sample_loop(fused=False): the step-wise callable protocol, model(x, t, y) + one gdx_sampler_update per step, through
    the drop-in module's own engine.  sample_chunks: two chunks of a guided ten-step loop, the second seeded on the device with
    the first one's last frames."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    T = 20 if arch == "mdm" else 12
    shp = (B, 16, 1, T)

    def setup():
        m = build_model(arch, TINY, weights_from(load_golden(f"loops_{arch}_tiny.npz")))
        return ClassifierFreeSampleModel(m)

    if what == "p_sample_loop_stepwise":
        def inputs(g, which):
            return {**cond_inputs(g, tiny_model(arch), T, which, x=False), "tape": rn(g, 11, *shp)}

        def call(model, i, o, which):
            y = {"seed": i["seed"], "mfcc": i["mfcc"], "scale": i["scale"]}
            return {"x": df_ddim().p_sample_loop(model, shp, clip_denoised=False, model_kwargs={"y": y}, noise_tape=i["tape"], fused=False)}
    else:
        from gesturediffusion_amd.sample.generate import sample_chunks

        def inputs(g, which):
            return dict(seed=rn(g, B, 16, 1, 10), mfcc0=rn(g, B, 26, 1, T), mfcc1=rn(g, B, 26, 1, T))

        def call(model, i, o, which):
            outs = sample_chunks(model, df_ddim(), i["seed"], lambda c: i[f"mfcc{c}"], 2, T, 10, guidance_param=2.5, sampler="ddim",
                                 eta=0.5, rng="philox", philox_seed=21 + which)
            return {f"chunk{c}": x for c, x in enumerate(outs)}
    return Case(setup, inputs, call)


# ----------------------------------------------------------------------------------------------------------------- the cases
def build(cid):
    fam, *p = cid.split("/")
    if fam == "fwd":
        return build_forward(*p)
    if fam == "weights":
        return build_weights(*p)
    if fam == "pose":
        return build_pose(*p)
    if fam == "loop" and p[:2] == ["sample", "torch_tape"]:
        return build_torch_tape(*p[2:])
    if fam == "loop":
        return build_loop(*p)
    if fam == "guards":
        return build_guards(*p[1:])
    if fam == "mfcc":
        return build_mfcc(int(p[0][1:]))
    if fam == "entry":
        return build_entry(p[0])
    if fam == "python":
        return build_python(*p)
    raise KeyError(cid)


def test_side_stream_is_not_the_default_stream_and_the_gate_holds():
    s = side_stream()
    assert s.cuda_stream != 0 and torch.cuda.current_stream(dev()).cuda_stream == 0
    g = gate()
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream(dev()).cuda_stream == s.cuda_stream
        g(MIN_GATE_MS)
        ev = torch.cuda.Event()
        ev.record(s)
        assert not ev.query(), "the gate's event was signalled as soon as it was recorded"
    s.synchronize()
    assert ev.query()
    print(f"[stream-gate] {g.kind}: {g.note}; {MIN_GATE_MS} ms request -> {g.check_ms:.2f} ms")


@pytest.mark.parametrize("cid", SC.PROTOCOL_CASES)
def test_side_stream_run_has_the_bits_of_the_default_stream_run(cid):
    run_protocol(cid, build(cid), SC.SYNCS[cid])


# --------------------------------------------------------------------------------------------- outside the delayed-input protocol
def _forward_case():
    return build_forward("old128", "fp32", "cfg")


def test_first_prepare_behind_a_busy_default_stream():
    """gdx_prepare fills every workspace buffer with a synchronous hipMemset on the null stream and takes no stream argument.
    Behind a busy default stream either the fill has completed when gdx_prepare returns -- then it simply takes as long as the
    gate -- or it lands later, on top of what gdx_set_condition wrote on the side stream: then the second forward below, made
    after everything has drained, reads a zeroed conditioning and differs."""
    case = _forward_case()
    X, ref, _ = reference(case)
    m, T = shape_model("old128")
    eng = new_engine(m, "fp32")                            # weights set; the first gdx_prepare is still to come
    i, o1, o2 = clone_all(X), case.outputs(), case.outputs()
    torch.cuda.synchronize()
    gate()(MIN_GATE_MS)                                    # on the default stream
    ev = torch.cuda.Event()
    ev.record()
    eng.prepare(B, T)
    print(f"[stream-prepare] the gate was {'still busy' if not ev.query() else 'over'} when the first gdx_prepare returned")
    with torch.cuda.stream(side_stream()):
        first = keep(case.call(eng, i, o1, 0))
    torch.cuda.synchronize()
    with torch.cuda.stream(side_stream()):
        second = keep({"out": forward_into(eng, i["x"], i["t"], E.GDX_CFG, i["scale"], o2["out"])})
    torch.cuda.synchronize()
    assert_equal(first, ref, "the forward enqueued behind the first gdx_prepare")
    assert_equal(second, ref, "a second forward on the same conditioning, after the device had drained")


@pytest.mark.parametrize("cid", ["loop/sample/layer_cache/mdm/fp32", "loop/parallel/tol0/mdm/fp32", "loop/bpd/cfg/mdm/fp32"])
def test_late_allocation_behind_a_busy_default_stream(cid):
    """The first layer-cache call, the first gdx_parallel_loop and the first gdx_bpd_loop of a handle allocate their workspace and
    zero it on the caller's stream (ws_alloc: hipMemsetAsync on the stream of the call that asks), so the stream itself orders the
    fill ahead of the call's first store and nothing waits.  With the default stream busy and the call on a side stream, a fill
    left on the null stream would land late and wipe what the loop had stored."""
    case = build(cid)
    X, ref, _ = reference(case)
    state = case.setup()
    i, o = clone_all(X), case.outputs()
    torch.cuda.synchronize()
    gate()(MIN_GATE_MS)                                    # on the default stream
    with torch.cuda.stream(side_stream()):
        got = keep(case.call(state, i, o, 0))
    torch.cuda.synchronize()
    assert_equal(got, ref, cid)


def test_two_handles_on_two_streams_do_not_disturb_each_other():
    """An fp32 MDM_Old handle and an fp16 MDM handle, each with a guided ten-step loop on its own side stream, issued one step
    at a time alternately from one thread without a host synchronisation: each result has the bits of its solo run on the default
    stream (process-wide state: gemm_init and the thread-local error string)."""
    d = dev()
    df = df_ddim()
    tmap, n = df._timestep_map(), df.num_timesteps
    coef = df.coef_table(P, d, 0.0)
    runs = []
    for k, (arch, dtype, T) in enumerate((("mdm_old", "fp32", 12), ("mdm", "fp16", 20))):
        m = tiny_model(arch)
        X = cond_inputs(gen(300 + k), m, T, 0)
        eng = new_engine(m, dtype)
        eng.prepare(B, T)
        eng.set_condition(X["seed"], X["mfcc"], cache=False)
        solo = X["x"].clone()
        eng.sample_loop(solo, P, E.GDX_CFG, coef, tmap, n - 1, scale=X["scale"], philox_seed=70 + k)
        torch.cuda.synchronize()
        eng2 = new_engine(m, dtype)
        eng2.prepare(B, T)
        runs.append((eng2, X, X["x"].clone(), solo, side_stream(k), k))
    torch.cuda.synchronize()
    for eng, X, x, _, s, k in runs:
        with torch.cuda.stream(s):
            eng.set_condition(X["seed"], X["mfcc"], cache=False)
    for step in range(n):
        for eng, X, x, _, s, k in runs:
            with torch.cuda.stream(s):
                eng.sample_loop(x, P, E.GDX_CFG, coef, tmap, n - 1 - step, scale=X["scale"], philox_seed=70 + k, run_steps=1, k_base=step)
    torch.cuda.synchronize()
    for eng, X, x, solo, s, k in runs:
        assert torch.isfinite(solo).all() and same_bits(x, solo), ("mdm_old fp32", "mdm fp16")[k]
