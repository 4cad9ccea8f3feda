"""The case table of tests/test_gpu_streams.py as plain data, importable without a GPU: which cases run each entry of include/gdx.h
that takes a `stream` on a non-default stream, and which entries synchronise that stream themselves (for those the module checks
that the gate is still busy immediately BEFORE the call, for the others when the call has returned).  tests/test_streams_host.py
holds this table against the header in both directions: an entry with a stream parameter that is added to gdx.h fails there
until it has a case here (or a written reason in EXEMPT).

A case id is "<family>/<parameters>"; the GPU module builds the case from the id alone (its BUILDERS, one per family), and
asserts that every id of this table has a builder and runs.  Shapes: the tiny models of the loop tests (njoints 16, latent_dim
128, ff_size 256, 2 layers, 4 heads, 10 seed poses) at B = 3 unless a shape below says otherwise."""

DTYPES = ("fp32", "fp16", "bf16")
MODES = ("cond", "uncond", "cfg")

# ---- forwards: name -> (arch, latent_dim, heads, ff_size, T, dtypes) and the launchers forward_core reaches only there
FORWARD_SHAPES = {
    "old128": ("mdm_old", 128, 4, 256, 20, DTYPES),      # V1: token0 with pe, the row-mapped input linear, attention3 / attentionh
    "v2_512": ("mdm", 512, 4, 256, 20, DTYPES),          # V2, E = 64: 16-bit front end in the half modes, fp32-MFMA front end in fp32
    "v2_256": ("mdm", 256, 4, 256, 20, DTYPES),          # V2, E = 32: fp32 front end with a 16-bit copy in the half modes
    "v2_384": ("mdm", 384, 4, 256, 20, DTYPES),          # V2, E = 48: the scalar front end; head width 96
    "d96": ("mdm_old", 96, 3, 160, 20, ("fp32",)),       # N = 96 / 288 / 160: csrc/gemm.hip instead of the persistent kernel
    "old128_T260": ("mdm_old", 128, 4, 256, 260, DTYPES),  # S = 261 > 256: the general fp32 attention kernel
}
TEXT = "text64"                                          # tests/golden/forward_text_tiny.npz's mdm_128_t64 configuration, T = 20

FORWARD = [f"fwd/{s}/{dt}/{m}" for s, v in FORWARD_SHAPES.items() for dt in v[5] for m in MODES]
FORWARD_TAPS = [f"fwd/{s}/{dt}/{m}+taps" for s in ("old128", "v2_512") for dt in DTYPES for m in ("cond", "cfg")]
FORWARD_RESCALE = [f"fwd/{s}/{dt}/cfg+rescale" for s in ("old128", "v2_512") for dt in DTYPES]
FORWARD_TEXT = [f"fwd/{TEXT}/{dt}/{m}" for dt in DTYPES for m in MODES]

# ---- weights
WEIGHTS_SET = [f"weights/set/{a}/{dt}" for a in ("mdm", "mdm_old") for dt in DTYPES]
WEIGHTS_PACKED = [f"weights/packed/{a}/{dt}" for a in ("mdm", "mdm_old") for dt in ("fp32", "fp16")]

# ---- pose-layout kernels: "v" = J 16, T 20, aligned operands (the 128-bit instantiation); "s" = J 37, T 23 (the scalar one)
POSE_SHAPES = {"v": (16, 20), "s": (37, 23)}
POSTPROCESS_SHAPES = {"v": (18, 20), "s": (42, 23)}      # gdx_postprocess needs 6 features per joint


def _both(name, variants):
    return [f"pose/{name}/{v}/{s}" for v in variants for s in POSE_SHAPES]


POSE = {
    "gdx_sampler_update": _both("sampler_update", ("p_cfg_mask_clip", "ddim_cond_grad")),
    "gdx_plms_update": _both("plms_update", ("kind0", "kind6", "kind7", "kind8")),
    "gdx_plms_step": _both("plms_step", tuple(f"kind{k}" for k in range(1, 7))),
    "gdx_dpm_step": _both("dpm_step", ("order1", "order2", "order3")),
    "gdx_dpm_sde_step": _both("dpm_sde_step", ("tape", "philox")),
    "gdx_unipc_step": _both("unipc_step", ("predictor", "corrector")),
    "gdx_ddim_reverse_step": _both("ddim_reverse_step", ("cfg",)),
    "gdx_q_sample": _both("q_sample", ("idx",)),
    "gdx_q_sample_t": _both("q_sample_t", ("t",)),
    "gdx_masked_l2": _both("masked_l2", ("prefix",)),
    "gdx_randn": _both("randn", ("draw",)),
    "gdx_postprocess": _both("postprocess", ("split",)),
    "gdx_cfg_rescale": _both("cfg_rescale", ("interval",)),
    "gdx_cfg_delta": _both("cfg_delta", ("sub",)),
    "gdx_bpd_terms": _both("bpd_terms", ("prior", "middle", "step0")),
    "gdx_window_sweep": _both("window_sweep", ("p_philox",)),
    "gdx_layer_delta": [f"pose/layer_delta/{op}_{dt}/v" for op in ("store", "apply") for dt in DTYPES],
}

# ---- loops: ten kept timesteps.  T = 20 (and 12 for MDM_Old) takes gdx_sample_loop's token-major path, T = 10 the pose-layout one
SAMPLE_LOOP = ["loop/sample/token_major/mdm/fp32", "loop/sample/token_major/mdm_old/fp16",
               "loop/sample/inpaint_dump/mdm/fp32", "loop/sample/inpaint_dump/mdm_old/bf16",
               "loop/sample/torch_tape/mdm/fp32",
               "loop/sample/interval/mdm_old/fp32", "loop/sample/refresh/mdm/fp32", "loop/sample/rescale/mdm/fp16",
               "loop/sample/layer_cache/mdm/fp32", "loop/sample/layer_cache/mdm_old/fp16", "loop/sample/layer_cache_tm/mdm/bf16",
               "loop/sample/graph_replay/mdm/fp32", "loop/sample/graph_replay/mdm_old/fp16"]
OTHER_LOOPS = {
    "gdx_plms_loop": ["loop/plms/cfg/mdm/fp32", "loop/plms/cfg/mdm_old/fp16"],
    "gdx_dpm_loop": ["loop/dpm/cfg/mdm/fp32", "loop/dpm/cfg/mdm_old/fp16"],
    "gdx_dpm_sde_loop": ["loop/dpm_sde/tape/mdm/fp32", "loop/dpm_sde/philox/mdm_old/fp16"],
    "gdx_unipc_loop": ["loop/unipc/cfg/mdm/fp32", "loop/unipc/cfg/mdm_old/fp16"],
    "gdx_ddim_reverse_loop": ["loop/ddim_reverse/cfg/mdm/fp32", "loop/ddim_reverse/cfg/mdm_old/fp16"],
    "gdx_bpd_loop": ["loop/bpd/cfg/mdm/fp32", "loop/bpd/cfg/mdm_old/fp16"],
    "gdx_parallel_loop": ["loop/parallel/tol0/mdm/fp32", "loop/parallel/tol1e-2/mdm_old/fp32"],
}
GUARDS = ["guards/check/mdm/fp32"]
MFCC = ["mfcc/n1000"]

# ---- test entry points (csrc/testapi.hip): one small case each; all of them stage through Scratch and synchronise
TEST_ENTRIES = {name: [f"entry/{name[4:]}"] for name in (
    "gdx_linear_full", "gdx_linear_half", "gdx_layernorm", "gdx_local_attention", "gdx_transpose_in", "gdx_transpose_out",
    "gdx_small_linear", "gdx_gather_rows", "gdx_mfcc_project", "gdx_token0", "gdx_attention_half", "gdx_attention_f32_rows",
    "gdx_attention_f16", "gdx_attention_f32")}

# ---- the Python protocol (no ABI name of its own)
PYTHON = {"p_sample_loop(fused=False)": ["python/p_sample_loop_stepwise/mdm"], "sample.generate.sample_chunks": ["python/sample_chunks/mdm_old"]}

# ---- cases outside the delayed-input protocol (their own tests in the GPU module; listed so that the table names every test)
SPECIAL = ["first_prepare_behind_a_busy_default_stream", "late_allocation/layer_cache", "late_allocation/parallel_loop",
           "late_allocation/bpd_loop", "two_handles_two_streams"]


def _entry(cases, syncs=False):
    return {"cases": list(cases), "syncs": syncs}


ALL_FORWARD = FORWARD + FORWARD_TAPS + FORWARD_RESCALE + FORWARD_TEXT
ALL_LOOPS = SAMPLE_LOOP + [c for v in OTHER_LOOPS.values() for c in v]

# ABI function name -> the cases that run it under the protocol, and whether it synchronises `stream` itself
ENTRY_CASES = {
    "gdx_set_weight": _entry(WEIGHTS_SET),
    "gdx_export_packed": _entry(WEIGHTS_PACKED, syncs=True),          # weights.hip: hipStreamSynchronize(s) before the host reads
    "gdx_import_packed": _entry(WEIGHTS_PACKED, syncs=True),          # weights.hip: the caller may free the blob on return
    "gdx_set_condition": _entry(FORWARD + FORWARD_TAPS + FORWARD_RESCALE + WEIGHTS_SET + WEIGHTS_PACKED + ALL_LOOPS),
    "gdx_set_condition_text": _entry(FORWARD_TEXT),
    "gdx_forward": _entry(ALL_FORWARD + WEIGHTS_SET + WEIGHTS_PACKED + PYTHON["p_sample_loop(fused=False)"]),
    "gdx_get_tap": _entry(FORWARD_TAPS),
    "gdx_check_guards": _entry(GUARDS, syncs=True),                   # handle.hip: hipStreamSynchronize(stream) before the read-back
    "gdx_sample_loop": _entry(SAMPLE_LOOP + PYTHON["sample.generate.sample_chunks"]),
    "gdx_mfcc": _entry(MFCC),
    **{name: _entry(cases) for name, cases in POSE.items()},
    **{name: _entry(cases, syncs=name == "gdx_parallel_loop") for name, cases in OTHER_LOOPS.items()},   # loops.hip: one
    # hipStreamSynchronize(s) per iteration of gdx_parallel_loop, to read the error rows
    **{name: _entry(cases, syncs=True) for name, cases in TEST_ENTRIES.items()},                         # Scratch::~Scratch
}

# Entries with a stream parameter and no case, each with its reason
EXEMPT = {
    "gdx_linear_f32": "a pure alias: it forwards its arguments to linear_full(), the body of the covered gdx_linear_full "
                      "(csrc/testapi.hip), and touches the stream nowhere else",
    "gdx_linear_f16": "a pure alias: it forwards its arguments to linear_half(), the body of the covered gdx_linear_half "
                      "(csrc/testapi.hip), and touches the stream nowhere else",
    "gdx_bench_ffn_gemm": "a timing hook: its only result is a duration, so there are no bits to compare; its launch is the "
                          "linear() of the covered forwards",
    "gdx_bench_gemm": "a timing hook: its only result is a duration; operands come from the covered gdx_randn, the launch "
                      "is gemm(), the one behind the covered gdx_linear_full",
    "gdx_bench_attention": "a timing hook: its only result is a duration; the launchers are those of the covered "
                           "gdx_attention_half / gdx_attention_f32_rows",
    "gdx_bench_gemm_f16": "a timing hook: its only result is a duration; the launch is launch_gemmh, the one behind the "
                          "covered gdx_linear_half",
}

PROTOCOL_CASES = sorted({c for e in ENTRY_CASES.values() for c in e["cases"]} | {c for v in PYTHON.values() for c in v})
# a case checks the gate before its call when any entry it runs synchronises; the step-wise Python loop does not synchronise
# (gaussian_diffusion.py's only synchronize() is under progress=True, which no case passes)
SYNCS = {c: any(e["syncs"] and c in e["cases"] for e in ENTRY_CASES.values()) for c in PROTOCOL_CASES}
