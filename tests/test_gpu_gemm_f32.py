"""Kernel-level tests of the fp32 GEMMs: every tile shape of the persistent kernel (csrc/gemm2.hip gemm4_kernel, its
residual-prefetch variant RESP included) and the 128 x 128 fallback (csrc/gemm.hip), under each of the five launches of the
fp32 forwards (csrc/forward.hip forward_core), through the test entry point gdx_linear_full and the forwards' own dispatcher,
against float64 torch on the same fp32 inputs.  Need an MI355X.

What each call checks:
  * `launched` (recorded where the launch is decided) names the kernel that ran: a forced tile that silently fell back, or
    a missing RESP instantiation, fails;
  * every output buffer is NaN-prefilled and carries sentinel rows.  Rows that must be written are finite; token-0 rows of
    a row map and ALL rows past the output stay NaN for the general epilogue and for gemm.hip (both guard their stores).
    The plain and RESP epilogues of gemm2.hip store whole tiles by contract: rows past M may be written up to the end of
    the last row tile of the shape that ran, every later row stays NaN (the buffer reaches 160 rows past M, beyond the
    143-row overhang of the tallest tile);
  * the entry point puts NaN rows behind A and R, so a kernel that lets padding rows leak into stored rows fails;
  * random-normal data: within 3e-6 of max|ref| (the bound of test_fp32_gemm_every_tile_shape_vs_torch, all epilogues);
  * exact probe: A, W, bias, R, V integers in [-8, 8].  Every partial sum is an integer of magnitude <= 64 K + 24 < 2^24
    for K <= 4096, so fp32 is exact in any summation order and the non-GELU outputs must EQUAL the float64 reference: a
    dropped, doubled or misplaced k-slab, a transposed fragment, a wrong sample index at a sample boundary, a row or
    column permutation cannot hide below a tolerance.
"""
import ctypes as C

import pytest
import torch

from gesturediffusion_amd import _lib

pytestmark = pytest.mark.gpu

# gemm2.hip G4_CONFIGS (mb, nbw, bk, nst): tile = 16 mb rows x 64 nbw columns, K slab bk, nst LDS stages
G4 = [(4, 2, 32, 4), (5, 2, 32, 4), (6, 2, 32, 4), (8, 2, 32, 3), (9, 2, 32, 3), (5, 3, 32, 3), (4, 3, 32, 3), (4, 1, 64, 3),
      (5, 1, 64, 3), (4, 1, 32, 4), (5, 1, 32, 4), (8, 1, 32, 4), (9, 1, 32, 4), (2, 1, 64, 3), (1, 1, 64, 3),
      (5, 2, 64, 2), (5, 3, 64, 2), (4, 2, 64, 2), (6, 2, 64, 2), (8, 2, 64, 2), (4, 3, 64, 2)]
COST_MODEL = (0, 0, 0, 0)
TOL = 3e-6                      # of max|ref|, random-normal data, every epilogue
OVERHANG = 160                  # sentinel rows behind M for the whole-tile epilogues: 143 (tallest tile) + 16, rounded up
GEMM2, GEMM1 = 1, 2             # launched[0]: csrc/gemm2.hip, csrc/gemm.hip

# name: (bias, gelu, R, V, rowmap) -- the launches of forward_core
EPILOGUES = {
    "bias": (1, 0, 0, 0, 0),            # QKV, output linear, V2 in_x
    "bias_gelu": (1, 1, 0, 0, 0),       # FFN-1
    "bias_res": (1, 0, 1, 0, 0),        # out-proj, FFN-2: RESP where mb * nbw <= 10
    "res_rowmap": (0, 0, 1, 0, 1),      # V1 input linear: + addend rows, frames into [B, T+1] rows
    "res_vec": (0, 0, 1, 1, 0),         # V2 proj_pose: + addend + per-sample coarse vector
}
USES_T = ("res_rowmap", "res_vec")


def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int32)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def g4_valid(tile, N, K):
    """gemm2.hip g4_valid: the tile divides N and K and its LDS ring plus the N-float bias copy fits 160 KiB."""
    mb, nbw, bk, nst = tile
    rowb = (bk + 8) * 4
    stage = (mb * 16 * rowb + 1023) // 1024 * 1024 + (nbw * 64 * rowb + 1023) // 1024 * 1024
    return N % (nbw * 64) == 0 and K % bk == 0 and nst * stage + N * 4 <= 160 * 1024


def offered(N, K, has_R):
    """The shapes launch_gemm2 chooses from: valid ones, without the two-stage rings when a residual / hoisted term is set."""
    return [t for t in G4 if g4_valid(t, N, K) and not (t[3] == 2 and has_R)]


class Problem:
    """Operands for up to Mmax rows, random-normal ("rand") and integer-valued ("int"), with the float64 product computed
    once; a call uses the leading M rows (R and V are indexed by output row / sample, so their leading rows serve too)."""

    def __init__(self, Mmax, N, K, seed, kinds=("rand", "int")):
        d = dev()
        self.Mmax, self.N, self.K = Mmax, N, K
        self.ldr, self.ldv = N + 4, N + 8                      # strides wider than N
        g = torch.Generator(device=d).manual_seed(seed)
        self.data = {}
        for kind in kinds:
            if kind == "rand":
                mk = lambda *s: torch.randn(*s, device=d, generator=g)               # noqa: E731
                A, W = mk(Mmax, K), mk(N, K) / K ** 0.5
            else:
                mk = lambda *s: torch.randint(-8, 9, s, device=d, generator=g).float()   # noqa: E731
                A, W = mk(Mmax, K), mk(N, K)
            bias, R, V = mk(N), mk(2 * Mmax + 1, self.ldr), mk(Mmax, self.ldv)    # T = 1: 2 M rows of R, M of V
            self.data[kind] = (A, W, bias, R, V, A.double() @ W.double().t())


def run(lib, A, W, bias, R, ldr, V, ldv, out, M, N, K, T, rowmap, gelu, kernel, tile):
    la = (C.c_int32 * 6)()
    _lib.check(lib.gdx_linear_full(vp(A), vp(W), vp(bias), vp(R), ldr, vp(V), ldv, vp(out), out.shape[0], M, N, K, T, rowmap,
                                   gelu, kernel, tile[0], tile[1], tile[2], la, stream()), lib)
    return tuple(la)


def check(lib, pb, kind, ename, M, T, tile, kernel=1, log=None):
    """One call on the leading M rows of pb: launched, sentinel rows, value check.  Returns (launched, output rows [M][N],
    relative error)."""
    d = dev()
    ub, gelu, uR, uV, rowmap = EPILOGUES[ename]
    A, W, bias, R, V, prod = pb.data[kind]
    N, K = pb.N, pb.K
    ar = torch.arange(M, device=d)
    rsel = ar + ar // T + 1 if rowmap else ar                                      # rowmap: m -> m + m/T + 1
    rows_out = M + (M - 1) // T + 1 if rowmap else M
    ref = prod[:M].clone()
    if ub:
        ref += bias.double()
    if uR:
        ref += R[rsel, :N].double()
    if uV:
        ref += V[ar // T, :N].double()
    if gelu:
        ref = torch.nn.functional.gelu(ref)
    whole_tiles_possible = kernel != 2 and not uV and not rowmap
    out = torch.full((rows_out + (OVERHANG if whole_tiles_possible else 3), N), float("nan"), device=d)
    la = run(lib, A, W, bias if ub else None, R if uR else None, pb.ldr, V if uV else None, pb.ldv, out, M, N, K, T, rowmap, gelu,
             kernel, tile)
    what = f"{kind} {ename} M={M} N={N} K={K} T={T} kernel={kernel} tile={tile[:3]} launched={la}"
    # ---- what ran
    if kernel == 2:
        assert la == (GEMM1, 0, 0, 0, 0, 0), f"{what}: gemm.hip was asked for"
    elif kernel == 1 or la[0] == GEMM2:
        ran = la[1:5]
        assert la[0] == GEMM2 and ran in offered(N, K, uR), f"{what}: not a shape launch_gemm2 offers for this problem"
        if tile != COST_MODEL and tile in offered(N, K, uR):
            assert ran == tile, f"{what}: the forced tile did not run"
        elif tile != COST_MODEL and g4_valid(tile, N, K):
            assert tile[3] == 2 and uR and ran[3] != 2, f"{what}: only a two-stage shape under R may be replaced"
        resp = ran[0] * ran[1] <= 10 and uR and not uV and not rowmap and not gelu
        assert la[5] == int(resp), f"{what}: RESP runs exactly when mb * nbw <= 10, R, no V, no row map, bias epilogue"
    else:
        assert la == (GEMM1, 0, 0, 0, 0, 0), what
    # ---- which rows were stored
    fin = torch.isfinite(out)
    assert bool(fin[rsel].all()), f"{what}: a row that must be written holds a non-finite value"
    untouched = torch.ones(out.shape[0], dtype=torch.bool, device=d)
    untouched[rsel] = False
    if la[0] == GEMM2 and (la[5] or not (uR or uV or rowmap)):                    # whole-tile stores: plain and RESP epilogues
        bm = 16 * la[1]
        untouched[M:(M + bm - 1) // bm * bm] = False
    assert bool(torch.isnan(out[untouched]).all()), f"{what}: a row that must stay untouched was written"
    # ---- values
    got = out[rsel]
    err = float(((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item())
    if log is not None:
        log[(kind, ename)] = max(log.get((kind, ename), 0.0), err)
    if kind == "int" and not gelu:
        assert torch.equal(got, ref.float()), f"{what}: exact-integer probe differs from float64 (rel err {err:.2e})"
    else:
        assert err < TOL, f"{what}: rel err {err:.2e}"
    return la, got, err


def fmt(log):
    return ", ".join(f"{k[0]}/{k[1]} {v:.2e}" for k, v in sorted(log.items()))


# ---------------------------------------------------------------------------------------------------------------------
# (a) + (b): every tile x every forward epilogue, random-normal and exact-integer data.  N = 384 = 6 x 64 = 3 x 128 = 2 x 192
# and K = 192 = 6 x 32 = 3 x 64 make all 21 shapes valid on ONE problem, so the float64 product is computed once per row class.
SWEEP_N, SWEEP_K = 384, 192
# row class -> (rows for a tile of mb 16-row blocks and ntn column tiles, T values for the epilogues that use T);
# T covers 1, fewer than 16 (several samples per 16-row block), 16, 17 and 197, with M a multiple of T and not
ROW_CLASSES = {
    "one_row": (lambda mb, ntn: 1, (1,)),
    "below_a_tile": (lambda mb, ntn: 77, (7, 16)),
    "three_tiles_plus_5": (lambda mb, ntn: 16 * mb * 3 + 5, (17, 16)),
    "more_tiles_than_cus_plus_11": (lambda mb, ntn: 16 * mb * (cus() // ntn + 1) + 11, (197, 7)),
}
SEEN = {}                       # row class -> {(tile, resp)} seen by the sweep (asserted per class at its end)


@pytest.mark.parametrize("rows", list(ROW_CLASSES))
def test_every_tile_every_forward_epilogue(rows):
    """All 21 G4_CONFIGS shapes forced in turn (kernel = 1: no fallback) and the cost model's choice, under the five launches
    of forward_core, on random-normal data (3e-6 of max|ref|) and exact-integer data (equal to float64).  `launched` must
    name the forced shape, with the two exceptions the code states, asserted: a two-stage shape is not offered when R is set
    (another valid shape runs), and RESP runs exactly when mb * nbw <= 10, R set, V null, OUT_ROWS, bias epilogue.  Every
    shape must have run plain and every eligible shape as RESP.  The non-GELU outputs of all shapes agree bit for bit on the
    rows they share (the shapes get different row counts in the last two classes; leading rows of a larger problem equal the
    smaller problem's rows)."""
    lib = _lib.load()
    N, K = SWEEP_N, SWEEP_K
    m_of, Ts = ROW_CLASSES[rows]
    tiles = G4 + [COST_MODEL]
    Ms = {t: m_of(t[0] or 9, N // (64 * (t[1] or 1))) for t in tiles}            # cost model: the rows of the 144 x 64 tile
    pb = Problem(max(Ms.values()), N, K, seed=len(rows))
    log, seen = {}, set()
    for kind in ("rand", "int"):
        for ename in EPILOGUES:
            for T in (Ts if ename in USES_T else Ts[:1]):
                first = None
                for tile in tiles:
                    la, got, _ = check(lib, pb, kind, ename, Ms[tile], T, tile, log=log)
                    if ename in ("bias", "bias_gelu", "bias_res"):
                        seen.add((la[1:5], la[5]))
                    if first is None:
                        first = got
                    n = min(first.shape[0], got.shape[0])
                    # (GELU across shapes is test_tile_and_batch_independence_bitwise's: it lists every differing pair)
                    assert ename == "bias_gelu" or torch.equal(bits(got[:n]), bits(first[:n])), \
                        f"{kind} {ename} T={T} tile {tile[:3]} (launched {la}): bits differ from tile {G4[0][:3]}"
    plain = {t for t, resp in seen if not resp}
    resp = {t for t, resp in seen if resp}
    assert plain == set(G4), f"shapes that never ran plain: {set(G4) - plain}"
    eligible = {t for t in G4 if t[0] * t[1] <= 10 and t[3] != 2}
    assert resp == eligible, f"RESP instantiations: ran {sorted(resp)}, expected {sorted(eligible)}"
    print(f"\n[gemm2 sweep {rows} N={N} K={K} rows {min(Ms.values())}..{max(Ms.values())} T={Ts}] {len(plain)} shapes ran plain, "
          f"{len(resp)} as RESP; all shapes bit-equal; worst rel err " + fmt(log))


# ---------------------------------------------------------------------------------------------------------------------
# (c) K and N edges, tile counts
RING_REPS = [(4, 2, 32, 4), (4, 1, 64, 3), (4, 2, 64, 2), COST_MODEL]             # one shape per ring depth + the cost model
EDGE_EPILOGUES = ("bias", "bias_res", "res_vec")                                  # plain, RESP (general for NST = 2), general


@pytest.mark.parametrize("tile", RING_REPS, ids=["nst4", "nst3", "nst2", "cost_model"])
def test_k_edges_ring_prologue(tile):
    """K = bk, 2 bk, 3 bk (fewer slabs than the NST - 1 the ring prologue issues: the loaders re-read past the end of the
    block's work) and K = 4096 (FFN-2), with a single tile and with several rounds of tiles."""
    lib = _lib.load()
    mb, nbw, bk = (tile[0] or 4), (tile[1] or 2), (tile[2] or 64)
    N1, N2 = 64 * nbw, 128 * nbw
    many = 16 * mb * (cus() + 2) - 5                                              # 2 (cus + 2) tiles on N2: > 2 rounds
    log, ran = {}, set()
    for K in (bk, 2 * bk, 3 * bk, 4096):
        for N, M in ((N1, 16 * mb - 3), (N2, many)):
            pb = Problem(M, N, K, seed=K + N, kinds=("int", "rand"))
            for ename in EDGE_EPILOGUES:
                la, _, _ = check(lib, pb, "int", ename, M, 37, tile, log=log)
                ran.add(la[1:6])
            check(lib, pb, "rand", "bias_res", M, 37, tile, log=log)
            del pb
    print(f"\n[gemm2 K edges tile={tile[:3]}] ran {sorted(ran)}; worst rel err " + fmt(log))


@pytest.mark.parametrize("N", [64, 1536, 4096, 8192])
def test_n_edges_lds_bias_copy(N):
    """N = 64 (one column tile: the MFCC mel GEMM), 1536 (QKV at d = 512), 4096 and 8192 (gemm2_supported's limit): the bias
    copy in LDS takes N floats from the ring, so g4_valid admits fewer shapes as N grows.  Every shape is forced; the ones
    g4_valid admits must run, for the others what ran must be an admitted shape."""
    lib = _lib.load()
    K = 192
    log, admitted, ran = {}, [t for t in G4 if g4_valid(t, N, K)], set()
    assert admitted, "no shape left: the dispatcher would fall back"
    pb = Problem(333, N, K, seed=N)
    for tile in G4 + [COST_MODEL]:
        for ename in EDGE_EPILOGUES:
            la, _, _ = check(lib, pb, "int", ename, 333, 37, tile, log=log)
            ran.add(la[1:5])
        check(lib, pb, "rand", "bias", 333, 37, tile, log=log)
    assert ran <= set(admitted)
    print(f"\n[gemm2 N={N} K={K}] g4_valid admits {len(admitted)} of 21 shapes, ran {len(ran)}; worst rel err " + fmt(log))


@pytest.mark.parametrize("tile", [(4, 1, 32, 4), (9, 1, 32, 4), COST_MODEL], ids=["64x64", "144x64", "cost_model"])
def test_tile_counts_and_xcd_remap(tile):
    """1, 3 and 13 tiles (grids that are not multiples of 8: the r != 0 arm of the XCD remap), exactly one tile per CU, and
    one tile more than CUs (one block walks two tiles)."""
    lib = _lib.load()
    mb = tile[0] or 4
    N, K = 64, 96
    log, ran = {}, set()
    for count in (1, 3, 13, cus(), cus() + 1):
        M = 16 * mb * count - 7
        pb = Problem(M, N, K, seed=count)
        for ename in ("bias", "bias_res", "res_rowmap"):
            la, _, _ = check(lib, pb, "int", ename, M, 17, tile, log=log)
            ran.add(la[1:6])
            if tile != COST_MODEL:
                assert (M + 16 * la[1] - 1) // (16 * la[1]) * (N // (64 * la[2])) == count
        check(lib, pb, "rand", "res_rowmap", M, 17, tile, log=log)
    print(f"\n[gemm2 tile counts 1, 3, 13, {cus()}, {cus() + 1} tile={tile[:3]}] ran {sorted(ran)}; worst rel err " + fmt(log))


# ---------------------------------------------------------------------------------------------------------------------
# (d) tile and batch independence, bit for bit
def test_tile_and_batch_independence_bitwise():
    """gemm2.hip's header: summation order per output element is k-slab by k-slab and does not depend on the tile shape.
    For each epilogue (GELU included), all 21 forced shapes (both slab depths, all ring depths) and the cost model's choice
    give identical bits on one problem, and rows 0 .. M1-1 of a problem with M2 > M1 rows (same leading rows of A and R, M1
    a multiple of T) equal the M1-row result."""
    lib = _lib.load()
    T, M1 = 37, 9 * 37
    M2 = M1 + 5 * 37 + 3
    pb = Problem(M2, SWEEP_N, SWEEP_K, seed=4, kinds=("rand",))
    differing = []
    for ename in EPILOGUES:
        first = None
        for tile in G4 + [COST_MODEL]:
            la1, got1, _ = check(lib, pb, "rand", ename, M1, T, tile)
            la2, got2, _ = check(lib, pb, "rand", ename, M2, T, tile)
            if first is None:
                first = got1
            for got, la, nm in ((got1, la1, "M1"), (got2[:M1], la2, "M2 leading rows")):
                if not torch.equal(bits(got), bits(first)):
                    differing.append((ename, tile[:3], la, nm, float((got - first).abs().max())))
    assert not differing, f"outputs depend on the tile shape / row count: {differing}"
    print(f"\n[gemm2 independence N={SWEEP_N} K={SWEEP_K} M1={M1} M2={M2} T={T}] 21 shapes + cost model, 5 epilogues: identical bits")


# ---------------------------------------------------------------------------------------------------------------------
# (e) hostile padding: the entry point's NaN rows behind A and R, at the largest overhang and at none
@pytest.mark.parametrize("tile", [(9, 1, 32, 4), (9, 2, 32, 3), (4, 2, 64, 2)], ids=["144x64", "144x128", "64x128_nst2"])
def test_hostile_padding_at_tile_boundaries(tile):
    """M one row past a tile boundary (the last row tile holds one real row and 16 mb - 1 NaN rows of A; RESP clamps its R
    rows) and M a multiple of the tile height (no overhang: nothing past M may be written), per epilogue."""
    lib = _lib.load()
    bm = 16 * tile[0]
    N, K = 128, 128
    log = {}
    pb = Problem(3 * bm + 1, N, K, seed=bm)
    for M in (2 * bm + 1, 3 * bm + 1, 2 * bm, bm):
        for ename in EPILOGUES:
            for kind in ("int", "rand"):
                check(lib, pb, kind, ename, M, 16, tile, log=log)
    print(f"\n[gemm2 hostile padding tile={tile[:3]}] worst rel err " + fmt(log))


# ---------------------------------------------------------------------------------------------------------------------
# (f) the fallback kernel
FALLBACK_T = {1: (1,), 77: (7, 16), 129: (17, 16), 3000: (197, 7)}


@pytest.mark.parametrize("N", [96, 160, 288, 8256, 128])
def test_fallback_kernel_every_epilogue(N):
    """csrc/gemm.hip's five instantiations: forced (kernel = 2) and, on widths gemm2.hip refuses (N % 64 != 0: d = 96 with
    3 d = 288 and ff = 160; N > 8192), through the dispatcher, where `launched` must say that gemm.hip ran.  N = 128 is a
    width gemm2.hip takes: forced only.  This kernel guards every store: all sentinel rows stay NaN."""
    lib = _lib.load()
    K = 96
    log = {}
    kernels = (2,) if N % 64 == 0 and N <= 8192 else (2, 0)
    if len(kernels) == 2:
        pb = Problem(77, N, K, seed=N, kinds=("int",))
        with pytest.raises(_lib.GdxError, match="does not take this problem"):
            check(lib, pb, "int", "bias", 77, 7, COST_MODEL, kernel=1)
    for M, Ts in FALLBACK_T.items():
        pb = Problem(M, N, K, seed=N + M)
        for kernel in kernels:
            for kind in ("rand", "int"):
                for ename in EPILOGUES:
                    for T in (Ts if ename in USES_T else Ts[:1]):
                        la, _, _ = check(lib, pb, kind, ename, M, T, COST_MODEL, kernel=kernel, log=log)
                        assert la[0] == GEMM1
    print(f"\n[gemm.hip N={N} K={K} kernels {kernels}] worst rel err " + fmt(log))
