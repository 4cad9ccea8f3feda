"""Operands that turn a linear kernel into a per-element probe of its activation (tests/test_gpu_activations.py; exactness is
checked on the host in tests/test_trained_scale_host.py).

A[m][0] = x_m, W[n][0] = 1, every other column of A and W zero, bias[n] = b_n: output element (m, n) is act(x_m + b_n) with no
summation error.  On the grids every x_m is exact in bf16, fp16 and fp32 and every x_m + b_n is an exact fp32 number, and all
M x 64 pre-activations differ, so every lane and register of a tile holds a different value.  Behind the grid rows come a few
special rows (M becomes odd, the last row tile partial); for those the pre-activation is the fp32 sum x_m + b_n (one rounding),
which `preact` computes the same way."""
import math

import torch

N = 64
BANDS = [(0.0, 1.0), (1.0, 2.0), (2.0, 3.0), (3.0, 4.2), (4.2, 6.0), (6.0, 16.0)]     # |x|; the last one closed; then "beyond"
BAND_NAMES = ["[0,1)", "[1,2)", "[2,3)", "[3,4.2)", "[4.2,6)", "[6,16]", ">16"]


def _m():
    return torch.arange(256, dtype=torch.float32) - 128.0


def _n():
    return torch.arange(N, dtype=torch.float32)


# name: (grid rows x_m, bias b_n)
GRIDS = {
    "wide": (lambda: _m() / 8.0, lambda: _n() / 512.0),                      # 16 384 values at spacing 1/512 over [-16, 16)
    "near": (lambda: _m() / 512.0, lambda: _n() * 2.0 ** -15),               # the same rows times 2^-6: [-0.25, 0.25)
    "silu": (lambda: _m() * 13.0 / 16.0, lambda: _n() / 512.0),              # [-104, 104): past expf's overflow at -88.7
}

# special rows: +-0, +-2^-14, +-32768 everywhere, 16 (the closed end of the last band); the fp32 kernels also get +-1e-30 and
# +-1e30, spread over the two launches so that each has nine special rows (M = 265)
COMMON = [0.0, -0.0, 2.0 ** -14, -2.0 ** -14, 32768.0, -32768.0]
SPECIAL = {
    ("half", "wide"): COMMON + [16.0],
    ("half", "near"): COMMON + [16.0],
    ("f32", "wide"): COMMON + [1e30, -1e30, 16.0],
    ("f32", "near"): COMMON + [1e-30, -1e-30, 16.0],
    ("f32", "silu"): COMMON + [1e30, -1e30, 1e-30],
}


def operands(kind, grid, device, K=64, tile_n=1):
    """(A [M][K], W [N tile_n][K], bias [N tile_n], pre-activation [M][N tile_n] in float64).  tile_n > 1 repeats b_n."""
    rows, bias = GRIDS[grid]
    x = torch.cat([rows(), torch.tensor(SPECIAL[(kind, grid)], dtype=torch.float32)])
    b = bias().repeat(tile_n)
    A = torch.zeros(x.numel(), K)
    A[:, 0] = x
    W = torch.zeros(b.numel(), K)
    W[:, 0] = 1.0
    pre = (x[:, None] + b[None, :]).double()                 # the fp32 sum: exact on the grid, one rounding on special rows
    return A.to(device), W.to(device), b.to(device), pre.to(device)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def silu64(x):
    return x * torch.sigmoid(x)


def band_masks(pre):
    """[(name, mask)] over |pre|, in BAND_NAMES order."""
    a = pre.abs()
    masks = [(a >= lo) & (a < hi) for lo, hi in BANDS]
    masks[-1] = (a >= BANDS[-1][0]) & (a <= BANDS[-1][1])
    masks.append(a > BANDS[-1][1])
    return list(zip(BAND_NAMES, masks))


def worst_per_band(err, pre, relative_to=None):
    """{band: worst err (or err / relative_to where given)} over the bands that hold an element."""
    out = {}
    for name, mk in band_masks(pre):
        if bool(mk.any()):
            e = err[mk] if relative_to is None else err[mk] / relative_to[mk].clamp_min(1e-300)
            out[name] = float(e.max())
    return out


def fmt(worst):
    return ", ".join(f"{k} {v:.3e}" for k, v in worst.items())
