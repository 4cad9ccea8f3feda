#!/usr/bin/env python3
"""Generate tests/golden/genea2023_items.npz by running the REFERENCE's Genea2023 class and gg_collate themselves.

Development-machine tool: builds the tree of tests/genea_tree.py (GOLDEN_TREE) in a temporary directory, imports the
reference at run time (never copied) and writes DATA only.  The reference's dataset module imports two packages that are
not installed here; both are stood in for in sys.modules: `librosa` by an empty module (imported, never called) and
`python_speech_features` by one whose `mfcc` is oracle/mfcc.py's restatement.  MFCC values are therefore NOT recorded --
they would be the stand-in's, not the reference's.

Recorded, for the 'train' and the 'val' split (window 20, 4 seed poses): `len`, `samples_per_file`, `samples_cumulative`,
`step`, and for EVERY item its motion, seed poses, text and audio window as (offset into the take, length, CRC-32 of the
bytes); the statistics after the class's zero-deviation fix; the collation of two 'val' items.

The archive is written with fixed zip timestamps: the same machine regenerates it byte for byte.

Usage:  python tools/make_golden_genea.py --ref <checkout of the reference> [--out tests/golden]
"""
import argparse
import os
import sys
import tempfile
import types
import zlib

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from genea_tree import GOLDEN_SEED_POSES, GOLDEN_TREE, GOLDEN_WINDOW, build_tree  # noqa: E402
from make_golden_bpd import save_npz  # noqa: E402
from oracle import mfcc as omfcc  # noqa: E402

COLLATED = (0, 8)          # 'val' items collated together: the first and the last one (different takes)


def import_reference(ref):
    psf = types.ModuleType("python_speech_features")
    psf.mfcc = omfcc.mfcc
    sys.modules.setdefault("python_speech_features", psf)
    sys.modules.setdefault("librosa", types.ModuleType("librosa"))
    sys.path.insert(0, ref)
    from data_loaders.gesture.data.dataset import Genea2023
    from data_loaders.tensors import gg_collate
    return Genea2023, gg_collate


def audio_record(window):
    """(offset into the take, length, CRC-32) of an audio window the reference returned: a view of the take it loaded."""
    whole = window.base
    offset = (window.__array_interface__["data"][0] - whole.__array_interface__["data"][0]) // window.itemsize
    return offset, window.size, zlib.crc32(np.ascontiguousarray(window).tobytes())


def gen(ref, out):
    Genea2023, gg_collate = import_reference(ref)
    d = {}
    with tempfile.TemporaryDirectory() as root:
        build_tree(root, **GOLDEN_TREE)
        for split in ("train", "val"):
            ds = Genea2023(split=split, datapath=root, window=GOLDEN_WINDOW, n_seed_poses=GOLDEN_SEED_POSES)
            items = [ds[i] for i in range(len(ds))]
            d[f"{split}.len"] = np.int64(len(ds))
            d[f"{split}.step"] = np.int64(ds.step)
            d[f"{split}.samples_per_file"] = np.asarray(ds.samples_per_file, dtype=np.int64)
            d[f"{split}.samples_cumulative"] = np.asarray(ds.samples_cumulative, dtype=np.int64)
            d[f"{split}.motion"] = np.stack([it[0] for it in items])
            d[f"{split}.seed_poses"] = np.stack([it[5] for it in items])
            d[f"{split}.text"] = np.asarray([it[1] for it in items])
            d[f"{split}.window"] = np.asarray([it[2] for it in items], dtype=np.int64)
            d[f"{split}.audio"] = np.asarray([audio_record(it[3]) for it in items], dtype=np.int64)
            d[f"{split}.audio_dtype"] = np.asarray(str(items[0][3].dtype))
            if split == "val":
                d["mean"], d["std"], d["mfcc_mean"], d["mfcc_std"] = ds.mean, ds.std, ds.mfcc_mean, ds.mfcc_std
                d["takes"] = np.asarray([t[0] for t in ds.takes])
                assert len(ds) == COLLATED[1] + 1
                motion, cond = gg_collate([items[i] for i in COLLATED])
                d["collate.idx"] = np.asarray(COLLATED, dtype=np.int64)
                d["collate.motion"] = motion.numpy()
                for k in ("seed", "mask", "lengths"):
                    d["collate." + k] = cond["y"][k].numpy()
    path = os.path.join(out, "genea2023_items.npz")
    save_npz(path, d)
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    path = gen(args.ref, args.out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
