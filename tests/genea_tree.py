"""A small GENEA 2023 data directory written from a seed: the layout `Genea2023` reads (see
gesturediffusion_amd/data_loaders/gesture/data/dataset.py), with random content.  The generator of
tests/golden/genea2023_items.npz (tools/make_golden_genea.py) and the tests build the same tree from GOLDEN_TREE, so what the
reference's class returned on it can be compared with what this project's class returns.
"""
import os

import numpy as np

GOLDEN_TREE = dict(J=12, frames_trn=[75, 64], frames_val=[95, 41, 130], seed=2023, zero_std_at=5)
GOLDEN_WINDOW, GOLDEN_SEED_POSES = 20, 4
FPS, SR, MFCC_DIM = 30, 22050, 26
WORDS = "so and then we went over there you know it was really quite something I mean yes no maybe".split()


def build_tree(root, J, frames_trn, frames_val, seed, zero_std_at=None):
    """Write a data directory under `root`, deterministically from `seed`: float32 motion [n, J] and float32 audio
    [n * 735] per take, word lists that end about one second before each take does (the windows at a take's end find no
    later word), float64 statistics.  zero_std_at: a feature whose deviation is 0 (it is constant in every take)."""
    rng = np.random.default_rng(seed)
    stats = os.path.join(root, "trn", "main-agent")
    os.makedirs(stats, exist_ok=True)
    mean, std = rng.normal(size=J), rng.uniform(0.5, 2.0, size=J)
    if zero_std_at is not None:
        std[zero_std_at] = 0.0
    for name, a in (("rotpos_Mean", mean), ("rotpos_Std", std), ("mfccs_Mean", rng.normal(size=MFCC_DIM)),
                    ("mfccs_Std", rng.uniform(0.5, 3.0, size=MFCC_DIM))):
        np.save(os.path.join(stats, name + ".npy"), a.astype(np.float64))
    for split, frames in (("trn", frames_trn), ("val", frames_val)):
        src = os.path.join(root, split, "main-agent")
        for sub in ("motion_npy_rotpos", "audio_npy", "tsv"):
            os.makedirs(os.path.join(src, sub), exist_ok=True)
        np.save(os.path.join(src, "rotpos_frames.npy"), np.asarray(frames, dtype=np.int64))
        rows = ["prefix,has_finger,speaker_id"]
        for k, n in enumerate(frames):
            take = f"{split}_2023_v0_{k:03d}"
            rows.append(f"{take},finger_incl,{k % 3}")
            motion = (mean + np.where(std == 0, 1.0, std) * rng.normal(size=(n, J))).astype(np.float32)
            if zero_std_at is not None:
                motion[:, zero_std_at] = np.float32(mean[zero_std_at])
            np.save(os.path.join(src, "motion_npy_rotpos", take + "_main-agent.npy"), motion)
            t = np.arange(n * SR // FPS) / SR
            audio = 0.3 * np.sin(2 * np.pi * (180 + 40 * k) * t) + 0.05 * rng.normal(size=t.size)
            np.save(os.path.join(src, "audio_npy", take + "_main-agent.npy"), audio.astype(np.float32))
            lines, start = [], 0.1
            while True:
                end = start + rng.uniform(0.15, 0.5)
                if end > n / FPS - 1.0:
                    break
                lines.append(f"{start:.3f}\t{end:.3f}\t{WORDS[rng.integers(len(WORDS))]}")
                start = end + rng.choice([0.0, 0.08, 0.3])
            with open(os.path.join(src, "tsv", take + "_main-agent.tsv"), "w") as f:
                f.write("\n".join(lines) + ("\n" if lines else ""))
        with open(os.path.join(root, split, "metadata.csv"), "w") as f:
            f.write("\n".join(rows) + "\n")
    return root
