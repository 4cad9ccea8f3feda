"""The GENEA 2023 dataset: drop-in for the `Genea2023` class of reference `data_loaders/gesture/data/dataset.py:9-127`.

A data directory holds, per split (`trn` for 'train', `val` for 'val'),

    <split>/metadata.csv                               one header row, then one row per take (column 0 = take name)
    <split>/main-agent/rotpos_frames.npy               frame count of every take
    <split>/main-agent/motion_npy_rotpos/<take>.npy    [n, J] poses
    <split>/main-agent/audio_npy/<take>.npy            [n * sr / fps] samples
    <split>/main-agent/tsv/<take>.tsv                  start <tab> end <tab> word, times in seconds

and the normalisation statistics of the training split under `trn/main-agent/` (`rotpos_Mean`, `rotpos_Std`, `mfccs_Mean`,
`mfccs_Std`, all `.npy`), which both splits use.  An item is one window of a take:
`(motion [window, J], text, window, audio [window * sr / fps], mfcc [window, 26], seed_poses [n_seed_poses, J])`, the tuple
`gg_collate` consumes.  Motion and seed poses are z-scored in numpy, so their dtype is numpy's (float64 for float64
statistics); the text is the words spoken during the window, joined by blanks.

What differs from the reference, none of it visible in the first four fields or the last:
  * the MFCCs are not computed on the CPU by python_speech_features but by `MfccExtractor` (libgdx's `gdx_mfcc`) on
    `device`: `mfcc` is an fp32 device tensor.  Without a GPU `__getitem__` raises `GdxError`; `locate`, `motion_window`,
    `audio_window` and `text_window`, from which it is composed, are host-only;
  * a take's arrays are memory-mapped on first use and kept (the reference re-reads both files for every item).
Genea2022 is not provided: its items have five fields and the generate path's `gg_collate` unpacks six.
"""
import csv
import functools
import os

import numpy as np
import torch
from torch.utils import data

SPLIT_DIR = {"train": "trn", "val": "val"}
OPEN_TAKES = 64          # takes whose files stay mapped (two maps and one word list each)


class Genea2023(data.Dataset):
    def __init__(self, split='train', datapath='./dataset/Genea2023/', step=30, window=80, fps=30, sr=22050, n_seed_poses=10,
                 device=None):
        if split not in SPLIT_DIR:
            raise NotImplementedError
        self.datapath, self.window, self.fps, self.sr, self.n_seed_poses = datapath, window, fps, sr, n_seed_poses
        self.step = step if split == 'train' else window          # validation windows do not overlap
        self.device = device

        stats = os.path.join(datapath, 'trn', 'main-agent')
        self.mean = np.load(os.path.join(stats, 'rotpos_Mean.npy'))
        self.std = _ones_for_zeros(np.load(os.path.join(stats, 'rotpos_Std.npy')))
        self.mfcc_mean = np.load(os.path.join(stats, 'mfccs_Mean.npy'))
        self.mfcc_std = np.load(os.path.join(stats, 'mfccs_Std.npy'))

        src = os.path.join(datapath, SPLIT_DIR[split], 'main-agent')
        self.motionpath = os.path.join(src, 'motion_npy_rotpos')
        self.audiopath = os.path.join(src, 'audio_npy')
        self.textpath = os.path.join(src, 'tsv')
        self.frames = np.load(os.path.join(src, 'rotpos_frames.npy'))
        self.samples_per_file = [int(np.floor((n - window) / self.step)) for n in self.frames]
        self.samples_cumulative = list(np.cumsum(self.samples_per_file))
        self.length = self.samples_cumulative[-1]

        with open(os.path.join(datapath, SPLIT_DIR[split], 'metadata.csv')) as f:
            self.takes = list(csv.reader(f, delimiter=','))[1:]
        for take in self.takes:
            take[0] += '_main-agent'
            for kind, path in (("Motion", self._path(self.motionpath, take[0])), ("Audio", self._path(self.audiopath, take[0])),
                               ("Text", self._path(self.textpath, take[0], '.tsv'))):
                assert os.path.isfile(path), f"{kind} file {path} not found"
        self._take = functools.lru_cache(maxsize=OPEN_TAKES)(self._open_take)
        self._extractor = None

    @staticmethod
    def _path(folder, name, ext='.npy'):
        return os.path.join(folder, name + ext)

    def _open_take(self, file_idx):
        """(motion map, audio map, words) of one take; words are [start frame, end frame, word]."""
        name = self.takes[file_idx][0]
        with open(self._path(self.textpath, name, '.tsv')) as f:
            words = [[float(row[0]) * self.fps, float(row[1]) * self.fps, row[2]] for row in csv.reader(f, delimiter='\t')]
        return (np.load(self._path(self.motionpath, name), mmap_mode='r'),
                np.load(self._path(self.audiopath, name), mmap_mode='r'), words)

    def __len__(self):
        return self.length

    # ------------------------------------------------------------------ host side
    def locate(self, idx):
        """Item index -> (take, window within the take)."""
        file_idx = int(np.searchsorted(self.samples_cumulative, idx + 1, side='left'))
        return file_idx, int(idx - self.samples_cumulative[file_idx - 1]) if file_idx > 0 else int(idx)

    def motion_window(self, file_idx, sample):
        """Z-scored poses of the window and of its first `n_seed_poses` frames."""
        rows = self._take(file_idx)[0]
        first = sample * self.step
        return ((rows[first: first + self.window, :] - self.mean) / self.std,
                (rows[first: first + self.n_seed_poses, :] - self.mean) / self.std)

    def audio_window(self, file_idx, sample):
        """The window's audio samples (a copy: the take itself stays mapped read-only)."""
        start = sample * self.sr * self.step / self.fps
        return np.array(self._take(file_idx)[1][int(start): int(start + self.window * self.sr / self.fps)])

    def text_window(self, file_idx, sample):
        """The words between the window's first frame and its end, joined by blanks."""
        words = self._take(file_idx)[2]
        first = sample * self.step
        span = slice(self.search_time(words, first), self.search_time(words, first + self.window))
        return ' '.join(word[-1] for word in words[span])

    def search_time(self, text, frame):
        """Index of the word at `frame`: the first word starting at or after it, or the one before that while `frame` has
        not passed its end.  None (an open slice bound) when every word starts earlier."""
        for i, word in enumerate(text):
            if frame <= word[0]:
                return i if i == 0 or frame > text[i - 1][1] else i - 1
        return None

    def inv_transform(self, data):
        return data * self.std + self.mean

    # ------------------------------------------------------------------ device side
    def mfcc_window(self, audio):
        """Normalised MFCCs [frames, 26] of an audio window: fp32, computed and left on the device."""
        if self._extractor is None:
            from ...mfcc import MfccExtractor
            device = self.device
            if device is None:
                if not torch.cuda.is_available():
                    from ...._lib import GdxError
                    raise GdxError("Genea2023 items need an MI355X GPU: their MFCCs are computed by gdx_mfcc "
                                   "(there is no CPU fallback in gesturediffusion_amd)")
                device = torch.device("cuda", torch.cuda.current_device())
            self._extractor = MfccExtractor(device, sr=self.sr, fps=self.fps, mfcc_mean=self.mfcc_mean, mfcc_std=self.mfcc_std)
        return self._extractor(torch.from_numpy(audio).to(self._extractor.device))

    def __getitem__(self, idx):
        file_idx, sample = self.locate(idx)
        motion, seed_poses = self.motion_window(file_idx, sample)
        audio = self.audio_window(file_idx, sample)
        return motion, self.text_window(file_idx, sample), self.window, audio, self.mfcc_window(audio), seed_poses


def _ones_for_zeros(std):
    """A zero deviation (a constant feature) divides as 1.  Replacing an entry widens the array as a Python 1 among its
    elements would (float32 statistics come back as float64), which is what the reference's rebuild of the array does."""
    zero = std == 0
    return np.where(zero, 1, std).astype(np.result_type(std.dtype, np.int64)) if zero.any() else np.array(std)
