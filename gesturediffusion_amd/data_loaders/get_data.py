"""Dataset and loader factory: drop-in for reference `data_loaders/get_data.py:5-37`.

Additive keywords: `datapath` (None = the class's default directory, the reference's only choice) and `device` (where the
items' MFCCs are computed; None = the current CUDA device).  The loader runs in the calling process (`num_workers=0`): an
item's MFCCs come from the GPU of that process, and the reference's eight CPU workers exist to run python_speech_features.
"""
from torch.utils.data import DataLoader

from .tensors import collate as all_collate
from .tensors import gg_collate


def get_dataset_class(name):
    if name == "genea2023":
        from .gesture.data.dataset import Genea2023
        return Genea2023
    if name == "genea2022":
        raise NotImplementedError("genea2022 is not provided: its items have five fields (no seed poses) and gg_collate, "
                                  "the generate path's collation, unpacks six -- the reference cannot sample from it either")
    raise ValueError(f'Unsupported dataset name [{name}]')


def get_collate_fn(name, hml_mode='train'):
    return gg_collate if name in ('genea2022', 'genea2023') else all_collate


def get_dataset(name, num_frames, seed_poses, split='train', hml_mode='train', datapath=None, device=None):
    where = {} if datapath is None else {"datapath": datapath}
    return get_dataset_class(name)(split=split, window=num_frames, n_seed_poses=seed_poses, device=device, **where)


def get_dataset_loader(name, batch_size, num_frames, split='train', hml_mode='train', seed_poses=10, datapath=None,
                       device=None):
    dataset = get_dataset(name, num_frames, seed_poses, split, hml_mode, datapath=datapath, device=device)
    return DataLoader(dataset, batch_size=batch_size, shuffle=split == 'train', num_workers=0, drop_last=True,
                      collate_fn=get_collate_fn(name, hml_mode))
