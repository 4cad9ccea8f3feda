"""Shared by the GPU tests of the pose-layout kernels (not a test module)."""
import torch


def shifted(t):
    """The same values one element (a float; for a mask, a byte) off 16-byte alignment (the scalar path of the kernel)."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size()
    return v
