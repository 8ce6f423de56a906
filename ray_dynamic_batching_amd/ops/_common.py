"""What every wrapper module shares: the dtype / activation codes of the C++
side, the extension handle, the host-side argument checks, and the fp32
activation the ``*_ref`` functions apply."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from ..utils.native import require_gpu_ops

DTYPE_CODE = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}
ACT_CODE = {"none": 0, "gelu": 1, "relu": 2, "tanh": 3, "silu": 4, "gelu_tanh": 5, "swiglu": 6, "sigmoid": 7}


def _ops():
    return require_gpu_ops()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _check(cond: bool, msg: str) -> None:
    if not cond:
        raise ValueError(msg)


def _aligned(t: torch.Tensor, n: int = 16) -> bool:
    return t.data_ptr() % n == 0


def _act_ref(y: torch.Tensor, act: str) -> torch.Tensor:
    if act == "gelu":
        return F.gelu(y)
    if act == "gelu_tanh":
        return F.gelu(y, approximate="tanh")
    if act == "relu":
        return F.relu(y)
    if act == "tanh":
        return torch.tanh(y)
    if act == "silu":
        return F.silu(y)
    if act == "sigmoid":
        return torch.sigmoid(y)
    return y
