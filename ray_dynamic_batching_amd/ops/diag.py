"""Which kernel build is loaded, and the per-block stamps of the diagnostic
build (ops/csrc/common.h RDB_STAMP_*; ``python -m ray_dynamic_batching_amd._build
--variant stamps -D RDB_BLOCK_STAMPS``, loaded with RDB_OPS_SO).
bench/stamp_timeline.py turns the records into co-residency / CU-time of the
UN-profiled serving bench."""
from __future__ import annotations

import torch

from ._common import _check, _ops

_V4_BUILT = None


def experimental_kernels_built() -> bool:
    """Whether the loaded kernel library carries the opt-in variants that lost
    their A/Bs (stream-K, row-LayerNorm, LNOUT / staged-LN epilogues): built only
    with ``python -m ray_dynamic_batching_amd._build --variant experimental -D
    RDB_EXPERIMENTAL_KERNELS`` and loaded with RDB_OPS_SO (ops/csrc/common.h)."""
    f = getattr(_ops(), "experimental_kernels_built", None)
    return bool(f and f())


def _v4_tiles_built() -> bool:
    """The 4-wave VGPR-staged tiles (cfg 26..28) are part of the opt-in
    RDB_EXPERIMENTAL_KERNELS build only."""
    global _V4_BUILT
    if _V4_BUILT is None:
        try:
            _V4_BUILT = experimental_kernels_built()
        except Exception:  # noqa: BLE001 -- no kernel library (CPU host): not built
            _V4_BUILT = False
    return _V4_BUILT


def stamps_built() -> bool:
    """Whether the loaded kernel library is the RDB_BLOCK_STAMPS diagnostic build."""
    f = getattr(_ops(), "stamps_built", None)
    return bool(f and f())


class BlockStamps:
    """Device buffer the instrumented kernels write one record per block to:
    [t_begin, t_end, meta, where] u64 (common.h).  ``cap`` records at most; the
    counter keeps counting past it (``dropped``)."""

    def __init__(self, cap: int = 1 << 22, device="cuda"):
        _check(stamps_built(), "BlockStamps needs the RDB_BLOCK_STAMPS kernel build (RDB_OPS_SO=<variant .so>)")
        self.cap = int(cap)
        self.buf = torch.zeros(self.cap * 4, dtype=torch.int64, device=device)
        self.count = torch.zeros(1, dtype=torch.int32, device=device)
        _ops().stamps_set(self.buf.data_ptr(), self.count.data_ptr(), self.cap)

    def reset(self) -> None:
        torch.cuda.synchronize()
        self.count.zero_()
        torch.cuda.synchronize()

    def read(self):
        """The records written since the last reset, as an [n, 4] uint64 array."""
        import numpy as np

        torch.cuda.synchronize()
        n = min(int(self.count.item()), self.cap)
        return self.buf[: n * 4].view(n, 4).cpu().numpy().view(np.uint64)

    @property
    def dropped(self) -> int:
        return max(0, int(self.count.item()) - self.cap)

    def close(self) -> None:
        torch.cuda.synchronize()
        _ops().stamps_set(0, 0, 0)
