"""Split-K workspaces: who owns one when (caller, stream, graph capture, tuner)."""
from __future__ import annotations

import contextlib
import threading
from typing import Callable, Dict, Optional

import torch

from ._common import _stream
from .tiles import SPLITK_HEADER, SPLITK_WS_BYTES, splits_of

_tune_ws: Dict[int, torch.Tensor] = {}
_priv_ws: Dict[tuple, torch.Tensor] = {}
_cap_ws_local = threading.local()    # .ws: the split-K workspace of the capture running on this thread


def splitk_workspace(device, nbytes: int = SPLITK_WS_BYTES, zeroed: bool = True) -> torch.Tensor:
    """A split-K workspace: zeroed tile counters + f32 partial tiles.  Every
    split-K launch leaves the counters zero again, so one workspace serves the
    consecutive convolutions of a forward; two launches that may overlap (two
    streams) need two workspaces.  ``zeroed=False``: the caller zeroes the
    counter header itself before the first split-K launch (``image_to_s2d(zero=)``)."""
    ws = torch.empty(nbytes, device=device, dtype=torch.uint8)
    if zeroed:
        ws[:SPLITK_HEADER].zero_()
    return ws


@contextlib.contextmanager
def capture_splitk_workspace(ws: Optional[torch.Tensor]):
    """Graph captures inside this block give their split-K launches (those
    without a caller workspace) ``ws`` instead of a memset graph-pool workspace per
    launch.  ``ws`` (``splitk_workspace``, zeroed counters) must be used only by
    graphs that never run concurrently -- the engine keeps one per compute stream.
    Thread-local: a live capture on another thread is unaffected."""
    prev = getattr(_cap_ws_local, "ws", None)
    _cap_ws_local.ws = ws
    try:
        yield ws
    finally:
        _cap_ws_local.ws = prev


def _private_splitk_ws(device, need: int) -> torch.Tensor:
    """The split-K workspace a launch without a caller workspace uses: one per
    (device, stream), grown on demand, so a forward that passes none pays no
    allocation or counter memset per call.  Split-K launches leave the counters
    zero, so consecutive launches on one stream may share it (two streams never do).
    Inside a graph capture it is the workspace the capturing code installed with
    ``capture_splitk_workspace`` (the engine: one per compute stream, shared by the
    graphs replayed on that stream, which run in stream order and leave the
    counters zero -- no memset node at all), else a fresh one from the graph's own
    pool zeroed by a memset node per launch (never cached: a cached one would be
    shared by graphs replayed concurrently on different streams, and would keep
    the capture pool alive past the graph)."""
    need = max(SPLITK_HEADER, int(need))
    if torch.cuda.is_current_stream_capturing():
        ws = getattr(_cap_ws_local, "ws", None)
        if ws is not None and ws.numel() >= need:
            return ws
        return splitk_workspace(device, need)
    key = (str(device), _stream())
    ws = _priv_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _priv_ws[key] = splitk_workspace(device, max(need, SPLITK_WS_BYTES))
    return ws


def _tune_launcher(launch: Callable[[int, Optional[torch.Tensor]], None], device) -> Callable[[int], None]:
    """``launch(c, ws)`` as the one-argument launch ``_tuned_cfg`` times.  Tuning
    launches may overlap on side streams: a split-K choice gets the workspace of
    the stream it runs on, one per stream."""
    def tune_launch(c: int) -> None:
        ws = None
        if splits_of(c) > 1:
            sid = _stream()
            ws = _tune_ws.get(sid)
            if ws is None:
                ws = _tune_ws[sid] = splitk_workspace(device)
        launch(c, ws)
    return tune_launch
