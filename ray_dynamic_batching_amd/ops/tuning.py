"""Per-shape autotuning of the GEMM / conv tile configuration.  The kernels
take a tile index (ops/tiles.py); on the first eager call of a shape every
candidate is timed and the fastest is cached.  Never runs while a hipGraph is
being captured (those calls use the cached choice, or the on-device heuristic
if the shape was never seen eagerly)."""
from __future__ import annotations

import os
from typing import Callable, Dict, Optional

import torch

from .tiles import NUM_TILE_CFGS, _cu_share, _key_mn

_TUNE: Dict[tuple, int] = {}


def autotune_enabled() -> bool:
    return os.environ.get("RDB_AUTOTUNE", "1") == "1"


def tuning_table() -> Dict[tuple, int]:
    return dict(_TUNE)


def _key_json(key: tuple) -> list:
    return [str(v) if isinstance(v, torch.dtype) else v for v in key]


def _key_from_json(key: list) -> tuple:
    return tuple(getattr(torch, v.split(".", 1)[1]) if isinstance(v, str) and v.startswith("torch.") else v
                 for v in key)


def save_tuning(path: str) -> None:
    """Write the per-shape tile table (JSON) so another process replays the same
    kernel choices (profiling passes, A/B runs) instead of re-tuning."""
    import json

    with open(path, "w") as f:
        json.dump([[_key_json(k), c] for k, c in _TUNE.items()], f)


def load_tuning(path: str) -> int:
    """Load a table written by save_tuning(); returns the number of entries."""
    import json

    with open(path) as f:
        rows = json.load(f)
    for k, c in rows:
        _TUNE[_key_from_json(k)] = int(c)
    return len(rows)


_TUNE_TOP: Dict[tuple, list] = {}


def tune_in_context(time_forward: Callable[[], float], keys: Optional[list] = None, min_gain: float = 0.01) -> dict:
    """Pick among each GEMM shape's near-tied tiles by timing the WHOLE forward.

    The per-shape tuner times a GEMM alone; inside a forward its inputs were just
    written by the previous kernel (dirty L2 lines, MALL residency) and its
    neighbours compete for the chip, and tiles within a few percent of each other
    alone can differ by 20 % there.  ``time_forward()`` must re-capture/replay the
    forward with the current ``_TUNE`` table and return its time; shapes are
    visited one at a time (coordinate descent), a change is kept only if it beats
    the current best by ``min_gain``.  Returns {key: (old, new)} for changed keys."""
    changed = {}
    best = time_forward()
    for key in list(keys if keys is not None else _TUNE_TOP):
        cands = _TUNE_TOP.get(key, [])
        if len(cands) < 2 or key not in _TUNE:
            continue
        start = cur = _TUNE[key]
        for c in cands:
            if c == cur:
                continue
            _TUNE[key] = c
            t = time_forward()
            if t < best * (1 - min_gain):
                best, cur = t, c
        _TUNE[key] = cur
        if cur != start:
            changed[key] = (start, cur)
    return changed


_KEY_LOG: Optional[list] = None


class record_tuning_keys:
    """``with record_tuning_keys() as keys: model(x)`` -> the tuned GEMM/conv keys that forward used."""

    def __enter__(self):
        global _KEY_LOG
        _KEY_LOG = []
        return _KEY_LOG

    def __exit__(self, *exc):
        global _KEY_LOG
        _KEY_LOG = None
        return False


# RDB_TUNE_GRAPH=1: time tuning candidates from a replayed hipGraph instead of eager launches.  Off by
# default: it ranks the kernels themselves without the Python launch path, but tables tuned that way
# served no better than eager-tuned ones (BERT 35.3k vs 35.0-35.8k, ResNet-50 41.1k vs 41.8-44.2k
# img/s, profiles/tuner_graph_timing_r6.json) -- the in-context pass decides among the top candidates
_TUNE_GRAPH = os.environ.get("RDB_TUNE_GRAPH", "0") == "1"
_tune_graph_broken = False
_TUNE_STREAMS: Dict[tuple, list] = {}


def _tune_streams(n: int) -> list:
    """The tuner's own streams on the current device (created once: per-stream
    split-K workspaces are cached by stream, so fresh streams per shape would
    each pin another workspace): [capture stream, side stream 1, ...]."""
    key = (torch.cuda.current_device(), n)
    st = _TUNE_STREAMS.get(key)
    if st is None:
        st = _TUNE_STREAMS[key] = [torch.cuda.Stream() for _ in range(n)]
    return st


def _time_tile_graph(launch: Callable[[int], None], c: int, cap, side: list, s, e, reps: int = 4) -> float:
    """Best-of-3 time of ``reps`` launches of tile ``c`` on the current stream
    (plus one per side stream each) replayed from a captured hipGraph.  Eager
    timing includes the Python launch path (~15 us per launch, as long as the
    faster BERT / ResNet kernels themselves at RDB_TUNE_STREAMS=3).  Every
    lazily allocated buffer (split-K workspaces) exists before the capture:
    the caller launched ``c`` eagerly on every stream first."""
    cur = torch.cuda.current_stream()
    cap.wait_stream(cur)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap, capture_error_mode="thread_local"):
        for _ in range(reps):
            launch(c)
            for sd in side:
                sd.wait_stream(cap)
                with torch.cuda.stream(sd):
                    launch(c)
        for sd in side:
            cap.wait_stream(sd)
    cur.wait_stream(cap)
    g.replay()                       # first replay: uploads the graph
    t = float("inf")
    for _trial in range(3):          # best of 3: clock / neighbour noise only ever adds time
        s.record()
        g.replay()
        e.record()
        e.synchronize()
        t = min(t, s.elapsed_time(e))
    del g
    return t


def _tuned_cfg(key: tuple, launch: Callable[[int], None], candidates=range(NUM_TILE_CFGS)) -> int:
    global _tune_graph_broken
    if _KEY_LOG is not None and key not in _KEY_LOG:
        _KEY_LOG.append(key)
    cfg = _TUNE.get(key)
    if cfg is not None:
        return cfg
    if not autotune_enabled() or torch.cuda.is_current_stream_capturing():
        return -1
    best_t, best_c = float("inf"), -1
    times: Dict[int, float] = {}
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    # RDB_TUNE_STREAMS=n (n > 1): rank tiles by THROUGHPUT with n launches in
    # flight on n streams -- what a replica running n concurrent batches sees --
    # instead of the isolated latency, which favours small tiles that fill the
    # CUs alone but cost more LDS/VMEM traffic per FLOP when streams overlap.
    ns = max(1, int(os.environ.get("RDB_TUNE_STREAMS", "1")))
    streams = _tune_streams(ns)
    cap, side = streams[0], streams[1:]
    cur = torch.cuda.current_stream()
    for c in candidates:
        launch(c)
        for sd in streams:               # every stream's lazily allocated buffers, outside any capture
            sd.wait_stream(cur)
            with torch.cuda.stream(sd):
                launch(c)
            cur.wait_stream(sd)
        t = float("inf")
        if _TUNE_GRAPH and not _tune_graph_broken:
            try:
                t = _time_tile_graph(launch, c, cap, side, s, e)
            except Exception:            # a launch path that cannot be captured: eager timing from here on
                _tune_graph_broken = True
                torch.cuda.synchronize()
        if t == float("inf"):
            for _trial in range(3):          # best of 3: clock / neighbour noise only ever adds time
                s.record()
                for sd in side:
                    sd.wait_stream(cur)
                for _ in range(4):
                    launch(c)
                    for sd in side:
                        with torch.cuda.stream(sd):
                            launch(c)
                for sd in side:
                    cur.wait_stream(sd)
                e.record()
                e.synchronize()
                t = min(t, s.elapsed_time(e))
        times[c] = t
        if t < best_t:
            best_t, best_c = t, c
    # the runners-up within 15 %: candidates for in-context selection (tune_in_context) ...
    top = [c for c in sorted(times, key=times.get) if times[c] <= best_t * 1.15][:3]
    mn = _key_mn(key)
    if mn is not None:
        # ... plus the two with the least CU-TIME (time x share of the CUs the grid holds): beside
        # another stream's batch a slower tile on fewer blocks can win (profiles/ab_r4_tables_cu_time.json:
        # BERT's o-projection on 96 ping-pong blocks, +2.7..6.5 % over the fastest-alone 256-block tile)
        cu = {c: t * _cu_share(c, *mn) for c, t in times.items() if t < float("inf")}
        top += [c for c in sorted(cu, key=cu.get)[:2] if c not in top]
    _TUNE_TOP[key] = top
    _TUNE[key] = best_c
    return best_c
