"""bench.py --dump-outputs on the GPU: the rows written for the last timed step
are the logits of the requests named by payload_index.npy."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_dumped_logits_are_the_models_forward_of_the_named_payloads(tmp_path):
    """Reference: the same model (seeded weights) called directly on all 256
    seeded payloads in batches of 32, with the tile table the benchmark
    replays, i.e. the kernels, tiles and batch size of the engine's graphs.

    Random-init BERT logits differ little between payloads (about 0.02 apart),
    so two things are asserted.  (1) Each dumped row is nearer the reference of
    the payload it names than the reference of any other of the 256 payloads:
    a row paired with the wrong request fails here.  (2) Each row is within one
    bf16 unit in the last place of the largest logit, 2^-8 * max|reference|
    (about 1.2e-3): activations are bf16, and identical kernels on identical
    inputs may differ by the rounding of one of them, not more.
    """
    import torch

    from ray_dynamic_batching_amd import ops
    from ray_dynamic_batching_amd.models.bert import BertConfig, BertForSequenceClassification
    from ray_dynamic_batching_amd.runtime.engine import resolve_tile_table

    steps = 20
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
           "--dump-outputs", str(tmp_path / "out")]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert line["steps"] == steps and line["completed"] == steps * 32 and line["errors"] == 0
    rows = np.load(tmp_path / "out" / "logits.npy")
    idx = np.load(tmp_path / "out" / "payload_index.npy")
    assert rows.dtype == np.float32 and rows.shape == (32, 2) and np.isfinite(rows).all()
    assert (idx == np.arange(steps * 32 - 32, steps * 32) % 256).all()
    idx = idx.astype(int)

    spec = importlib.util.spec_from_file_location("rdb_bench_script", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    cfg = BertConfig(seq_len=128, layers=12)
    payloads = bench.request_payloads(cfg.vocab_size, 128)
    m = BertForSequenceClassification(cfg, device="cuda", backend="hip")     # seeded weights, as in bench.py
    table = resolve_tile_table("auto", m, 32, line["config"]["compute_streams"], line["config"]["pipeline_depth"])
    assert os.path.basename(table) == line["config"]["tile_table"]
    ops.load_tuning(table)
    ids = torch.stack(payloads).to("cuda")
    ref = torch.cat([m(ids[i:i + 32]).float() for i in range(0, 256, 32)]).cpu().numpy()

    dist = np.linalg.norm(rows[:, None, :] - ref[None, :, :], axis=2)          # [32 rows, 256 payloads]
    own = dist[np.arange(32), idx]
    others = dist.copy()
    others[np.arange(32), idx] = np.inf
    err = float(np.abs(rows - ref[idx]).max())
    bound = 2.0 ** -8 * float(np.abs(ref).max())
    print(f"max abs diff {err:.3g} (bound {bound:.3g}); distance to the named payload's reference at most "
          f"{own.max():.3g}, to the nearest other payload's at least {others.min():.3g}")
    assert (dist.argmin(axis=1) == idx).all(), (dist.argmin(axis=1), idx)
    assert err <= bound
