"""FP8 (W8A8) against bf16 on the four Llama-3-8B projection shapes, per op and
graph-replayed: ops.linear (bf16, its tuned tile), ops.linear_fp8 alone (the
static tile rule and every forced tile), and producer + GEMM on both sides --
rms_norm -> linear against rms_norm_fp8 -> linear_fp8 where a norm feeds the
GEMM (QKV, gate-up), linear against quantize_fp8_rows -> linear_fp8 elsewhere
(o-proj, down).  Each graph walks over enough copies of the weight that no call
finds its weight in L2 / MALL, as in a forward over 32 different layers.

    python bench/fp8_probe.py [--m 128,1024] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, N, K, act, norm feeds the GEMM)
SHAPES = [("qkv", 6144, 4096, "none", True), ("o_proj", 4096, 4096, "none", False),
          ("gate_up", 28672, 4096, "swiglu", True), ("down", 4096, 14336, "none", False)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", default="128,1024")
    ap.add_argument("--cold-mb", type=int, default=600, help="weight bytes a graph cycles through")
    ap.add_argument("--max-copies", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args(argv)
    import torch

    from ray_dynamic_batching_amd import ops

    def timed(fn, n) -> float:
        """us per call of fn(i), i = 0 .. n - 1, in one captured graph (best of --reps replays)."""
        fn(0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st), torch.cuda.graph(g, stream=st):
            for i in range(n):
                fn(i)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = 1e30
        for _ in range(a.reps):
            s.record()
            g.replay()
            e.record()
            torch.cuda.synchronize()
            best = min(best, s.elapsed_time(e) / n * 1e3)
        return best

    rows = []
    torch.manual_seed(0)
    for M in [int(v) for v in a.m.split(",")]:
        for name, N, K, act, normed in SHAPES:
            n = max(2, min(a.max_copies, -(-a.cold_mb * 2 ** 20 // (N * K))))
            ws = [(torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02) for _ in range(n)]
            wq = [ops.quantize_weight_fp8(w) for w in ws]
            x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
            gamma = torch.ones(K, device="cuda", dtype=torch.bfloat16)
            xq, xs = ops.quantize_fp8_rows(x)
            ops.linear(x, ws[0], act=act)             # tunes the bf16 tile for this shape (eager, once)
            r = dict(M=M, N=N, K=K, proj=name, act=act, weight_copies=n)
            r["bf16_linear_us"] = timed(lambda i: ops.linear(x, ws[i], act=act), n)
            r["fp8_linear_us"] = timed(lambda i: ops.linear_fp8(xq, xs, wq[i][0], wq[i][1], act=act), n)
            r["fp8_tile_us"] = [timed(lambda i: ops.linear_fp8(xq, xs, wq[i][0], wq[i][1], act=act, tile_cfg=t), n)
                                for t in range(ops.fp8_num_tiles())]
            if normed and K <= 4096:
                r["producer"] = "rms_norm_fp8 (bf16 side: rms_norm)"
                r["bf16_chain_us"] = timed(lambda i: ops.linear(ops.rms_norm(x, gamma), ws[i], act=act), n)
                r["fp8_chain_us"] = timed(
                    lambda i: ops.linear_fp8(*ops.rms_norm_fp8(x, gamma), wq[i][0], wq[i][1], act=act), n)
            else:
                r["producer"] = "quantize_fp8_rows (bf16 side: none)"
                r["bf16_chain_us"] = r["bf16_linear_us"]
                r["fp8_chain_us"] = timed(
                    lambda i: ops.linear_fp8(*ops.quantize_fp8_rows(x), wq[i][0], wq[i][1], act=act), n)
            fl = 2.0 * M * N * K
            r["bf16_tflops"] = fl / r["bf16_linear_us"] / 1e6
            r["fp8_tflops"] = fl / r["fp8_linear_us"] / 1e6
            r["speedup_linear"] = r["bf16_linear_us"] / r["fp8_linear_us"]
            r["speedup_chain"] = r["bf16_chain_us"] / r["fp8_chain_us"]
            r = {k: (round(v, 2) if isinstance(v, float) else [round(t, 2) for t in v] if isinstance(v, list) else v)
                 for k, v in r.items()}
            rows.append(r)
            print(json.dumps(r), flush=True)
            del ws, wq
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(metric="Llama-3-8B projections, bf16 ops.linear vs FP8 W8A8 ops.linear_fp8, us per call",
                           mfma="v_mfma_scale_f32_16x16x128_f8f6f4 (scales 1.0)", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
