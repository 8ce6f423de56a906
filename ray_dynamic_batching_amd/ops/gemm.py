"""GEMM (+ fused bias / activation / residual epilogue) and the stream-K GEMM."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from ._common import ACT_CODE, DTYPE_CODE, _act_ref, _aligned, _check, _ops, _ptr, _stream
from .splitk import _private_splitk_ws, _tune_launcher
from .tiles import SKINNY_MAX_M, _SWIGLU_TILE_CFGS, _gemm_candidates, splits_of
from .tuning import _tuned_cfg


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: str = "none",
           residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
           out_dtype: Optional[torch.dtype] = None, alpha: float = 1.0, tile_cfg: int = -1,
           workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = act(alpha * x @ w.T + bias + residual).  x: [..., K] or a 2-D row-strided
    view; w: [N, K] contiguous.  act="swiglu" expects w rows interleaved (gate, up)
    and returns N/2 columns.  ``workspace`` (``splitk_workspace``): used when the
    chosen tile is split-K (else a private one is allocated)."""
    _check(x.is_cuda and w.is_cuda, "linear: tensors must be on the GPU")
    _check(x.dtype in (torch.bfloat16, torch.float16) and w.dtype == x.dtype, "linear: bf16/f16 inputs of equal dtype")
    _check(w.dim() == 2 and w.is_contiguous(), "linear: w must be a contiguous [N, K] matrix")
    N, K = w.shape
    _check(x.shape[-1] == K, f"linear: K mismatch {tuple(x.shape)} vs {tuple(w.shape)}")
    _check(K % 8 == 0, "linear: K must be a multiple of 8")
    if x.dim() == 2 and x.stride(1) == 1:
        x2, lead = x, (x.shape[0],)
    else:
        _check(x.is_contiguous(), "linear: x must be contiguous (or a 2-D row-strided view)")
        lead = tuple(x.shape[:-1])
        x2 = x.reshape(-1, K)
    M = x2.shape[0]
    lda = x2.stride(0)
    _check(lda % 8 == 0 and _aligned(x2) and _aligned(w), "linear: rows must be 16-byte aligned")
    n_out = N // 2 if act == "swiglu" else N
    od = out_dtype or x.dtype
    if out is None:
        out = torch.empty(*lead, n_out, device=x.device, dtype=od)
    _check(out.is_contiguous() and out.shape[-1] == n_out and out.numel() == M * n_out, "linear: bad out")
    if bias is not None:
        _check(bias.is_contiguous() and bias.numel() == N and bias.dtype == x.dtype, "linear: bad bias")
    ldr = 0
    if residual is not None:
        if residual.is_contiguous():
            _check(residual.numel() == M * n_out, "linear: bad residual")
            ldr = n_out
        else:
            _check(residual.dim() == 2 and residual.stride(1) == 1 and residual.shape[0] == M
                   and residual.stride(0) % 4 == 0 and _aligned(residual, 8), "linear: bad strided residual")
            ldr = residual.stride(0)          # 2-D row-strided view (e.g. the CLS rows)
        _check(residual.dtype == x.dtype and residual.shape[-1] == n_out, "linear: bad residual")
    args = (DTYPE_CODE[x.dtype], DTYPE_CODE[od], x2.data_ptr(), lda, w.data_ptr(), K, out.data_ptr(),
            n_out, _ptr(bias), _ptr(residual), ldr, M, N, K, float(alpha), ACT_CODE[act])
    fn = _ops().gemm_tn_sk
    skinny = M <= SKINNY_MAX_M and K % 32 == 0 and act != "swiglu"   # C++ routes these to the skinny-M kernel

    def launch(c: int, ws: Optional[torch.Tensor]) -> None:
        if c >= 0 and splits_of(c) > 1 and ws is None:
            # a split-K choice without a caller workspace: the cached one of this stream
            ws = _private_splitk_ws(x.device, int(_ops().conv_splitk_bytes(M, N, c & 255, splits_of(c))))
        fn(*args, _stream(), int(c), _ptr(ws), 0 if ws is None else ws.numel())

    if tile_cfg < 0 and od != torch.float32 and not skinny:
        key = ("gemm", x.dtype, M, N, K, lda, act, bias is not None, residual is not None)
        tile_cfg = _tuned_cfg(key, _tune_launcher(launch, x.device),
                              _gemm_candidates(M, N, K, splitk=True) if act != "swiglu" else _SWIGLU_TILE_CFGS)
    launch(int(tile_cfg), workspace)
    return out


def linear_ref(x, w, bias=None, act="none", residual=None, out_dtype=None, alpha=1.0):
    y = alpha * (x.float() @ w.float().t())
    if bias is not None:
        y = y + bias.float()
    if act == "swiglu":
        g, u = y[..., 0::2], y[..., 1::2]
        y = F.silu(g) * u
        if residual is not None:
            y = y + residual.float()
    else:
        if residual is not None:
            y = y + residual.float()
        y = _act_ref(y, act)
    return y.to(out_dtype or x.dtype)


def streamk_workspace(device, grid: int = 192, tile: int = 0) -> torch.Tensor:
    """A zeroed workspace for ``linear_streamk`` (arrival counters + f32 partial
    tiles).  One per stream: two launches must never share one at the same time."""
    n = int(_ops().gemm_sk_workspace_size(int(tile), int(grid)))
    return torch.zeros(n, device=device, dtype=torch.uint8)


def linear_streamk(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: str = "none",
                   residual: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                   grid: int = 192, tile: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``linear`` on the stream-K ping-pong GEMM (ops/csrc/gemm_sk.h): the
    (tile, K-step) space split evenly over ``grid`` workgroups, split tiles
    finished by their last-arriving segment.  bf16 only, contiguous operands,
    N % 8 == 0.  tile 0 = 256 x 128 (BK 64, 3 stages), 1 = 128 x 128 (BK 64, 4 stages)."""
    _check(x.is_cuda and w.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16,
           "linear_streamk: bf16 GPU tensors")
    _check(w.dim() == 2 and w.is_contiguous() and x.is_contiguous(), "linear_streamk: contiguous x, w")
    N, K = w.shape
    _check(x.shape[-1] == K and K % 8 == 0 and N % 8 == 0, "linear_streamk: shapes")
    _check(act != "swiglu", "linear_streamk: no SwiGLU")
    x2 = x.reshape(-1, K)
    M = x2.shape[0]
    if out is None:
        out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=x.dtype)
    _check(out.is_contiguous() and out.numel() == M * N, "linear_streamk: bad out")
    if residual is not None:
        _check(residual.is_contiguous() and residual.numel() == M * N and residual.dtype == x.dtype,
               "linear_streamk: bad residual")
    if bias is not None:
        _check(bias.is_contiguous() and bias.numel() == N and bias.dtype == x.dtype, "linear_streamk: bad bias")
    need = int(_ops().gemm_sk_workspace_size(int(tile), int(grid)))
    _check(workspace is not None and workspace.is_cuda and workspace.numel() >= need,
           f"linear_streamk: needs a zeroed workspace of {need} bytes (ops.streamk_workspace)")
    _ops().gemm_sk_bf16(x2.data_ptr(), K, w.data_ptr(), K, out.data_ptr(), N, _ptr(bias), _ptr(residual), N, M, N,
                        K, 1.0, ACT_CODE[act], workspace.data_ptr(), int(grid), int(tile), _stream())
    return out
