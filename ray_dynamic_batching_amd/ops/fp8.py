"""FP8 (OCP e4m3fn) W8A8: per-row activation scales, per-output-channel weight
scales, both f32 and applied in the GEMM epilogue (quant_fp8.hip, gemm_fp8.hip)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from ._common import ACT_CODE, DTYPE_CODE, _act_ref, _aligned, _check, _ops, _ptr, _stream

FP8_MAX = 448.0          # largest finite e4m3fn
FP8_DTYPE = torch.float8_e4m3fn


def _fp8_rows(x: torch.Tensor, what: str):
    """x as (rows, K, row stride): contiguous [..., K] or a 2-D row-strided view."""
    K = x.shape[-1]
    if x.is_contiguous():
        return x.numel() // K, K, K
    _check(x.dim() == 2 and x.stride(1) == 1, f"{what}: x must be contiguous or a 2-D row-strided view")
    return x.shape[0], K, x.stride(0)


def quantize_fp8_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-row dynamic quantisation: (q float8_e4m3fn [..., K], scale f32 [rows]),
    scale = amax(|row|) / 448 (1 for an all-zero row), q = clamp(x / scale, +-448)."""
    _check(x.is_cuda and x.dtype in (torch.bfloat16, torch.float16), "quantize_fp8_rows: bf16/f16 GPU tensor")
    rows, K, ldx = _fp8_rows(x, "quantize_fp8_rows")
    _check(K % 16 == 0 and K > 0, "quantize_fp8_rows: K must be a multiple of 16")
    _check(ldx % 8 == 0 and _aligned(x), "quantize_fp8_rows: rows must be 16-byte aligned")
    q = torch.empty(x.shape, device=x.device, dtype=FP8_DTYPE)
    scale = torch.empty(rows, device=x.device, dtype=torch.float32)
    _ops().quant_fp8_rows(DTYPE_CODE[x.dtype], x.data_ptr(), ldx, q.data_ptr(), scale.data_ptr(), rows, K, _stream())
    return q, scale


def rms_norm_fp8(x, gamma, eps=1e-5, residual=None, residual_out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``quantize_fp8_rows(rms_norm(x [+ residual]))`` in one kernel, quantising the
    normalised f32 row directly (no 16-bit rounding in between)."""
    _check(x.is_cuda and x.dtype in (torch.bfloat16, torch.float16), "rms_norm_fp8: bf16/f16 GPU tensor")
    rows, D, ldx = _fp8_rows(x, "rms_norm_fp8")
    _check(ldx == D or residual is None, "rms_norm_fp8: a row-strided x takes no residual")
    _check(D % 16 == 0 and 0 < D <= 4096, "rms_norm_fp8: D must be a multiple of 16, <= 4096")
    _check(ldx % 8 == 0 and _aligned(x), "rms_norm_fp8: rows must be 16-byte aligned")
    _check(gamma.numel() == D and gamma.dtype == x.dtype and gamma.is_contiguous() and _aligned(gamma),
           "rms_norm_fp8: bad gamma")
    if residual is not None:
        _check(residual.shape == x.shape and residual.is_contiguous() and residual.dtype == x.dtype
               and _aligned(residual), "rms_norm_fp8: bad residual")
    if residual_out is not None:
        _check(residual is not None and residual_out.shape == x.shape and residual_out.is_contiguous()
               and residual_out.dtype == x.dtype and _aligned(residual_out), "rms_norm_fp8: bad residual_out")
    q = torch.empty(x.shape, device=x.device, dtype=FP8_DTYPE)
    scale = torch.empty(rows, device=x.device, dtype=torch.float32)
    _ops().rms_norm_fp8(DTYPE_CODE[x.dtype], x.data_ptr(), _ptr(residual), _ptr(residual_out), gamma.data_ptr(),
                        q.data_ptr(), scale.data_ptr(), rows, D, ldx, float(eps), _stream())
    return q, scale


def fp8_num_tiles() -> int:
    """Block tiles of the FP8 GEMM: ``linear_fp8(tile_cfg=i)`` for i in range(n)."""
    return int(_ops().gemm_fp8_num_tiles())


_FP8_ACTS = ("none", "gelu", "silu", "swiglu")


def linear_fp8(xq: torch.Tensor, x_scale: torch.Tensor, wq: torch.Tensor, w_scale: torch.Tensor,
               bias: Optional[torch.Tensor] = None, act: str = "none", residual: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.bfloat16,
               tile_cfg: int = -1) -> torch.Tensor:
    """y = act((xq @ wq.T) * x_scale[m] * w_scale[n] + bias) + residual with e4m3
    operands and f32 accumulation.  xq: [..., K] or a 2-D row-strided view, wq:
    [N, K] contiguous; K % 128 == 0, N % 8 == 0.  act="swiglu" expects wq rows
    interleaved (gate, up) and returns N/2 columns.  bias / residual are bf16 or
    f16 (the output dtype when that is 16-bit).  ``tile_cfg`` = -1: static rule on
    (M, N); 0 .. fp8_num_tiles() - 1 forces a block tile."""
    _check(xq.is_cuda and wq.is_cuda, "linear_fp8: tensors must be on the GPU")
    _check(xq.dtype == FP8_DTYPE and wq.dtype == FP8_DTYPE, "linear_fp8: float8_e4m3fn operands")
    _check(act in _FP8_ACTS, f"linear_fp8: act must be one of {_FP8_ACTS}")
    _check(out_dtype in DTYPE_CODE, "linear_fp8: out_dtype must be bf16, f16 or f32")
    _check(wq.dim() == 2 and wq.is_contiguous(), "linear_fp8: wq must be a contiguous [N, K] matrix")
    N, K = wq.shape
    _check(xq.shape[-1] == K, f"linear_fp8: K mismatch {tuple(xq.shape)} vs {tuple(wq.shape)}")
    _check(K % 128 == 0 and K > 0, "linear_fp8: K must be a multiple of 128")
    _check(N % 8 == 0 and N > 0, "linear_fp8: N must be a multiple of 8")
    if xq.dim() == 2 and xq.stride(1) == 1:
        x2, lead = xq, (xq.shape[0],)
    else:
        _check(xq.is_contiguous(), "linear_fp8: xq must be contiguous (or a 2-D row-strided view)")
        lead = tuple(xq.shape[:-1])
        x2 = xq.reshape(-1, K)
    M = x2.shape[0]
    lda = x2.stride(0)
    _check(M >= 1, "linear_fp8: empty input")
    _check(lda % 16 == 0 and _aligned(x2) and _aligned(wq), "linear_fp8: rows must be 16-byte aligned")
    _check(M * lda < 2 ** 31 and N * K < 2 ** 31, "linear_fp8: operand larger than 2 GiB")
    for s, n, what in ((x_scale, M, "x_scale"), (w_scale, N, "w_scale")):
        _check(s.is_cuda and s.dtype == torch.float32 and s.is_contiguous() and s.numel() == n and _aligned(s),
               f"linear_fp8: {what} must be {n} contiguous f32 values")
    n_out = N // 2 if act == "swiglu" else N
    if out is None:
        out = torch.empty(*lead, n_out, device=xq.device, dtype=out_dtype)
    _check(out.is_cuda and out.dtype in DTYPE_CODE and out.is_contiguous() and out.shape[-1] == n_out
           and out.numel() == M * n_out and _aligned(out), "linear_fp8: bad out")
    aux = None
    for t, what in ((bias, "bias"), (residual, "residual")):
        if t is None:
            continue
        _check(t.is_cuda and t.dtype in (torch.bfloat16, torch.float16) and t.is_contiguous() and _aligned(t),
               f"linear_fp8: {what} must be a contiguous bf16/f16 tensor")
        _check(aux is None or aux == t.dtype, "linear_fp8: bias and residual of equal dtype")
        aux = t.dtype
    if out.dtype != torch.float32:
        _check(aux is None or aux == out.dtype, "linear_fp8: bias / residual must have the 16-bit output dtype")
        aux = out.dtype
    if bias is not None:
        _check(bias.numel() == N, "linear_fp8: bad bias")
    if residual is not None:
        _check(residual.numel() == M * n_out and residual.shape[-1] == n_out, "linear_fp8: bad residual")
    nt = fp8_num_tiles()
    _check(-1 <= int(tile_cfg) < nt, f"linear_fp8: tile_cfg must be -1 or 0..{nt - 1}")
    _ops().gemm_fp8(DTYPE_CODE[out.dtype], DTYPE_CODE[aux or torch.bfloat16], x2.data_ptr(), lda, wq.data_ptr(), K,
                    x_scale.data_ptr(), w_scale.data_ptr(), out.data_ptr(), n_out, _ptr(bias), _ptr(residual), n_out,
                    M, N, K, ACT_CODE[act], int(tile_cfg), _stream())
    return out


def linear_w8a8(x: torch.Tensor, wq: torch.Tensor, w_scale: torch.Tensor, **kw) -> torch.Tensor:
    """``linear_fp8`` of a 16-bit activation quantised per row on the fly."""
    kw.setdefault("out_dtype", x.dtype)
    xq, xs = quantize_fp8_rows(x)
    return linear_fp8(xq, xs, wq, w_scale, **kw)


def _fp8_quant_f32(xf: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The scale rule and clamp shared by activations and weights (plain torch, f32 in)."""
    amax = xf.abs().amax(dim=-1)
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    q = (xf / scale.unsqueeze(-1)).clamp(-FP8_MAX, FP8_MAX).to(FP8_DTYPE)
    return q, scale


def quantize_weight_fp8(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """w [N, K] -> (wq float8_e4m3fn [N, K], w_scale f32 [N]): one scale per output
    row, the activation quantiser's rule.  Plain torch (CPU or GPU): model build / load time."""
    _check(w.dim() == 2, "quantize_weight_fp8: w must be [N, K]")
    q, scale = _fp8_quant_f32(w.float())
    return q.contiguous(), scale.contiguous()


def quantize_fp8_rows_ref(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    q, scale = _fp8_quant_f32(x.float())
    return q, scale.reshape(-1)


def rms_norm_fp8_ref(x, gamma, eps=1e-5, residual=None) -> Tuple[torch.Tensor, torch.Tensor]:
    xf = x.float() + (residual.float() if residual is not None else 0)
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * gamma.float()
    q, scale = _fp8_quant_f32(y)
    return q, scale.reshape(-1)


def linear_fp8_ref(xq, x_scale, wq, w_scale, bias=None, act="none", residual=None, out_dtype=torch.bfloat16):
    """Both operands dequantised to f32, matmul, then scales, bias, activation, residual."""
    y = xq.float() @ wq.float().t()
    y = y * x_scale.float().reshape(*y.shape[:-1], 1) * w_scale.float()
    if bias is not None:
        y = y + bias.float()
    if act == "swiglu":
        y = F.silu(y[..., 0::2]) * y[..., 1::2]
    else:
        y = _act_ref(y, act)
    if residual is not None:
        y = y + residual.float()
    return y.to(out_dtype)
