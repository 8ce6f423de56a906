"""GEMMs with LayerNorm folded into their operands or epilogue (``gemm_ln.hip``,
``gemm_rowln.hip``): deferred, staged, residual + LayerNorm output, full-row."""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

from ._common import ACT_CODE, _act_ref, _aligned, _check, _ops, _ptr, _stream
from .tiles import NUM_LN_TILE_CFGS, STG_TILE_CFGS
from .tuning import _TUNE, _tuned_cfg

LN_LNA, LN_LNR, LN_STATS, LN_SELF = 1, 2, 4, 8
LN_STG = 32            # gemm_core.h EPI_STG: staged LayerNorm epilogues with per-N-tile partial statistics
_PSTATS_MAX = 16       # partials per row a producer may write (N / smallest staged BN, N = 768: 768 / 48)


def _pstats_layout(st: torch.Tensor, M: int, what: str):
    """(row stride in floats, partials per row) of a [M, P, 2] f32 partial-statistics view."""
    _check(st.dtype == torch.float32 and st.dim() == 3 and st.shape[0] == M and st.shape[2] == 2
           and st.stride(2) == 1 and st.stride(1) == 2 and st.stride(0) % 2 == 0 and _aligned(st, 8),
           f"{what}: partial statistics must be a [M, P, 2] f32 row-strided view")
    return st.stride(0), st.shape[1]


def _stats_ld(st: torch.Tensor, M: int, what: str) -> int:
    _check(st.dtype == torch.float32 and st.dim() == 2 and st.shape[0] == M and st.shape[1] >= 2
           and st.stride(1) == 1 and st.stride(0) % 2 == 0 and _aligned(st, 8), f"linear_ln: bad {what} stats")
    return st.stride(0)


def linear_ln_staged(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: str = "none",
                     residual: Optional[torch.Tensor] = None, lna: Optional[tuple] = None,
                     lnr: Optional[tuple] = None, pstats: bool = False, out: Optional[torch.Tensor] = None,
                     tile_cfg: int = -1, max_parts: int = _PSTATS_MAX):
    """The deferred-LayerNorm GEMM on the STAGED epilogue with partial statistics
    (gemm_core.h EPI_STG; ping-pong and 4-wave tiles):

    * ``lna=(stats, colsum, bias_f32, D, eps)``: x holds RAW rows whose LayerNorm
      is folded into w (``fold_ln_weights``); ``stats`` [M, P, 2] f32 = the
      producer's per-N-tile partial (sum, sum of squares) of every row.
      y = act(LN(x) @ W.T + b); no ``bias`` / ``residual``.
    * ``lnr=(stats, gamma, beta, D, eps)``: ``residual`` holds RAW rows (partials
      ``stats``), added as LayerNorm(residual).
    * ``pstats=True``: also returns this GEMM's output statistics as partials
      [M, P, 2] (P = N-tiles of the tile it ran): ``(out, stats)``.  No zeroing,
      no atomics: each N-tile writes its own partial.  ``max_parts``: only tiles
      with at most that many N-tiles (a consumer's limit, e.g. 8 for
      ``qkv_attention(a_stats=...)``).
    """
    _check(x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16, "linear_ln_staged: bf16 on the GPU")
    _check(w.dim() == 2 and w.is_contiguous(), "linear_ln_staged: w must be a contiguous [N, K] matrix")
    N, K = w.shape
    _check(x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == K, "linear_ln_staged: x must be a 2-D [M, K] view")
    M, lda = x.shape[0], x.stride(0)
    _check(K % 8 == 0 and lda % 8 == 0 and N % 8 == 0 and _aligned(x) and _aligned(w), "linear_ln_staged: alignment")
    _check(act != "swiglu", "linear_ln_staged: no swiglu")
    mode = LN_STG | (LN_LNA if lna is not None else 0) | (LN_LNR if lnr is not None else 0) | \
        (LN_STATS if pstats else 0)
    _check(mode in (LN_STG | LN_LNA, LN_STG | LN_STATS, LN_STG | LN_LNR | LN_STATS, LN_STG | LN_LNR),
           "linear_ln_staged: modes are lna, pstats, lnr + pstats, lnr")
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=x.dtype)
    _check(out.is_contiguous() and out.shape == (M, N) and _aligned(out), "linear_ln_staged: bad out")
    if bias is not None:
        _check(bias.is_contiguous() and bias.numel() == N and bias.dtype == x.dtype, "linear_ln_staged: bad bias")
    ldr = 0
    if residual is not None:
        _check(residual.dim() == 2 and residual.shape == (M, N) and residual.stride(1) == 1
               and residual.stride(0) % 8 == 0 and residual.dtype == x.dtype and _aligned(residual),
               "linear_ln_staged: bad residual")
        ldr = residual.stride(0)
    a_st = a_cs = a_b = r_st = r_g = r_b = None
    a_ld = r_ld = 0
    a_parts = r_parts = 1
    a_inv = r_inv = 0.0
    eps = 0.0
    if lna is not None:
        a_st, a_cs, a_b, d, eps = lna
        a_ld, a_parts = _pstats_layout(a_st, M, "lna")
        _check(a_cs.dtype == torch.float32 and a_cs.numel() == N and a_cs.is_contiguous()
               and a_b.dtype == torch.float32 and a_b.numel() == N and a_b.is_contiguous(),
               "linear_ln_staged: bad lna vectors")
        a_inv = 1.0 / d
    if lnr is not None:
        _check(residual is not None, "linear_ln_staged: lnr needs the residual")
        r_st, r_g, r_b, d, eps = lnr
        r_ld, r_parts = _pstats_layout(r_st, M, "lnr")
        _check(r_g.numel() == N and r_b.numel() == N and r_g.dtype == x.dtype and r_b.dtype == x.dtype
               and r_g.is_contiguous() and r_b.is_contiguous(), "linear_ln_staged: bad lnr gamma/beta")
        r_inv = 1.0 / d
    o_buf = None
    if pstats:
        o_buf = torch.empty(M, _PSTATS_MAX, 2, device=x.device, dtype=torch.float32)
    fn = _ops().gemm_tn_ln

    def launch(c):
        fn(x.data_ptr(), lda, w.data_ptr(), K, out.data_ptr(), N, _ptr(bias), _ptr(residual), ldr, M, N, K, 1.0,
           ACT_CODE[act], mode, _ptr(a_st), a_ld, _ptr(a_cs), _ptr(a_b), _ptr(r_st), r_ld, _ptr(r_g), _ptr(r_b),
           _ptr(o_buf), 2 * _PSTATS_MAX if pstats else 0, float(a_inv), float(r_inv), float(eps), _stream(), c,
           0, 0, a_parts, r_parts)

    def parts(c):
        return -(-N // int(_ops().gemm_tile_bn(int(_ops().gemm_stg_cfg(int(c))))))

    cands = [c for c in STG_TILE_CFGS if not pstats or parts(c) <= max_parts]
    _check(len(cands) > 0, f"linear_ln_staged: no tile writes <= {max_parts} partials for N = {N}")
    if tile_cfg < 0:
        key = ("gemm_stg", x.dtype, M, N, K, lda, act, mode, a_parts, r_parts) + \
            ((max_parts,) if pstats and max_parts < _PSTATS_MAX else ())
        tile_cfg = _tuned_cfg(key, launch, cands)
    tile_cfg = int(_ops().gemm_stg_cfg(int(tile_cfg)))
    if tile_cfg not in cands:
        tile_cfg = int(_ops().gemm_stg_cfg(int(cands[0])))
    launch(tile_cfg)
    if not pstats:
        return out
    bn = int(_ops().gemm_tile_bn(tile_cfg))
    return out, o_buf[:, : -(-N // bn), :]


def linear_ln(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: str = "none",
              residual: Optional[torch.Tensor] = None, lna: Optional[tuple] = None, lnr: Optional[tuple] = None,
              out_stats: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              tile_cfg: int = -1) -> torch.Tensor:
    """GEMM with the deferred-LayerNorm epilogues (bf16; ``gemm_ln.hip``).

    * ``lna=(stats, colsum, bias_f32, D, eps)``: x holds RAW rows whose LayerNorm
      is folded into w (w = W * gamma, colsum = w.float().sum(1), bias_f32 =
      b + W @ beta); ``stats`` [M, 2] f32 = per-row (sum, sum of squares).
      y = act(LN(x) @ W.T + b); ``bias`` must be None.  ``stats=None``: the
      GEMM computes x's row statistics itself in its main loop (no producer
      pass) and, if ``out_stats`` is given, STORES them there (for a later
      ``lnr`` of the same rows) -- ``out_stats`` needs no zeroing in this mode.
    * ``lnr=(stats, gamma, beta, D, eps)``: ``residual`` holds raw rows and is
      added as LayerNorm(residual) (normalised on load).
    * ``out_stats`` [M, 2] f32: += per-row (sum, sum of squares) of the stored y
      (must be zeroed by the caller before the first producer writes it).
    """
    _check(x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16, "linear_ln: bf16 on the GPU")
    _check(w.dim() == 2 and w.is_contiguous(), "linear_ln: w must be a contiguous [N, K] matrix")
    N, K = w.shape
    _check(x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == K, "linear_ln: x must be a 2-D [M, K] (row-strided) view")
    M, lda = x.shape[0], x.stride(0)
    _check(K % 8 == 0 and lda % 8 == 0 and N % 4 == 0 and _aligned(x) and _aligned(w), "linear_ln: alignment")
    _check(act != "swiglu", "linear_ln: no swiglu")
    self_stats = lna is not None and lna[0] is None
    if self_stats:
        mode = LN_LNA | LN_SELF
        _check(lnr is None, "linear_ln: lna with in-kernel statistics takes no lnr")
    else:
        mode = (LN_LNA if lna is not None else 0) | (LN_LNR if lnr is not None else 0) | \
            (LN_STATS if out_stats is not None else 0)
    _check(mode in (LN_LNA, LN_STATS, LN_LNR | LN_STATS, LN_LNR, LN_LNA | LN_SELF),
           "linear_ln: modes are lna, out_stats, lnr, lnr + out_stats, or lna with in-kernel statistics")
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=x.dtype)
    _check(out.is_contiguous() and out.shape == (M, N), "linear_ln: bad out")
    if bias is not None:
        _check(bias.is_contiguous() and bias.numel() == N and bias.dtype == x.dtype, "linear_ln: bad bias")
    ldr = 0
    if residual is not None:
        _check(residual.dim() == 2 and residual.shape == (M, N) and residual.stride(1) == 1
               and residual.stride(0) % 4 == 0 and residual.dtype == x.dtype and _aligned(residual, 8),
               "linear_ln: bad residual")
        ldr = residual.stride(0)
    a_st = a_cs = a_b = r_st = r_g = r_b = o_st = None
    a_ld = r_ld = o_ld = 0
    a_inv = r_inv = 0.0
    eps = 0.0
    if lna is not None:
        a_st, a_cs, a_b, d, eps = lna
        a_ld = 0 if a_st is None else _stats_ld(a_st, M, "lna")
        _check(a_cs.dtype == torch.float32 and a_cs.numel() == N and a_cs.is_contiguous()
               and a_b.dtype == torch.float32 and a_b.numel() == N and a_b.is_contiguous(), "linear_ln: bad lna vectors")
        a_inv = 1.0 / d
    if lnr is not None:
        _check(residual is not None, "linear_ln: lnr needs the residual")
        r_st, r_g, r_b, d, eps_r = lnr
        r_ld = _stats_ld(r_st, M, "lnr")
        _check(r_g.numel() == N and r_b.numel() == N and r_g.dtype == x.dtype and r_b.dtype == x.dtype
               and r_g.is_contiguous() and r_b.is_contiguous(), "linear_ln: bad lnr gamma/beta")
        _check(lna is None or eps_r == eps, "linear_ln: one eps")
        r_inv, eps = 1.0 / d, eps_r
    if out_stats is not None:
        o_ld = _stats_ld(out_stats, M, "out")
    args = (x.data_ptr(), lda, w.data_ptr(), K, out.data_ptr(), N, _ptr(bias), _ptr(residual), ldr, M, N, K, 1.0,
            ACT_CODE[act], mode, _ptr(a_st), a_ld, _ptr(a_cs), _ptr(a_b), _ptr(r_st), r_ld, _ptr(r_g), _ptr(r_b),
            _ptr(out_stats), o_ld, float(a_inv), float(r_inv), float(eps))
    fn = _ops().gemm_tn_ln
    if tile_cfg < 0:
        key = ("gemm_ln", x.dtype, M, N, K, lda, act, mode)
        tuned = key in _TUNE
        tile_cfg = _tuned_cfg(key, lambda c: fn(*args, _stream(), c), range(NUM_LN_TILE_CFGS))
        if not tuned and mode & LN_STATS and not torch.cuda.is_current_stream_capturing():
            out_stats.zero_()        # the tuning launches accumulated into it
    fn(*args, _stream(), int(tile_cfg))
    return out


def fold_ln_weights(w: torch.Tensor, b: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor):
    """(w', colsum, bias_f32) for ``linear_ln(lna=...)``: LN(x) @ w.T + b ==
    rstd * (x @ w'.T - mean * colsum) + bias_f32 with w' = w * gamma."""
    wf = w.float()
    w2 = (wf * gamma.float()[None, :]).to(w.dtype).contiguous()
    return w2, w2.float().sum(1).contiguous(), (b.float() + wf @ beta.float()).contiguous()


def linear_ln_ref(x, w, bias=None, act="none", residual=None, ln_x=None, ln_res=None, eps=1e-12):
    """fp32 reference of linear_ln in terms of the UNFOLDED LayerNorms:
    act(LN_x(x) @ w.T + bias + LN_res(residual)); ln_* = (gamma, beta) or None."""
    xf = x.float()
    if ln_x is not None:
        xf = F.layer_norm(xf, (xf.shape[-1],), ln_x[0].float(), ln_x[1].float(), eps)
    y = xf @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    if residual is not None:
        rf = residual.float()
        if ln_res is not None:
            rf = F.layer_norm(rf, (rf.shape[-1],), ln_res[0].float(), ln_res[1].float(), eps)
        y = y + rf
    return _act_ref(y, act)


LN_OUT = 16
_LNOUT_ERR: Dict[int, torch.Tensor] = {}


def _lnout_err(dev: torch.device) -> torch.Tensor:
    i = dev.index if dev.index is not None else torch.cuda.current_device()
    if i not in _LNOUT_ERR:
        _LNOUT_ERR[i] = torch.zeros(1, device=dev, dtype=torch.int32)
    return _LNOUT_ERR[i]


def ln_out_error(device=None, reset: bool = True) -> bool:
    """True if a ``linear_residual_ln`` row-panel wait timed out on ``device``
    since the last reset (its output is then wrong; the kernel never hangs)."""
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    e = _lnout_err(dev)
    bad = bool(e.item())
    if reset and bad:
        e.zero_()
    return bad


def linear_residual_ln(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, residual: torch.Tensor,
                       gamma: torch.Tensor, beta: torch.Tensor, eps: float, stats_ws: torch.Tensor,
                       panel_ws: torch.Tensor, out: Optional[torch.Tensor] = None, tile_cfg: int = -1) -> torch.Tensor:
    """y = LayerNorm(x @ w.T + bias + residual) * gamma + beta in ONE GEMM (bf16;
    gemm_core.h EPI_LNOUT): the blocks of a row panel reduce the row statistics
    through ``stats_ws`` (f32 [M, 2]) and ``panel_ws`` (int32, >= M entries),
    which must be ZERO at launch (one use per zeroing: models/bert.py zeroes a
    forward's workspaces in its embedding kernel).  The post-LN transformer's
    o-proj -> LN1 and FFN-down -> LN2 without a LayerNorm kernel or the pre-LN
    activation round trip."""
    _check(x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == x.dtype, "linear_residual_ln: bf16 on the GPU")
    _check(w.dim() == 2 and w.is_contiguous(), "linear_residual_ln: w must be a contiguous [N, K] matrix")
    N, K = w.shape
    _check(x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == K, "linear_residual_ln: x must be a 2-D [M, K] view")
    M, lda = x.shape[0], x.stride(0)
    _check(K % 8 == 0 and lda % 8 == 0 and N % 8 == 0 and _aligned(x) and _aligned(w), "linear_residual_ln: alignment")
    _check(bias.is_contiguous() and bias.numel() == N and bias.dtype == x.dtype, "linear_residual_ln: bad bias")
    _check(residual.dim() == 2 and residual.shape == (M, N) and residual.stride(1) == 1 and residual.stride(0) % 8 == 0
           and residual.dtype == x.dtype and _aligned(residual), "linear_residual_ln: bad residual")
    for v in (gamma, beta):
        _check(v.is_contiguous() and v.numel() == N and v.dtype == x.dtype and _aligned(v), "linear_residual_ln: gamma/beta")
    _check(stats_ws.dtype == torch.float32 and stats_ws.is_contiguous() and stats_ws.numel() >= 2 * M
           and _aligned(stats_ws, 8), "linear_residual_ln: stats_ws must be contiguous f32 [M, 2]")
    _check(panel_ws.dtype == torch.int32 and panel_ws.is_contiguous() and panel_ws.numel() >= M,
           "linear_residual_ln: panel_ws must be contiguous int32 with >= M entries")
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=x.dtype)
    _check(out.is_contiguous() and out.shape == (M, N) and _aligned(out), "linear_residual_ln: bad out")
    err = _lnout_err(x.device)
    fn = _ops().gemm_tn_ln

    def launch(c):
        fn(x.data_ptr(), lda, w.data_ptr(), K, out.data_ptr(), N, bias.data_ptr(), residual.data_ptr(),
           residual.stride(0), M, N, K, 1.0, 0, LN_OUT, 0, 0, 0, 0, 0, 0, gamma.data_ptr(), beta.data_ptr(),
           stats_ws.data_ptr(), 2, 0.0, 1.0 / N, float(eps), _stream(), int(c), panel=panel_ws.data_ptr(),
           err=err.data_ptr())

    if tile_cfg < 0:
        key = ("gemm_lnout", M, N, K, lda)
        tuned = key in _TUNE
        tile_cfg = _tuned_cfg(key, launch, range(NUM_LN_TILE_CFGS))
        if not tuned and not torch.cuda.is_current_stream_capturing():
            stats_ws.zero_()         # the tuning launches used (and left) the workspaces
            panel_ws.zero_()
    launch(tile_cfg)
    return out


def linear_rowln_supported(M: int, N: int, K: int) -> bool:
    """Shapes the full-row GEMM + LayerNorm kernel (``gemm_rowln.hip``) takes."""
    return N == 768 and K % 32 == 0 and M > 0


def pack_rowln_weight(w: torch.Tensor) -> torch.Tensor:
    """[N, K] weight -> the k-tile-major [K/32, N, 32] layout ``linear_rowln`` reads
    (each 32-wide k-step of all N rows contiguous).  Done once per weight."""
    N, K = w.shape
    _check(K % 32 == 0, "pack_rowln_weight: K must be a multiple of 32")
    return w.reshape(N, K // 32, 32).permute(1, 0, 2).contiguous()


def linear_rowln(x: torch.Tensor, wp: torch.Tensor, bias: torch.Tensor, residual: torch.Tensor,
                 gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = LayerNorm(x @ w.T + bias + residual) * gamma + beta (bf16, N = 768) in ONE
    kernel whose 64-row blocks own whole output rows (``gemm_rowln.hip``): the row
    statistics never leave the block -- no workspace, no zeroing, no cross-block
    wait, no LayerNorm launch.  ``wp`` = ``pack_rowln_weight(w)``.  The post-LN
    transformer's o-proj -> LN1 and FFN-down -> LN2."""
    _check(x.is_cuda and x.dtype == torch.bfloat16 and wp.dtype == x.dtype, "linear_rowln: bf16 on the GPU")
    _check(wp.dim() == 3 and wp.shape[2] == 32 and wp.is_contiguous(),
           "linear_rowln: wp must be pack_rowln_weight(w), [K/32, N, 32]")
    N, K = wp.shape[1], wp.shape[0] * 32
    _check(x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == K, "linear_rowln: x must be a 2-D [M, K] view")
    M, lda = x.shape[0], x.stride(0)
    _check(linear_rowln_supported(M, N, K), f"linear_rowln: unsupported shape M={M} N={N} K={K}")
    _check(lda % 8 == 0 and _aligned(x) and _aligned(wp), "linear_rowln: x / w rows must be 16-byte aligned")
    _check(bias.is_contiguous() and bias.numel() == N and bias.dtype == x.dtype and _aligned(bias, 8),
           "linear_rowln: bad bias")
    _check(residual.dim() == 2 and residual.shape == (M, N) and residual.stride(1) == 1
           and residual.stride(0) % 4 == 0 and residual.dtype == x.dtype and _aligned(residual, 8),
           "linear_rowln: bad residual")
    for v in (gamma, beta):
        _check(v.is_contiguous() and v.numel() == N and v.dtype == x.dtype and _aligned(v, 8), "linear_rowln: gamma/beta")
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=x.dtype)
    _check(out.dim() == 2 and out.shape == (M, N) and out.stride(1) == 1 and out.stride(0) % 4 == 0
           and _aligned(out, 8), "linear_rowln: bad out")
    _ops().gemm_rowln(x.data_ptr(), lda, wp.data_ptr(), bias.data_ptr(), residual.data_ptr(), residual.stride(0),
                      gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), out.stride(0), M, N, K, float(eps), _stream())
    return out


def linear_residual_ln_ref(x, w, bias, residual, gamma, beta, eps=1e-12):
    y = x.float() @ w.float().t() + bias.float() + residual.float()
    return F.layer_norm(y, (y.shape[-1],), gamma.float(), beta.float(), eps).to(x.dtype)
