"""Transformer-side kernels: embeddings, sequence lengths, attention, the fused
QKV projection + attention, RoPE, the softmax + top-k head, row gather."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from ._common import DTYPE_CODE, _aligned, _check, _ops, _ptr, _stream
from .gemm_ln import _pstats_layout
from .tuning import _tuned_cfg


def embed_ln(ids, word, pos, typ, gamma, beta, eps=1e-12, types=None, zero_stats=None):
    """BERT embeddings: LN(word[ids] + pos[t % S] + type[types or 0]); ids [B, S] int32.
    ``zero_stats`` [..., B*S, 2] f32 (contiguous): also zeroed (the deferred-LN
    row statistics of the folded forward), saving a fill kernel."""
    _check(ids.dtype == torch.int32 and ids.is_contiguous() and ids.dim() == 2, "embed_ln: ids must be [B, S] int32")
    B, S = ids.shape
    D = word.shape[1]
    _check(pos.shape[0] >= S and pos.shape[1] == D and typ.shape[1] == D, "embed_ln: table shapes")
    _check(D % 256 == 0, "embed_ln: hidden size must be a multiple of 256")
    if types is not None:
        _check(types.dtype == torch.int32 and types.shape == ids.shape and types.is_contiguous(), "embed_ln: bad types")
    zn = 0
    if zero_stats is not None:
        _check(zero_stats.dtype == torch.float32 and zero_stats.is_contiguous() and zero_stats.shape[-1] == 2
               and zero_stats.shape[-2] == B * S, "embed_ln: zero_stats must be [..., B*S, 2] f32")
        zn = zero_stats.numel() // (2 * B * S)
    y = torch.empty(B * S, D, device=ids.device, dtype=word.dtype)
    _ops().embed_ln_fwd(DTYPE_CODE[word.dtype], ids.data_ptr(), _ptr(types), word.data_ptr(), pos.data_ptr(),
                        typ.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), B * S, S, D,
                        word.shape[0], float(eps), _ptr(zero_stats), zn, B * S, _stream())
    return y


def embed_ln_ref(ids, word, pos, typ, gamma, beta, eps=1e-12, types=None):
    B, S = ids.shape
    idl = ids.long().clamp(0, word.shape[0] - 1)
    x = word.float()[idl] + pos.float()[:S][None] + typ.float()[(types.long() if types is not None else torch.zeros_like(idl))]
    return F.layer_norm(x, (word.shape[1],), gamma.float(), beta.float(), eps).to(word.dtype).reshape(B * S, -1)


def seq_lens(ids: torch.Tensor, pad_id: int = 0) -> torch.Tensor:
    """int32 [B]: number of non-pad ids per row of ``ids`` [B, S] int32 (min 1)."""
    _check(ids.is_cuda and ids.dtype == torch.int32 and ids.dim() == 2 and ids.is_contiguous(), "seq_lens: ids")
    B, S = ids.shape
    lens = torch.empty(B, device=ids.device, dtype=torch.int32)
    _ops().seq_lens(ids.data_ptr(), B, S, int(pad_id), lens.data_ptr(), _stream())
    return lens


def seq_lens_ref(ids, pad_id=0):
    return (ids != pad_id).sum(dim=1, dtype=torch.int32).clamp_(min=1)


# ---------------------------------------------------------------------------
# Attention
# ---------------------------------------------------------------------------
def attention(qkv: torch.Tensor, B: int, S: int, H: int, Hkv: int, D: int, lens: Optional[torch.Tensor] = None,
              causal: bool = False, scale: Optional[float] = None, out: Optional[torch.Tensor] = None,
              q_off: int = 0, k_off: Optional[int] = None, v_off: Optional[int] = None) -> torch.Tensor:
    """Fused MHA / GQA on the packed projection output qkv [B*S, ld] (q | k | v)."""
    _check(qkv.is_cuda and qkv.dtype in (torch.bfloat16, torch.float16) and qkv.dim() == 2 and qkv.stride(1) == 1,
           "attention: bad qkv")
    _check(qkv.shape[0] == B * S, "attention: qkv rows must be B*S")
    _check(D in (64, 128), "attention: head dim must be 64 or 128")
    _check(H % Hkv == 0, "attention: H % Hkv")
    k_off = H * D if k_off is None else k_off
    v_off = (H + Hkv) * D if v_off is None else v_off
    ld = qkv.stride(0)
    _check(max(q_off + H * D, k_off + Hkv * D, v_off + Hkv * D) <= qkv.shape[1], "attention: offsets exceed row")
    _check(ld % 8 == 0 and q_off % 8 == 0 and k_off % 8 == 0 and v_off % 8 == 0 and _aligned(qkv), "attention: alignment")
    if lens is not None:
        _check(lens.dtype == torch.int32 and lens.numel() == B and lens.is_cuda, "attention: lens must be int32 [B]")
    if out is None:
        out = torch.empty(B * S, H * D, device=qkv.device, dtype=qkv.dtype)
    _check(out.is_contiguous() and out.shape == (B * S, H * D), "attention: bad out")
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    _ops().attn_fwd(DTYPE_CODE[qkv.dtype], qkv.data_ptr(), ld, q_off, k_off, v_off, B, H, Hkv, S, D, _ptr(lens), int(causal),
                    out.data_ptr(), H * D, float(scale), _stream())
    return out


NUM_QKV_ATTN_CFGS = 5   # qkv_attention.hip: 8 waves (4x2) x 3 stages, 8 (4x2) x 2, 4 x 2, 8 (2x4) x 2, two sequences per block (S == 128)
QKV_ATTN_MAX_S = 128


def pack_qkv_heads(w: torch.Tensor, b: torch.Tensor, H: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """[q | k | v] projection rows (nn.Linear [3*H*D, K] layout) -> head-major
    [H*3*D, K]: rows h*3D + [0,D) = q_h, [D,2D) = k_h, [2D,3D) = v_h (and the
    bias likewise) -- the operand layout of ``qkv_attention``."""
    N, K = w.shape
    _check(N % (3 * H) == 0 and b.numel() == N, "pack_qkv_heads: rows must be 3*H*D")
    D = N // (3 * H)
    wp = w.view(3, H, D, K).transpose(0, 1).reshape(N, K).contiguous()
    bp = b.view(3, H, D).transpose(0, 1).reshape(N).contiguous()
    return wp, bp


def pack_qkv_vec(v: torch.Tensor, H: int) -> torch.Tensor:
    """A per-output-row vector of the [q | k | v] projection (bias, folded
    colsum / bias) in ``pack_qkv_heads`` order."""
    N = v.numel()
    _check(N % (3 * H) == 0, "pack_qkv_vec: length must be 3*H*D")
    return v.view(3, H, N // (3 * H)).transpose(0, 1).reshape(N).contiguous()


def qkv_attention_supported(S: int, H: int, D: int, K: int) -> bool:
    return 1 <= S <= QKV_ATTN_MAX_S and D == 64 and K % 8 == 0


def qkv_attention(x: torch.Tensor, w_packed: torch.Tensor, b_packed: Optional[torch.Tensor], B: int, S: int, H: int,
                  lens: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                  out: Optional[torch.Tensor] = None, cfg: int = -1, lna: Optional[tuple] = None,
                  stats_out: Optional[torch.Tensor] = None, key_ids: Optional[tuple] = None,
                  a_stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused QKV projection + bidirectional attention (qkv_attention.hip):
    ctx [B*S, H*64] = MHA(x @ W^T + b) for S <= 128, head dim 64, with the
    projection weight in ``pack_qkv_heads`` layout.  The [B*S, 3*H*64] QKV
    activation is never materialised.

    Key lengths: ``lens`` (int32 [B], e.g. ``seq_lens``) or ``key_ids=(ids,
    pad_id)`` -- the kernel counts each sequence's non-pad tokens itself
    (right padding, as ``seq_lens``), so no lengths kernel runs.

    ``lna=(colsum, bias_f32, eps)`` (packed order, f32): x holds RAW rows whose
    LayerNorm is folded into ``w_packed`` (``fold_ln_weights`` then packing);
    the kernel computes each row's statistics itself and, with ``stats_out``
    [B*S, 2] f32, stores (sum, sum of squares) for a later ``linear_ln(lnr=...)``.
    ``b_packed`` must then be None.  ``a_stats`` [B*S, P, 2] f32 (P <= 8, row-
    strided view): the producer's per-N-tile partial statistics of x
    (``linear_ln(..., pstats=True)``) -- the kernel sums them instead of
    computing statistics in its main loop."""
    _check(x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and x.dim() == 2 and x.stride(1) == 1,
           "qkv_attention: x must be a 2-D [B*S, K] (row-strided) bf16/f16 view")
    N, K = w_packed.shape
    _check(w_packed.dtype == x.dtype and w_packed.is_contiguous(), "qkv_attention: weight dtype and layout")
    cs = bf = None
    eps = 0.0
    if lna is not None:
        cs, bf, eps = lna
        _check(b_packed is None, "qkv_attention: the folded form takes its bias from lna")
        _check(all(v.dtype == torch.float32 and v.is_contiguous() and v.numel() == N and _aligned(v) for v in (cs, bf)),
               "qkv_attention: lna colsum / bias must be contiguous f32 [H*192]")
        if stats_out is not None:
            _check(stats_out.dtype == torch.float32 and stats_out.is_contiguous() and stats_out.shape == (B * S, 2),
                   "qkv_attention: stats_out must be contiguous f32 [B*S, 2]")
    else:
        _check(b_packed is not None and b_packed.dtype == x.dtype and b_packed.is_contiguous()
               and b_packed.numel() == N and _aligned(b_packed, 8), "qkv_attention: bias dtype / layout")
        _check(stats_out is None, "qkv_attention: stats_out needs lna")
    _check(x.shape == (B * S, K), f"qkv_attention: x must be [B*S, K] = [{B * S}, {K}], got {tuple(x.shape)}")
    _check(N == H * 192, "qkv_attention: packed weight must be [H*3*64, K]")
    _check(qkv_attention_supported(S, H, 64, K), "qkv_attention: S <= 128, head dim 64, K % 8 == 0")
    _check(x.stride(0) % 8 == 0 and _aligned(x) and _aligned(w_packed), "qkv_attention: alignment")
    if lens is not None:
        _check(lens.dtype == torch.int32 and lens.numel() == B and lens.is_cuda, "qkv_attention: lens must be int32 [B]")
    kid, pad = None, 0
    if key_ids is not None:
        kid, pad = key_ids
        _check(lens is None, "qkv_attention: pass lens or key_ids, not both")
        _check(kid.dtype == torch.int32 and kid.is_cuda and kid.is_contiguous() and tuple(kid.shape) == (B, S),
               "qkv_attention: key_ids must be contiguous int32 [B, S] on the GPU")
    if out is None:
        out = torch.empty(B * S, H * 64, device=x.device, dtype=x.dtype)
    _check(out.is_contiguous() and out.shape == (B * S, H * 64) and _aligned(out), "qkv_attention: bad out")
    scale = 1.0 / 8.0 if scale is None else scale
    args = (DTYPE_CODE[x.dtype], x.data_ptr(), x.stride(0), w_packed.data_ptr(), _ptr(b_packed), B, S, H, K,
            _ptr(lens), out.data_ptr(), H * 64, float(scale))
    a_ld = a_parts = 0
    if a_stats is not None:
        _check(lna is not None and stats_out is None, "qkv_attention: a_stats needs lna and no stats_out")
        a_ld, a_parts = _pstats_layout(a_stats, B * S, "qkv_attention a_stats")
        _check(a_parts <= 8, "qkv_attention: at most 8 partials per row")
    extra = (_ptr(cs), _ptr(bf), _ptr(stats_out), float(eps), _ptr(kid), int(pad), _ptr(a_stats), a_ld, a_parts)
    fn = _ops().qkv_attn_fwd
    if cfg < 0:
        key = ("qkv_attn", x.dtype, B, S, H, K, x.stride(0), lna is not None) + (("pstats",) if a_stats is not None else ())
        cfg = _tuned_cfg(key, lambda c: fn(*args, c, _stream(), *extra), range(NUM_QKV_ATTN_CFGS))
    fn(*args, int(cfg), _stream(), *extra)
    return out


def qkv_attention_ref(x, w, b, B, S, H, lens=None, scale=None):
    """Unfused fp32 reference with the UNPACKED [q | k | v] weight; the projection
    is rounded to x's dtype like the two-kernel path."""
    qkv = F.linear(x.float(), w.float(), b.float()).to(x.dtype)
    return attention_ref(qkv, B, S, H, H, w.shape[0] // (3 * H), lens=lens, scale=scale)


def attention_ref(qkv, B, S, H, Hkv, D, lens=None, causal=False, scale=None, q_off=0, k_off=None, v_off=None):
    k_off = H * D if k_off is None else k_off
    v_off = (H + Hkv) * D if v_off is None else v_off
    x = qkv.float()
    q = x[:, q_off:q_off + H * D].reshape(B, S, H, D).transpose(1, 2)
    k = x[:, k_off:k_off + Hkv * D].reshape(B, S, Hkv, D).transpose(1, 2)
    v = x[:, v_off:v_off + Hkv * D].reshape(B, S, Hkv, D).transpose(1, 2)
    if Hkv != H:
        k = k.repeat_interleave(H // Hkv, dim=1)
        v = v.repeat_interleave(H // Hkv, dim=1)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    s = (q @ k.transpose(-1, -2)) * scale
    keys = torch.arange(S, device=qkv.device)
    mask = torch.zeros(B, 1, S, S, dtype=torch.bool, device=qkv.device)
    if lens is not None:
        mask |= (keys[None, None, None, :] >= lens.long()[:, None, None, None])
    if causal:
        mask |= keys[None, None, None, :] > keys[None, None, :, None]
    s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    p = torch.nan_to_num(p, nan=0.0)
    o = (p @ v).transpose(1, 2).reshape(B * S, H * D)
    return o.to(qkv.dtype)


# ---------------------------------------------------------------------------
# Heads / misc
# ---------------------------------------------------------------------------
def softmax_topk(logits: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    _check(logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous(),
           "softmax_topk: logits must be contiguous f32 [B, C]")
    B, C = logits.shape
    _check(C <= 4096 and 1 <= k <= min(16, C), "softmax_topk: C <= 4096 and 1 <= k <= 16")
    probs = torch.empty(B, k, device=logits.device, dtype=torch.float32)
    idx = torch.empty(B, k, device=logits.device, dtype=torch.int32)
    _ops().softmax_topk(logits.data_ptr(), B, C, k, probs.data_ptr(), idx.data_ptr(), _stream())
    return probs, idx


def softmax_topk_packed(logits: torch.Tensor, k: int) -> torch.Tensor:
    """softmax + top-k written as the serving output row [k probs | k class ids
    as f32] ([B, 2k]) by the kernel itself (no cat / cast kernels)."""
    _check(logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous(),
           "softmax_topk: logits must be contiguous f32 [B, C]")
    B, C = logits.shape
    _check(C <= 4096 and 1 <= k <= min(16, C), "softmax_topk: C <= 4096 and 1 <= k <= 16")
    out = torch.empty(B, 2 * k, device=logits.device, dtype=torch.float32)
    _ops().softmax_topk(logits.data_ptr(), B, C, k, out.data_ptr(), 0, _stream())
    return out


def softmax_topk_ref(logits, k):
    p = torch.softmax(logits.float(), dim=-1)
    v, i = torch.topk(p, k, dim=-1)
    return v, i.to(torch.int32)


def rope_tables(max_pos: int, D: int, theta: float = 500000.0, device=None):
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    t = torch.arange(max_pos, dtype=torch.float64)
    f = torch.outer(t, inv)
    return f.cos().float().to(device), f.sin().float().to(device)


def rope_(qkv, cos, sin, B, S, H, Hkv, D, q_off=0, k_off=None, pos_offset=0):
    """In-place rotary embedding of the q and k heads of qkv [B*S, ld]."""
    _check(qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 2 and qkv.stride(1) == 1, "rope: bad qkv")
    _check(cos.dtype == torch.float32 and cos.shape[1] == D // 2 and cos.shape[0] >= S + pos_offset, "rope: bad tables")
    k_off = H * D if k_off is None else k_off
    _ops().rope(qkv.data_ptr(), qkv.stride(0), q_off, k_off, H, Hkv, D, S, cos.data_ptr(), sin.data_ptr(),
                B * S, pos_offset, _stream())
    return qkv


def rope_ref(qkv, cos, sin, B, S, H, Hkv, D, q_off=0, k_off=None, pos_offset=0):
    k_off = H * D if k_off is None else k_off
    x = qkv.float().clone()
    pos = (torch.arange(B * S, device=qkv.device) % S) + pos_offset
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]

    def rot(a):
        a1, a2 = a[..., : D // 2], a[..., D // 2:]
        return torch.cat([a1 * c - a2 * s, a2 * c + a1 * s], dim=-1)

    x[:, q_off:q_off + H * D] = rot(x[:, q_off:q_off + H * D].reshape(-1, H, D)).reshape(-1, H * D)
    x[:, k_off:k_off + Hkv * D] = rot(x[:, k_off:k_off + Hkv * D].reshape(-1, Hkv, D)).reshape(-1, Hkv * D)
    return x.to(qkv.dtype)


def gather_rows(src_ptrs: torch.Tensor, n: int, rows: int, row_bytes: int, dst: torch.Tensor):
    _ops().gather_rows(src_ptrs.data_ptr(), n, rows, row_bytes, dst.data_ptr(), _stream())
