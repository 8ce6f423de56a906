"""Convolution family (NHWC f16): the image / stem transforms that feed it,
conv2d, depthwise conv, pools, ShuffleNet remap, squeeze-excitation scaling."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from ._common import ACT_CODE, DTYPE_CODE, _act_ref, _aligned, _check, _ops, _ptr, _stream
from .splitk import _private_splitk_ws, _tune_launcher
from .tiles import CONV_HALO, CONV_LINEAR, SPLITK_HEADER, _conv_candidates, conv_halo_candidates, splits_of
from .tuning import _tuned_cfg


def image_to_nhwc(img_u8: torch.Tensor, Cp: int = 8) -> torch.Tensor:
    """uint8 [N, H, W, 3] -> normalised f16 [N, H, W, Cp] (ImageNet mean/std)."""
    _check(img_u8.is_cuda and img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.shape[-1] == 3, "image_to_nhwc: bad input")
    N, H, W, _ = img_u8.shape
    out = torch.empty(N, H, W, Cp, device=img_u8.device, dtype=torch.float16)
    _ops().image_to_nhwc(img_u8.data_ptr(), N, H * W, Cp, out.data_ptr(), _stream())
    return out


def image_to_s2d(img_u8: torch.Tensor, zero: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [N, H, W, 3] -> normalised f16 space-to-depth [N, H/2, W/2, 16]
    (channel (dy*2+dx)*3 + c = pixel (2i+dy, 2j+dx) channel c; 12..15 zero).
    ``zero``: a split-K workspace (``splitk_workspace(..., zeroed=False)``) whose
    counter header the same kernel zeroes -- no separate memset per forward."""
    _check(img_u8.is_cuda and img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.shape[-1] == 3,
           "image_to_s2d: bad input")
    N, H, W, _ = img_u8.shape
    _check(H % 2 == 0 and W % 4 == 0, "image_to_s2d: H must be even and W a multiple of 4")
    out = torch.empty(N, H // 2, W // 2, 16, device=img_u8.device, dtype=torch.float16)
    zb = 0
    if zero is not None:
        _check(zero.is_cuda and zero.dtype == torch.uint8 and zero.numel() >= SPLITK_HEADER and _aligned(zero),
               "image_to_s2d: zero must be a split-K workspace")
        zb = SPLITK_HEADER
    _ops().image_to_s2d(img_u8.data_ptr(), N, H, W, out.data_ptr(), _ptr(zero), zb, _stream())
    return out


def stem_s2d_pool(img_u8: torch.Tensor, w_s2d: torch.Tensor, bias: torch.Tensor,
                  zero: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The ResNet stem in one kernel (ops/csrc/cnn_stem.hip): uint8 [N, H, W, 3]
    -> normalise -> space-to-depth -> 4x4 conv with ``w_s2d`` [64, 4, 4, 16]
    (``stem_weight_s2d``) + bias + ReLU -> 3x3 / stride-2 max-pool (pad 1) ->
    f16 [N, H/4, W/4, 64].  H, W multiples of 32.  ``zero``: a split-K workspace
    whose counter header the kernel zeroes on the side."""
    _check(img_u8.is_cuda and img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.shape[-1] == 3,
           "stem_s2d_pool: bad image")
    N, H, W, _ = img_u8.shape
    _check(H % 32 == 0 and W % 32 == 0, "stem_s2d_pool: H and W must be multiples of 32")
    _check(w_s2d.shape == (64, 4, 4, 16) and w_s2d.dtype == torch.float16 and w_s2d.is_contiguous()
           and bias.numel() == 64 and bias.dtype == torch.float16 and _aligned(w_s2d), "stem_s2d_pool: bad weights")
    out = torch.empty(N, H // 4, W // 4, 64, device=img_u8.device, dtype=torch.float16)
    zb = 0
    if zero is not None:
        _check(zero.is_cuda and zero.dtype == torch.uint8 and zero.numel() >= SPLITK_HEADER and _aligned(zero),
               "stem_s2d_pool: zero must be a split-K workspace")
        zb = SPLITK_HEADER
    _ops().stem_s2d_pool(img_u8.data_ptr(), N, H, W, w_s2d.data_ptr(), bias.data_ptr(), out.data_ptr(), _ptr(zero),
                         zb, _stream())
    return out


def image_to_s2d_ref(img_u8):
    x = image_to_nhwc_ref(img_u8, 3).float()                       # [N, H, W, 3]
    N, H, W, _ = x.shape
    x = x.view(N, H // 2, 2, W // 2, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 12)
    return torch.cat([x, torch.zeros(N, H // 2, W // 2, 4, device=x.device)], -1).half()


def stem_weight_s2d(w: torch.Tensor) -> torch.Tensor:
    """7x7 stride-2 pad-3 conv weights [K, 7, 7, 3] -> the equivalent 4x4 stride-1
    pad-2 conv on the space-to-depth input, [K, 4, 4, 16]: input row 2(p-2+bi)+dy
    is tap r = 2*bi + dy - 1 of output row p (taps outside 0..6 are zero)."""
    K = w.shape[0]
    out = torch.zeros(K, 4, 4, 16, dtype=w.dtype, device=w.device)
    for bi in range(4):
        for bj in range(4):
            for dy in range(2):
                for dx in range(2):
                    r, c = 2 * bi + dy - 1, 2 * bj + dx - 1
                    if 0 <= r < 7 and 0 <= c < 7:
                        ch = (dy * 2 + dx) * 3
                        out[:, bi, bj, ch:ch + 3] = w[:, r, c, :3]
    return out.contiguous()


def image_to_nhwc_ref(img_u8, Cp=8):
    mean = torch.tensor([0.485, 0.456, 0.406], device=img_u8.device)
    std = torch.tensor([0.229, 0.224, 0.225], device=img_u8.device)
    x = (img_u8.float() / 255.0 - mean) / std
    pad = torch.zeros(*x.shape[:-1], Cp - 3, device=x.device)
    return torch.cat([x, pad], -1).half()


def conv2d_nhwc(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, stride: int = 1,
                pad: int = 0, act: str = "none", residual: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, tile_cfg: int = -1, out_hw: Optional[tuple] = None,
                workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [N, H, W, C] f16, w [K, R, S, C] f16 (BN folded), bias [K]; fused residual + act.
    ``out_hw`` = (P, Q) computes only the first P x Q outputs (an asymmetric pad:
    the space-to-depth stem pads 2 on top / left and 1 on the bottom / right).
    ``workspace`` (``splitk_workspace``): used when the chosen tile is split-K;
    without one a split-K choice allocates its own (one extra memset)."""
    _check(x.is_cuda and x.dtype == torch.float16 and x.is_contiguous() and x.dim() == 4, "conv2d: bad x")
    _check(w.dtype == torch.float16 and w.is_contiguous() and w.dim() == 4, "conv2d: bad w")
    N, H, W, C = x.shape
    K, R, S, C2 = w.shape
    _check(C == C2 and C % 8 == 0, f"conv2d: channel mismatch/alignment {C} vs {C2}")
    P = (H + 2 * pad - R) // stride + 1
    Q = (W + 2 * pad - S) // stride + 1
    if out_hw is not None:
        _check(0 < out_hw[0] <= P and 0 < out_hw[1] <= Q, "conv2d: out_hw larger than the padded output")
        P, Q = int(out_hw[0]), int(out_hw[1])
    if out is None:
        out = torch.empty(N, P, Q, K, device=x.device, dtype=torch.float16)
    _check(out.shape == (N, P, Q, K) and out.is_contiguous(), "conv2d: bad out")
    if bias is not None:
        _check(bias.numel() == K and bias.dtype == torch.float16, "conv2d: bad bias")
    if residual is not None:
        _check(residual.shape == (N, P, Q, K) and residual.is_contiguous() and residual.dtype == torch.float16, "conv2d: bad residual")
    _check(_aligned(x) and _aligned(w), "conv2d: alignment")
    M, Kg = N * P * Q, R * S * C
    one_by_one = R == 1 and S == 1 and stride == 1 and pad == 0
    fn = _ops().conv2d_nhwc
    args = (x.data_ptr(), w.data_ptr(), _ptr(bias), _ptr(residual), out.data_ptr(), N, H, W, C, K, R, S,
            stride, pad, P, Q, ACT_CODE[act])

    def launch(c: int, ws: Optional[torch.Tensor]) -> None:
        if c >= 0 and c & CONV_LINEAR:
            _ops().gemm_tn(DTYPE_CODE[torch.float16], DTYPE_CODE[torch.float16], x.data_ptr(), C, w.data_ptr(), C,
                           out.data_ptr(), K, _ptr(bias), _ptr(residual), K if residual is not None else 0, M, K, C,
                           1.0, ACT_CODE[act], _stream(), c & ~CONV_LINEAR)
            return
        sp = splits_of(c)
        if sp > 1 and ws is None:
            need = _ops().conv_halo_ws_bytes(c & 255, N, H, W, C, K, sp, stride) if c & CONV_HALO else \
                _ops().conv_splitk_bytes(M, K, c & ~0xF00, sp)
            ws = _private_splitk_ws(x.device, int(need))
        fn(*args, _stream(), int(c), _ptr(ws), 0 if ws is None else ws.numel())

    if tile_cfg < 0:
        key = ("conv", N, H, W, C, K, R, S, stride, pad, act, bias is not None, residual is not None) + \
            ((P, Q) if out_hw is not None else ())
        tile_cfg = _tuned_cfg(key, _tune_launcher(launch, x.device),
                              _conv_candidates(M, K, Kg, one_by_one, C, bias is not None) +
                              conv_halo_candidates(N, H, W, C, K, R, S, stride, pad, P, Q, bias is not None,
                                                   residual is not None, act))
    launch(int(tile_cfg), workspace)
    return out


def conv2d_nhwc_ref(x, w, bias=None, stride=1, pad=0, act="none", residual=None):
    y = F.conv2d(x.permute(0, 3, 1, 2).float(), w.permute(0, 3, 1, 2).float(),
                 bias.float() if bias is not None else None, stride=stride, padding=pad)
    y = y.permute(0, 2, 3, 1)
    if residual is not None:
        y = y + residual.float()
    return _act_ref(y, act).to(torch.float16)


def dwconv_nhwc(x, w, bias, stride=1, pad=1, act="none"):
    """Depthwise conv: x [N, H, W, C], w [R, R, C], bias [C]."""
    _check(x.is_cuda and x.dtype == torch.float16 and x.is_contiguous(), "dwconv: bad x")
    N, H, W, C = x.shape
    R = w.shape[0]
    _check(w.shape == (R, R, C) and w.is_contiguous() and bias.numel() == C and C % 8 == 0, "dwconv: bad w/bias")
    P = (H + 2 * pad - R) // stride + 1
    Q = (W + 2 * pad - R) // stride + 1
    out = torch.empty(N, P, Q, C, device=x.device, dtype=torch.float16)
    _ops().dwconv_nhwc(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), N, H, W, C, R, stride, pad, P, Q,
                       ACT_CODE[act], _stream())
    return out


def dwconv_nhwc_ref(x, w, bias, stride=1, pad=1, act="none"):
    C = x.shape[-1]
    y = F.conv2d(x.permute(0, 3, 1, 2).float(), w.permute(2, 0, 1).unsqueeze(1).float(), bias.float(),
                 stride=stride, padding=pad, groups=C)
    return _act_ref(y.permute(0, 2, 3, 1), act).to(torch.float16)


def maxpool_nhwc(x, k=3, stride=2, pad=1):
    _check(x.is_cuda and x.dtype == torch.float16 and x.is_contiguous() and x.shape[-1] % 8 == 0, "maxpool: bad x")
    N, H, W, C = x.shape
    P = (H + 2 * pad - k) // stride + 1
    Q = (W + 2 * pad - k) // stride + 1
    out = torch.empty(N, P, Q, C, device=x.device, dtype=torch.float16)
    _ops().maxpool_nhwc(x.data_ptr(), out.data_ptr(), N, H, W, C, k, stride, pad, P, Q, _stream())
    return out


def maxpool_nhwc_ref(x, k=3, stride=2, pad=1):
    return F.max_pool2d(x.permute(0, 3, 1, 2).float(), k, stride, pad).permute(0, 2, 3, 1).half()


def avgpool_nhwc(x):
    _check(x.is_cuda and x.dtype == torch.float16 and x.is_contiguous() and x.shape[-1] % 8 == 0, "avgpool: bad x")
    N, H, W, C = x.shape
    out = torch.empty(N, C, device=x.device, dtype=torch.float16)
    _ops().avgpool_nhwc(x.data_ptr(), out.data_ptr(), N, H * W, C, _stream())
    return out


def avgpool_nhwc_ref(x):
    return x.float().mean(dim=(1, 2)).half()


def shuffle_remap(a: torch.Tensor, b: torch.Tensor, ch: int, split: bool, ld1: int, ld2: int = 0):
    """ShuffleNetV2 concat(a, b) + channel_shuffle(groups=2) [+ split] in one pass.

    a, b: [..., >=ch] f16 (x1 / branch output, possibly channel-padded views with
    unit stride in the last dim).  Returns one tensor [..., ld1] (``split=False``,
    2*ch real channels) or two tensors [..., ld1], [..., ld2] (the next unit's
    halves, ch real channels each); padded channels are zero."""
    _check(a.is_cuda and a.dtype == torch.float16 and b.dtype == torch.float16, "shuffle_remap: f16 cuda tensors")
    _check(a.stride(-1) == 1 and b.stride(-1) == 1 and a.shape[:-1] == b.shape[:-1], "shuffle_remap: bad views")
    lead = a.shape[:-1]
    pixels = 1
    for d in lead:
        pixels *= d
    lda = a.stride(-2) if a.dim() > 1 else a.shape[-1]
    ldb = b.stride(-2) if b.dim() > 1 else b.shape[-1]
    _check(a.dim() < 2 or all(a.stride(i) == a.stride(i + 1) * a.shape[i + 1] for i in range(a.dim() - 2)),
           "shuffle_remap: a must be a channel slice of a contiguous tensor")
    _check(b.dim() < 2 or all(b.stride(i) == b.stride(i + 1) * b.shape[i + 1] for i in range(b.dim() - 2)),
           "shuffle_remap: b must be a channel slice of a contiguous tensor")
    o1 = torch.empty(*lead, ld1, device=a.device, dtype=torch.float16)
    o2 = torch.empty(*lead, ld2, device=a.device, dtype=torch.float16) if split else None
    _ops().shuffle_remap(a.data_ptr(), lda, b.data_ptr(), ldb, ch, pixels, o1.data_ptr(), ld1, _ptr(o2), ld2,
                         int(split), _stream())
    return (o1, o2) if split else o1


def shuffle_remap_ref(a, b, ch, split, ld1, ld2=0):
    cat = torch.cat([a[..., :ch], b[..., :ch]], dim=-1)
    lead = cat.shape[:-1]
    sh = cat.reshape(*lead, 2, ch).transpose(-1, -2).reshape(*lead, 2 * ch)

    def pad(t, ld):
        out = torch.zeros(*lead, ld, device=t.device, dtype=t.dtype)
        out[..., :t.shape[-1]] = t
        return out
    if split:
        return pad(sh[..., :ch], ld1), pad(sh[..., ch:], ld2)
    return pad(sh, ld1)


def se_scale(x: torch.Tensor, s: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Squeeze-excitation scaling: x [N, H, W, C] * s [N, C] (f16)."""
    _check(x.is_cuda and x.dtype == torch.float16 and x.is_contiguous() and x.dim() == 4, "se_scale: bad x")
    N, H, W, C = x.shape
    _check(s.shape == (N, C) and s.is_contiguous() and s.dtype == torch.float16, "se_scale: bad s")
    out = torch.empty_like(x) if out is None else out
    _ops().se_scale(x.data_ptr(), s.data_ptr(), out.data_ptr(), N, H * W, C, _stream())
    return out


def se_scale_ref(x, s):
    return (x.float() * s.float()[:, None, None, :]).to(torch.float16)
