"""LayerNorm / RMSNorm (``norm.hip``)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ._common import DTYPE_CODE, _aligned, _check, _ops, _ptr, _stream


def _norm(x, gamma, beta, eps, residual, residual_out, mode):
    _check(x.is_cuda and x.dtype in (torch.bfloat16, torch.float16), "norm: bad x")
    D = x.shape[-1]
    if x.is_contiguous():
        rows, ldx = x.numel() // D, D
    else:
        # a 2-D row-strided view (e.g. the [CLS] rows): read in place
        _check(x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and _aligned(x, 8)
               and residual is None, "norm: x must be contiguous or a 2-D row-strided view without residual")
        rows, ldx = x.shape[0], x.stride(0)
    _check(D % 4 == 0 and D <= 8192, "norm: D must be a multiple of 4, <= 8192")
    _check(gamma.numel() == D and gamma.dtype == x.dtype, "norm: bad gamma")
    if beta is not None:
        _check(beta.numel() == D and beta.dtype == x.dtype, "norm: bad beta")
    if residual is not None:
        _check(residual.shape == x.shape and residual.is_contiguous() and residual.dtype == x.dtype, "norm: bad residual")
    if residual_out is not None:
        _check(residual_out.shape == x.shape and residual_out.is_contiguous(), "norm: bad residual_out")
    y = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    _ops().norm_fwd(DTYPE_CODE[x.dtype], mode, x.data_ptr(), _ptr(residual), _ptr(residual_out),
                    gamma.data_ptr(), _ptr(beta), y.data_ptr(), rows, D, ldx, float(eps), _stream())
    return y


def layer_norm(x, gamma, beta, eps=1e-12, residual=None, residual_out=None):
    """LayerNorm(x [+ residual]) (optionally also writing x + residual)."""
    return _norm(x, gamma, beta, eps, residual, residual_out, 0)


def rms_norm(x, gamma, eps=1e-5, residual=None, residual_out=None):
    return _norm(x, gamma, None, eps, residual, residual_out, 1)


def layer_norm_ref(x, gamma, beta, eps=1e-12, residual=None):
    xf = x.float() + (residual.float() if residual is not None else 0)
    return F.layer_norm(xf, (x.shape[-1],), gamma.float(), beta.float(), eps).to(x.dtype)


def rms_norm_ref(x, gamma, eps=1e-5, residual=None):
    xf = x.float() + (residual.float() if residual is not None else 0)
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * gamma.float()).to(x.dtype)
