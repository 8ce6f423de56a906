"""Sharp-edge tests of the attention family: ``ops.attention`` (both query-tile
bodies QT = 1 / 2, both 16-bit dtypes, every masking combination, the wrapper's
offset / stride / out / scale arguments), the fused ``ops.qkv_attention`` and
``ops.rope_`` -- each against the plain fp32 reference of the same operation.

Most cases use RAMP inputs (``ramp_qkv``): the scaled score of key j is 8 * j for
every query, so each query row puts >= 1 - e^-8 of its softmax weight on its LAST
visible key and its output is that key's V row.  A kernel that admits one key too
many, or drops the last one, returns a neighbouring (independent random) V row:
an O(1) error on every affected row instead of a shift inside the tolerance.
``test_ramp_inputs_discriminate`` proves that on the CPU (no GPU needed).
"""
import pytest
import torch

ATOL = RTOL = 2e-2           # the suite's attention tolerance (tests/test_ops_gpu.py)
DTYPES = [torch.bfloat16, torch.float16]


def _ops():
    from ray_dynamic_batching_amd import ops

    return ops


def _name(dtype):
    return "bf16" if dtype == torch.bfloat16 else "f16"


def _close(tag, a, b, atol, rtol):
    """tests/test_ops_gpu.py's criterion; prints the observed error first."""
    a, b = a.float(), b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).sum().item()
    print(f"[edges] {tag}: max err {err.max().item():.4g}  max err/tol {(err / tol).max().item():.4g}")
    assert bad == 0, f"{tag}: {bad} / {a.numel()} elements out of tolerance; max err {err.max().item():.4g}"


def _bits(t):
    return t.view(torch.int16)


def ramp_qkv(B, S, H, Hkv, D, dtype, seed):
    """Packed [B*S, (H + 2*Hkv)*D] (q | k | v) on the CPU: q = 64 in elements 0 and 1,
    k of token position j = (16 * (j // 16), j % 16, 0, ...), v random.  q . k = 64 * j,
    so with scale 0.125 the score of key j is 8 * j."""
    assert S <= 512, "16 * (j // 16) must stay exact in bf16"
    x = torch.zeros(B * S, (H + 2 * Hkv) * D, dtype=torch.float32)
    j = torch.arange(B * S) % S
    q = x[:, :H * D].view(B * S, H, D)
    q[:, :, 0] = 64.0
    q[:, :, 1] = 64.0
    k = x[:, H * D:(H + Hkv) * D].view(B * S, Hkv, D)
    k[:, :, 0] = (16 * (j // 16)).float()[:, None]
    k[:, :, 1] = (j % 16).float()[:, None]
    g = torch.Generator().manual_seed(seed)
    x[:, (H + Hkv) * D:] = torch.randn(B * S, Hkv * D, generator=g)
    x = x.to(dtype)
    kk = x[:, H * D:(H + Hkv) * D].float().view(B * S, Hkv, D)
    assert torch.equal(kk[:, :, 0] + kk[:, :, 1], j.float()[:, None].expand(B * S, Hkv)), "ramp not exact"
    return x


# name -> (B, S, H, Hkv, D, causal, lens)
_EDGE_LENS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 199, 200]
ATTN_CASES = {
    "lens_edges_d64": (12, 200, 2, 2, 64, False, _EDGE_LENS),
    "lens_edges_d128": (12, 200, 4, 1, 128, False, _EDGE_LENS),     # KB = 64: 63/64/65, 127/128/129 are block edges
    "causal_d128": (2, 200, 4, 1, 128, True, None),
    "causal_gqa_d64": (2, 200, 4, 2, 64, True, None),
    "causal_s1": (1, 1, 1, 1, 64, True, None),
    "causal_s17": (1, 17, 2, 2, 64, True, None),
    "causal_lens": (4, 200, 4, 2, 128, True, [200, 1, 64, 130]),
}
# name -> (B, S, lens): H = 2, head dim 64 (the fused kernel's)
FUSED_CASES = {
    "s128": (5, 128, [128, 1, 127, 64, 65]),     # cfg 4 pairs sequences of different lengths; odd B
    "s100": (3, 100, [100, 17, 99]),
    "s37": (2, 37, [37, 16]),
}
SELF_CHECK_CASES = dict(ATTN_CASES)
SELF_CHECK_CASES.update({f"fused_{n}": (B, S, 2, 2, 64, False, lens) for n, (B, S, lens) in FUSED_CASES.items()})
SELF_CHECK_CASES.update({
    "wide_d64": (3, 300, 4, 2, 64, False, [300, 129, 257]),
    "long_causal_d128": (2, 512, 2, 1, 128, True, None),
})


def _scale(D):
    return 0.125 if D == 128 else None      # 0.125 is the default at D = 64


# ---------------------------------------------------------------------------
# B. CPU self-check: the ramp inputs make every mask error visible on every row
# ---------------------------------------------------------------------------
def _visible(B, S, lens, causal, dlen=0, dcausal=0):
    """[B, S(query), S(key)] bool: key visible.  dlen shifts every length (clamped to
    [1, S]), dcausal the causal bound (key > q + dcausal is masked)."""
    keys = torch.arange(S)
    vis = torch.ones(B, S, S, dtype=torch.bool)
    if lens is not None:
        ln = torch.tensor(lens, dtype=torch.long)
        if dlen:
            ln = (ln + dlen).clamp(1, S)
        vis &= keys[None, None, :] < ln[:, None, None]
    if causal:
        vis &= ~(keys[None, None, :] > keys[None, :, None] + dcausal)
    return vis


def _masked_ref(qkv, B, S, H, Hkv, D, vis, scale):
    """ops.attention_ref with an explicit visibility mask."""
    x = qkv.float()
    q = x[:, :H * D].reshape(B, S, H, D).transpose(1, 2)
    k = x[:, H * D:(H + Hkv) * D].reshape(B, S, Hkv, D).transpose(1, 2)
    v = x[:, (H + Hkv) * D:].reshape(B, S, Hkv, D).transpose(1, 2)
    if Hkv != H:
        k = k.repeat_interleave(H // Hkv, dim=1)
        v = v.repeat_interleave(H // Hkv, dim=1)
    s = (q @ k.transpose(-1, -2)) * (D ** -0.5 if scale is None else scale)
    s = s.masked_fill(~vis[:, None], float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
    return (p @ v).transpose(1, 2).reshape(B * S, H * D).to(qkv.dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", list(SELF_CHECK_CASES))
def test_ramp_inputs_discriminate(case, dtype):
    """No GPU.  On the ramp inputs the fp32 reference is finite, and a reference
    with every length off by one (either way) or the causal bound off by one (either
    way) fails the suite's tolerance on EVERY query row whose visible keys it
    changes, and on no other row."""
    ops = _ops()
    B, S, H, Hkv, D, causal, lens = SELF_CHECK_CASES[case]
    x = ramp_qkv(B, S, H, Hkv, D, dtype, seed=1)
    lens_t = None if lens is None else torch.tensor(lens, dtype=torch.int32)
    ref = ops.attention_ref(x, B, S, H, Hkv, D, lens=lens_t, causal=causal, scale=_scale(D))
    assert torch.isfinite(ref.float()).all()
    vis = _visible(B, S, lens, causal)
    assert torch.equal(_masked_ref(x, B, S, H, Hkv, D, vis, _scale(D)), ref)
    # the last visible key carries the row: its V row is the output
    last = vis.long().cumsum(-1).argmax(-1)                                   # [B, S]
    v = x[:, (H + Hkv) * D:].float().view(B, S, Hkv, D)
    want = torch.stack([v[b, last[b]] for b in range(B)]).repeat_interleave(H // Hkv, dim=2).reshape(B * S, H * D)
    assert ((ref.float() - want).abs() <= ATOL + RTOL * want.abs()).all()

    mutants = []
    if lens is not None:
        mutants += [("lens+1", dict(dlen=1)), ("lens-1", dict(dlen=-1))]
    if causal:
        mutants += [("key>q+1", dict(dcausal=1)), ("key>q-1", dict(dcausal=-1))]
    touched = 0
    for name, kw in mutants:
        vis_m = _visible(B, S, lens, causal, **kw)
        mut = _masked_ref(x, B, S, H, Hkv, D, vis_m, _scale(D))
        affected = (vis_m != vis).any(-1).reshape(B * S)
        err = (mut.float() - ref.float()).abs()
        flagged = (err > ATOL + RTOL * ref.float().abs()).any(-1)
        assert flagged[affected].all(), f"{name}: {int((~flagged[affected]).sum())} affected rows pass the tolerance"
        assert not flagged[~affected].any(), f"{name}: unaffected rows flagged"
        touched += int(affected.sum())
    assert touched > 0, "no mutant changes anything at this shape"


# ---------------------------------------------------------------------------
# C. ops.attention on ramp inputs, both QT bodies, both dtypes
# ---------------------------------------------------------------------------
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    """The shared inputs / references live for this module only."""
    yield
    _cache.clear()


def _cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def _ramp_case(case, dtype):
    """(qkv, lens, fp32 reference) on the GPU, built once per (case, dtype)."""
    def build():
        ops = _ops()
        B, S, H, Hkv, D, causal, lens = ATTN_CASES[case]
        x = ramp_qkv(B, S, H, Hkv, D, dtype, seed=2).cuda()
        lens_t = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
        ref = ops.attention_ref(x, B, S, H, Hkv, D, lens=lens_t, causal=causal, scale=_scale(D))
        return x, lens_t, ref

    return _cached(("ramp", case, dtype), build)


@pytest.mark.gpu
@pytest.mark.parametrize("QT", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", list(ATTN_CASES))
def test_attention_ramp(case, dtype, QT, monkeypatch):
    """Length edges at key-tile / key-block boundaries, causal (D = 64 and 128, GQA,
    S = 1, S = 17, a partial second query block at QT = 2), causal + lens."""
    ops = _ops()
    monkeypatch.setenv("RDB_ATTN_QT", str(QT))
    B, S, H, Hkv, D, causal, _ = ATTN_CASES[case]
    x, lens, ref = _ramp_case(case, dtype)
    y = ops.attention(x, B, S, H, Hkv, D, lens=lens, causal=causal, scale=_scale(D))
    _close(f"C attention_ramp {case} {_name(dtype)} QT{QT}", y, ref, ATOL, RTOL)


@pytest.mark.gpu
@pytest.mark.parametrize("QT", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("B,S,H,Hkv,D,causal,lens", [
    (4, 200, 2, 2, 64, False, [200, 0, 65, 1]),
    (3, 130, 4, 2, 128, True, [0, 130, 64]),
])
def test_attention_zero_length(B, S, H, Hkv, D, causal, lens, dtype, QT, monkeypatch):
    """A sequence of length 0 has no visible key: its rows are exactly zero (what
    attention_ref gives through nan_to_num); its neighbours are untouched by it."""
    ops = _ops()
    monkeypatch.setenv("RDB_ATTN_QT", str(QT))
    x = ramp_qkv(B, S, H, Hkv, D, dtype, seed=3).cuda()
    lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
    y = torch.full((B * S, H * D), 7.0, device="cuda", dtype=dtype)
    ops.attention(x, B, S, H, Hkv, D, lens=lens_t, causal=causal, scale=_scale(D), out=y)
    ref = ops.attention_ref(x, B, S, H, Hkv, D, lens=lens_t, causal=causal, scale=_scale(D))
    b0 = lens.index(0)
    assert torch.equal(ref[b0 * S:(b0 + 1) * S], torch.zeros(S, H * D, device="cuda", dtype=dtype))
    assert torch.equal(y[b0 * S:(b0 + 1) * S], torch.zeros(S, H * D, device="cuda", dtype=dtype))
    _close(f"C attention_zero_length D{D} {_name(dtype)} QT{QT}", y, ref, ATOL, RTOL)


# ---------------------------------------------------------------------------
# D. natural dispatch to QT = 2 (no override)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,S,H,Hkv,D,dtype,causal", [
    (22, 197, 12, 12, 64, torch.float16, False),        # ViT-B/16 at batch 22: <f16, 64, 2>
    (16, 130, 32, 8, 128, torch.bfloat16, True),        # Llama-like prefill: <bf16, 128, 2>, GQA
], ids=["vit", "llama"])
def test_attention_natural_qt2(B, S, H, Hkv, D, dtype, causal, monkeypatch):
    ops = _ops()
    monkeypatch.delenv("RDB_ATTN_QT", raising=False)
    assert -(-S // 128) * H * B >= 512, "this shape would dispatch to QT = 1"
    tag = f"D natural_qt2 S{S} D{D} {_name(dtype)}"
    torch.manual_seed(21)
    x = torch.randn(B * S, (H + 2 * Hkv) * D, device="cuda", dtype=dtype)
    _close(tag + " random", ops.attention(x, B, S, H, Hkv, D, causal=causal),
           ops.attention_ref(x, B, S, H, Hkv, D, causal=causal), ATOL, RTOL)
    x = ramp_qkv(B, S, H, Hkv, D, dtype, seed=4).cuda()
    _close(tag + " ramp", ops.attention(x, B, S, H, Hkv, D, causal=causal, scale=_scale(D)),
           ops.attention_ref(x, B, S, H, Hkv, D, causal=causal, scale=_scale(D)), ATOL, RTOL)
    # the same launch with a length per sequence, cycling through the tile / block edges
    edges = [S, 1, 63, 64, 65, 127, 128, 129, S - 1, 16, 17]
    lens = torch.tensor([edges[i % len(edges)] for i in range(B)], dtype=torch.int32, device="cuda")
    _close(tag + " ramp+lens", ops.attention(x, B, S, H, Hkv, D, lens=lens, causal=causal, scale=_scale(D)),
           ops.attention_ref(x, B, S, H, Hkv, D, lens=lens, causal=causal, scale=_scale(D)), ATOL, RTOL)


# ---------------------------------------------------------------------------
# E. wrapper arguments: offsets, row stride, scale, out
# ---------------------------------------------------------------------------
_WRAP_CASES = {
    "causal_gqa": (2, 200, 4, 2, 128, True, None),
    "noncausal": (3, 150, 2, 2, 64, False, [150, 77, 1]),
}


def _wrap_case(case, dtype):
    def build():
        ops = _ops()
        B, S, H, Hkv, D, causal, lens = _WRAP_CASES[case]
        # columns [8 pad | v | q | 8 pad | k] in a buffer 72 columns wider than the row
        v_off = 8
        q_off = v_off + Hkv * D
        k_off = q_off + H * D + 8
        W = k_off + Hkv * D
        g = torch.Generator().manual_seed(31)
        buf = torch.randn(B * S, W + 72, generator=g).to(dtype).cuda()
        lens_t = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
        ref = ops.attention_ref(buf[:, :W], B, S, H, Hkv, D, lens=lens_t, causal=causal, scale=0.2,
                                q_off=q_off, k_off=k_off, v_off=v_off)
        return buf, W, (q_off, k_off, v_off), lens_t, ref

    return _cached(("wrap", case, dtype), build)


@pytest.mark.gpu
@pytest.mark.parametrize("QT", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", list(_WRAP_CASES))
def test_attention_wrapper_arguments(case, dtype, QT, monkeypatch):
    """q_off / k_off / v_off in a non-default column order, a row stride above the
    row, a non-default scale and a preallocated out=."""
    ops = _ops()
    monkeypatch.setenv("RDB_ATTN_QT", str(QT))
    B, S, H, Hkv, D, causal, _ = _WRAP_CASES[case]
    buf, W, (q_off, k_off, v_off), lens, ref = _wrap_case(case, dtype)
    view = buf[:, :W]
    assert view.stride(0) == W + 72
    before = buf.clone()
    out = torch.full((B * S, H * D), 30000.0, device="cuda", dtype=dtype)
    sentinel = out[0, 0].clone()
    y = ops.attention(view, B, S, H, Hkv, D, lens=lens, causal=causal, scale=0.2, out=out,
                      q_off=q_off, k_off=k_off, v_off=v_off)
    assert y is out
    assert not (out == sentinel).any(), "out= was not fully written"
    assert torch.equal(_bits(buf), _bits(before)), "attention wrote to its input"
    _close(f"E wrapper_arguments {case} {_name(dtype)} QT{QT}", y, ref, ATOL, RTOL)


# ---------------------------------------------------------------------------
# F. fused projection + attention, driven by identity weights
# ---------------------------------------------------------------------------
def _fused_case(case, dtype):
    def build():
        ops = _ops()
        B, S, lens = FUSED_CASES[case]
        H = 2
        x = ramp_qkv(B, S, H, H, 64, dtype, seed=5).cuda()           # [B*S, 384]: K = 3 * H * 64
        w = torch.eye(3 * H * 64, device="cuda", dtype=dtype)
        wp, bp = ops.pack_qkv_heads(w, torch.zeros(3 * H * 64, device="cuda", dtype=dtype), H)
        lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
        ref_lens = ops.attention_ref(x, B, S, H, H, 64, lens=lens_t)
        ref_full = ops.attention_ref(x, B, S, H, H, 64)
        return x, wp, bp, lens_t, ref_lens, ref_full

    return _cached(("fused", case, dtype), build)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", list(FUSED_CASES))
def test_qkv_attention_identity_ramp(case, dtype, cfg):
    """W = I, b = 0: products with 1 and 0 accumulate exactly, so the kernel's
    internal q | k | v IS x, and x can be a ramp tensor: every query row probes the
    fused kernel's length mask (and, for S < 128, the mask of keys >= S, which
    belong to the next sequence or lie past the last row)."""
    ops = _ops()
    B, S, lens = FUSED_CASES[case]
    H = 2
    x, wp, bp, lens_t, ref_lens, ref_full = _fused_case(case, dtype)
    tag = f"F qkv_attention_identity {case} {_name(dtype)} cfg{cfg}"
    y = ops.qkv_attention(x, wp, bp, B, S, H, lens=lens_t, cfg=cfg)
    _close(tag + " lens", y, ref_lens, ATOL, RTOL)
    _close(tag + " nolens", ops.qkv_attention(x, wp, bp, B, S, H, cfg=cfg), ref_full, ATOL, RTOL)
    # lengths counted in-kernel from right-padded ids: bit-identical
    ids = torch.full((B, S), 9, device="cuda", dtype=torch.int32)
    for i, n in enumerate(lens):
        ids[i, n:] = 7
    assert torch.equal(_bits(ops.qkv_attention(x, wp, bp, B, S, H, cfg=cfg, key_ids=(ids, 7))), _bits(y))
    # a length of 0 behaves as 1 (the kernel's clamp, the seq_lens contract)
    l0, l1 = lens_t.clone(), lens_t.clone()
    l0[1], l1[1] = 0, 1
    y1 = ops.qkv_attention(x, wp, bp, B, S, H, lens=l1, cfg=cfg)
    assert torch.equal(_bits(ops.qkv_attention(x, wp, bp, B, S, H, lens=l0, cfg=cfg)), _bits(y1))
    ids[1, :] = 7
    assert torch.equal(_bits(ops.qkv_attention(x, wp, bp, B, S, H, cfg=cfg, key_ids=(ids, 7))), _bits(y1))
    _close(tag + " len0as1", y1, ops.attention_ref(x, B, S, H, H, 64, lens=l1), ATOL, RTOL)


# ---------------------------------------------------------------------------
# G. RoPE
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,S,H,Hkv,D,pos_offset,layout", [
    (4, 128, 32, 8, 128, 0, "packed"),          # 1.31 M pairs: the grid-stride loop runs
    (3, 37, 4, 2, 64, 5, "packed"),
    (2, 64, 8, 2, 128, 100, "strided"),
])
def test_rope_edges(B, S, H, Hkv, D, pos_offset, layout):
    """Rotated q / k columns within one bf16 ulp of the fp32 reference (both sides
    compute in fp32 and round once; an FMA contraction moves the fp32 value by
    ~1e-7, which can flip the rounding but no more); V, pad columns and the
    buffer beyond the row are bit-identical to their values before the call."""
    ops = _ops()
    torch.manual_seed(41)
    T = B * S
    if layout == "packed":
        q_off, k_off, W, ld = 0, H * D, (H + 2 * Hkv) * D, (H + 2 * Hkv) * D
        assert (B, S) != (4, 128) or T * (H + Hkv) * D // 2 > 4096 * 256
    else:       # [8 pad | q | 24 pad | k | 8 pad | v] in a buffer 40 columns wider than the row
        q_off = 8
        k_off = q_off + H * D + 24
        W = k_off + Hkv * D + 8 + Hkv * D
        ld = W + 40
    buf = torch.randn(T, ld, device="cuda", dtype=torch.bfloat16)
    qkv = buf[:, :W]
    before = buf.clone()
    cos, sin = ops.rope_tables(256, D, device="cuda")
    if layout == "packed":
        ref = ops.rope_ref(qkv, cos, sin, B, S, H, Hkv, D, pos_offset=pos_offset)
        ops.rope_(qkv, cos, sin, B, S, H, Hkv, D, pos_offset=pos_offset)
    else:
        ref = ops.rope_ref(qkv, cos, sin, B, S, H, Hkv, D, q_off=q_off, k_off=k_off, pos_offset=pos_offset)
        ops.rope_(qkv, cos, sin, B, S, H, Hkv, D, q_off=q_off, k_off=k_off, pos_offset=pos_offset)
    rot = torch.zeros(ld, dtype=torch.bool, device="cuda")
    rot[q_off:q_off + H * D] = True
    rot[k_off:k_off + Hkv * D] = True
    y, r = buf[:, rot].float(), ref[:, rot[:W]].float()
    err = (y - r).abs()
    tol = 1e-6 + 2.0 ** -7 * r.abs()
    print(f"[edges] G rope {layout} S{S} D{D} pos{pos_offset} bf16: max err {err.max().item():.4g}  "
          f"max err/tol {(err / tol).max().item():.4g}  elements differing {int((err > 0).sum())} / {err.numel()}")
    assert (err <= tol).all(), f"{int((err > tol).sum())} rotated elements beyond one bf16 ulp"
    assert not torch.equal(_bits(buf[:, rot]), _bits(before[:, rot])), "nothing was rotated"
    assert torch.equal(_bits(buf[:, ~rot]), _bits(before[:, ~rot])), "rope_ wrote outside the q / k heads"
    assert torch.equal(_bits(ref[:, ~rot[:W]]), _bits(before[:, :W][:, ~rot[:W]]))
