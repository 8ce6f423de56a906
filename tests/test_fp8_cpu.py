"""FP8 (e4m3fn) W8A8 on the CPU: the host-side weight quantiser, the fp32
references of the FP8 ops, and the fake-quantised Llama path (backend="torch")."""
import pytest
import torch

FP8 = torch.float8_e4m3fn


def _ops():
    from ray_dynamic_batching_amd import ops

    return ops


def check_fp8_rows(x32, q, scale):
    """The properties every row quantiser here must have, against the f32 values
    ``x32`` [rows, K] it quantised: the amax element of a non-zero row decodes to
    exactly +-448, a zero row gives scale 1 and zero bytes, |deq - x| is at most
    half an e4m3 step (2^-4 relative for normals, scale * 2^-10 for subnormals),
    and no byte is a NaN encoding."""
    assert q.dtype == FP8 and scale.dtype == torch.float32
    rows, K = x32.shape
    q, scale = q.reshape(rows, K).cpu(), scale.reshape(rows).cpu()
    x32 = x32.cpu()
    raw = q.view(torch.uint8)
    assert int(((raw & 0x7F) == 0x7F).sum()) == 0, "NaN encodings"
    qf = q.float()
    amax = x32.abs().amax(1)
    zero = amax == 0
    assert torch.equal(scale[zero], torch.ones(int(zero.sum())))
    assert int(raw[zero].count_nonzero()) == 0
    idx = x32.abs().argmax(1)
    top = qf[torch.arange(rows), idx]
    assert torch.equal(top[~zero].abs(), torch.full((int((~zero).sum()),), 448.0))
    assert torch.equal(torch.sign(top[~zero]), torch.sign(x32[torch.arange(rows), idx][~zero]))
    deq = qf * scale[:, None]
    bound = torch.maximum(x32.abs() * 2.0 ** -4, scale[:, None] * 2.0 ** -10)
    ratio = ((deq - x32).abs() / bound.clamp_min(1e-30)).max().item()
    assert ratio <= 1.0, f"quantisation error {ratio:.3f} x half a step"


def quant_inputs(dtype, K=384, rows=37, gain=3.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, K, generator=g) * gain).to(dtype)
    x[5] = 0                       # an all-zero row
    x[9] = 0
    x[9, 17] = -0.37               # a single non-zero
    return x


def exact_int_problem(M, N, K):
    """Asymmetric integer operands exactly representable in e4m3, power-of-two
    scales and an integer bias: every partial sum stays below 2^24, so the f32
    result is exact whatever the accumulation order."""
    A = ((torch.arange(M * K) * 7) % 17 - 8).reshape(M, K).float()
    W = ((torch.arange(N * K) * 5) % 13 - 6).reshape(N, K).float()
    sa = torch.pow(2.0, (torch.arange(M) % 3 - 1).float())
    sw = torch.pow(2.0, (torch.arange(N) % 4 - 2).float())
    bias = (torch.arange(N) % 11 - 5).float()
    want = (A.double() @ W.double().t() * sa.double()[:, None] * sw.double()[None, :] + bias.double()).float()
    return A.to(FP8), W.to(FP8), sa, sw, bias, want


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("gain", [1e-3, 3.0, 200.0])
def test_quantizer_properties(dtype, gain):
    ops = _ops()
    x = quant_inputs(dtype, gain=gain, seed=int(gain * 10) % 7)
    for fn in (ops.quantize_weight_fp8, ops.quantize_fp8_rows_ref):
        q, s = fn(x)
        assert q.shape == x.shape and s.shape == (x.shape[0],)
        check_fp8_rows(x.float(), q, s)
        assert torch.allclose(s, torch.where(x.float().abs().amax(1) > 0, x.float().abs().amax(1) / 448, torch.ones(37)),
                              rtol=1e-6, atol=0)


def test_rms_norm_fp8_ref_properties():
    ops = _ops()
    x = quant_inputs(torch.bfloat16)
    g = (torch.rand(384) + 0.5).to(torch.bfloat16)
    q, s = ops.rms_norm_fp8_ref(x, g, 1e-5)
    y = ops.rms_norm_ref(x.float(), g.float(), 1e-5)
    check_fp8_rows(y, q, s)


@pytest.mark.parametrize("M,N,K", [(48, 80, 128), (130, 136, 384), (17, 16, 1024), (1, 8, 128)])
def test_linear_fp8_ref_exact_integers(M, N, K):
    ops = _ops()
    A, W, sa, sw, bias, want = exact_int_problem(M, N, K)
    y = ops.linear_fp8_ref(A, sa, W, sw, bias=bias.to(torch.bfloat16), out_dtype=torch.float32)
    assert torch.equal(y, want)


def _tiny(quant):
    from ray_dynamic_batching_amd.models.llama import LlamaConfig, LlamaTP

    return LlamaTP(LlamaConfig.tiny(quant=quant), device="cpu", backend="torch", dtype=torch.float32, init="full")


def test_llama_fp8_build_and_fake_quant_forward():
    m, base = _tiny("fp8"), _tiny("none")
    for L in m.layers:
        for k in ("w_qkv", "w_o", "w_gu", "w_down"):
            q, s = L[k]
            assert q.dtype == FP8 and s.dtype == torch.float32 and s.shape == (q.shape[0],)
        assert L["attn_norm"].dtype == torch.float32 and L["mlp_norm"].dtype == torch.float32
    assert m.embed.dtype == torch.float32 and m.lm_head.dtype == torch.float32
    assert m.layer_weight_bytes() < 0.6 * base.layer_weight_bytes()
    assert m.flops_per_prompt() == base.flops_per_prompt()
    ids = m.example_input(2, seed=1)
    out = m(ids)
    assert out.shape == (2, 2) and out.dtype == torch.int32
    h, hb = m.hidden_states(ids), base.hidden_states(ids)
    assert torch.isfinite(h).all()
    assert not torch.equal(h, hb), "quantisation is not on the path"
    # ... and it is a small perturbation of the unquantised network, not another one
    from ray_dynamic_batching_amd.models.reference import rel_err

    assert rel_err(h, hb) < 0.2


def test_llama_fp8_fp32_reference_upcasts_exactly():
    from ray_dynamic_batching_amd.models.reference import fp32_reference

    m = _tiny("fp8")
    r = fp32_reference(m)
    q, s = r.layers[0]["w_qkv"]
    assert q.dtype == torch.float32 and torch.equal(q, m.layers[0]["w_qkv"][0].float())
    ids = m.example_input(1, seed=2)
    assert torch.equal(r.hidden_states(ids), m.hidden_states(ids))


def test_llama_from_hf_quantises_at_load(tmp_path):
    transformers = pytest.importorskip("transformers")
    from ray_dynamic_batching_amd import ops
    from ray_dynamic_batching_amd.models import weights as W

    cfg = transformers.LlamaConfig(vocab_size=512, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, head_dim=64, intermediate_size=512,
                                   max_position_embeddings=128, rope_theta=10000.0, rms_norm_eps=1e-5)
    torch.manual_seed(2)
    transformers.LlamaForCausalLM(cfg).eval().save_pretrained(tmp_path / "llama")
    kw = dict(seq_len=16, device="cpu", dtype=torch.float32, backend="torch")
    plain = W.llama_from_hf(tmp_path / "llama", **kw)
    m = W.llama_from_hf(tmp_path / "llama", quant="fp8", **kw)
    assert m.cfg.quant == "fp8" and plain.cfg.quant == "none"
    for L, P in zip(m.layers, plain.layers):
        for k in ("w_qkv", "w_o", "w_gu", "w_down"):
            q, s = ops.quantize_weight_fp8(P[k])
            assert torch.equal(L[k][0].view(torch.uint8), q.view(torch.uint8)) and torch.equal(L[k][1], s)
    assert torch.equal(m.lm_head, plain.lm_head) and torch.equal(m.embed, plain.embed)
    with pytest.raises(ValueError):
        W.llama_from_hf(tmp_path / "llama", quant="int8", **kw)
    ids = m.example_input(2, seed=1)
    assert m(ids).shape == (2, 2)


def test_llama_config_rejects_unknown_quant():
    from ray_dynamic_batching_amd.models.llama import LlamaConfig

    with pytest.raises(ValueError):
        LlamaConfig(quant="int4")
    with pytest.raises(ValueError):
        LlamaConfig.tiny(quant="fp4")


def test_factory_builds_fp8_llama():
    from ray_dynamic_batching_amd.models import factories

    f = factories.llama3("tiny", quant="fp8", backend="torch")
    m = f(device="cpu")
    assert m.cfg.quant == "fp8" and isinstance(m.layers[0]["w_down"], tuple)
    assert m.layers[0]["w_down"][0].dtype == FP8
