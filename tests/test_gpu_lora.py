"""GPU (-m gpu): low-rank adapters — the three kernel families of csrc/lora.hip against fp64 torch, and the adapter block path of
models/modeling_bloom.py against the CPU oracle through the identity  adapted model == base model with W' = W + scaling * B A:
R.loss_and_grads on the merged weights gives loss, logits and dW', and the adapter gradients are dA = scaling * B^T dW', dB = scaling * dW' A^T.

Kernel error bound (derived, not tuned).  Inputs are exact in fp64.  With fp32 accumulation over n terms and one rounding to the storage dtype,
    |got - ref| <= 2 * u * |ref| + n * 2^-23 * sum_k |a_k| |b_k|,        u = 2^-9 (bf16), 2^-12 (fp16), 0 for the fp32-output weight gradient.
The first term is the unit roundoff of the storage dtype (half an ulp at the bottom of a binade: 2^-8 for bf16's 8 significant bits, 2^-11 for
fp16's 11), the second twice the worst case of a length-n fp32 sum (n * 2^-24 * sum|a_k||b_k|, which also covers the rounding being applied to the
fp32 value instead of the exact one).  For expand-add the old value of Y counts as one more term.
"""
import functools
import math

import numpy as np
import pytest
import torch

import golden_npz

pytestmark = pytest.mark.gpu

from oracle import bloom_ref as R  # noqa: E402

DEV = "cuda:0"
TINY = golden_npz.load("tiny_bloom")
U = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}
SHAPES = [(1, 64, 64, 8), (200, 256, 768, 16), (1024, 1024, 3072, 64)]                 # (T, K, N, r)
SENTINEL = -77.0
PAD = 8                                                                               # extra columns (ld = N + 8) and 3 extra rows around every output


def T_(a):
    return torch.from_numpy(np.asarray(a))


def _rand(shape, dtype, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


@functools.lru_cache(maxsize=None)
def _case(dtype, shape):
    """inputs (CPU, storage dtype — exact in fp64) of one shape, made once and shared by the kernel tests; never modified"""
    Tn, K, N, r = shape
    s = 100 * SHAPES.index(shape) + (0 if dtype == torch.bfloat16 else 50)
    return dict(x=_rand((Tn, K), dtype, s + 1), a=_rand((r, K), dtype, s + 2, K ** -0.5), xa=_rand((Tn, r), dtype, s + 3),
                b=_rand((N, r), dtype, s + 4, r ** -0.5), y=_rand((Tn, N), dtype, s + 5), dy=_rand((Tn, N), dtype, s + 6))


def _framed(rows, cols, dtype, fill=None):
    """a [rows, cols] window at the top left of a sentinel-filled [rows + 3, cols + PAD] buffer"""
    buf = torch.full((rows + 3, cols + PAD), SENTINEL, dtype=dtype, device=DEV)
    win = buf[:rows, :cols]
    if fill is not None:
        win.copy_(fill)
    return buf, win


def _frame_untouched(buf, rows, cols):
    ref = torch.full_like(buf, SENTINEL)
    bits = {2: torch.int16, 4: torch.int32}[buf.element_size()]
    a, b = buf.view(bits).clone(), ref.view(bits)
    a[:rows, :cols] = b[:rows, :cols]
    return torch.equal(a, b)


def _check(name, got, ref, absprod, n, u):
    got = got.detach().double().cpu()
    err = (got - ref).abs()
    bound = 2 * u * ref.abs() + n * 2.0 ** -23 * absprod
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: max err {float(err.max()):.3e}, worst err/bound {worst:.3f}")
    assert torch.isfinite(got).all(), name
    assert (err <= bound).all(), f"{name}: {int((err > bound).sum())}/{err.numel()} beyond the bound, worst err/bound {worst:.3f}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d-K%d-N%d-r%d" % s)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_project_both_layouts(dtype, shape):
    from cleantransformer_amd import ops
    Tn, K, N, r = shape
    c = _case(dtype, shape)
    # forward layout: out = alpha * x A^T, A [r, K]
    x, a = c["x"].double(), c["a"].double()
    buf, out = _framed(Tn, r, dtype)
    ops.lora_project(c["x"].to(DEV), c["a"].to(DEV), False, alpha=2.0, out=out)
    _check("project [r,K]", out, 2.0 * (x @ a.T), 2.0 * (x.abs() @ a.abs().T), K, U[dtype])
    assert _frame_untouched(buf, Tn, r)
    # backward layout: dxa = alpha * dy B, B [N, r] read k-major (the reduction runs over N)
    dy, b = c["dy"].double(), c["b"].double()
    buf, out = _framed(Tn, r, dtype)
    ops.lora_project(c["dy"].to(DEV), c["b"].to(DEV), True, alpha=0.5, out=out)
    _check("project [K,r]", out, 0.5 * (dy @ b), 0.5 * (dy.abs() @ b.abs()), N, U[dtype])
    assert _frame_untouched(buf, Tn, r)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d-K%d-N%d-r%d" % s)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_expand_add_both_layouts_in_place_inside_a_wider_buffer(dtype, shape):
    from cleantransformer_amd import ops
    Tn, K, N, r = shape
    c = _case(dtype, shape)
    xa, y0 = c["xa"].double(), c["y"].double()
    # forward layout: y += xa B^T, B [N, r]
    b = c["b"].double()
    buf, y = _framed(Tn, N, dtype, c["y"])
    assert ops.lora_expand_add(c["xa"].to(DEV), c["b"].to(DEV), y, False) is y
    _check("expand-add [N,r]", y, y0 + xa @ b.T, y0.abs() + xa.abs() @ b.abs().T, r + 1, U[dtype])
    assert _frame_untouched(buf, Tn, N)
    # backward layout: dx += dxa A with A [r, N'] (N' = K of the forward: the other wide extent of the shape)
    a = c["a"].double()
    x0 = c["x"].double()
    buf, y = _framed(Tn, K, dtype, c["x"])
    ops.lora_expand_add(c["xa"].to(DEV), c["a"].to(DEV), y, True)
    _check("expand-add [r,N]", y, x0 + xa @ a, x0.abs() + xa.abs() @ a.abs(), r + 1, U[dtype])
    assert _frame_untouched(buf, Tn, K)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d-K%d-N%d-r%d" % s)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_skinny_weight_gradient_both_orientations(dtype, shape):
    from cleantransformer_amd import ops
    Tn, K, N, r = shape
    c = _case(dtype, shape)
    # dB [N, r] = alpha * dy^T xa  (the wide operand on the left)
    dy, xa = c["dy"].double(), c["xa"].double()
    buf, out = _framed(N, r, torch.float32)
    ops.lora_wgrad(c["dy"].to(DEV), c["xa"].to(DEV), alpha=2.0, out=out)
    _check("wgrad [N,r]", out, 2.0 * (dy.T @ xa), 2.0 * (dy.abs().T @ xa.abs()), Tn, 0.0)
    assert _frame_untouched(buf, N, r)
    # dA [r, K] = dxa^T x  (the wide operand on the right)
    x = c["x"].double()
    buf, out = _framed(r, K, torch.float32)
    ops.lora_wgrad(c["xa"].to(DEV), c["x"].to(DEV), out=out)
    _check("wgrad [r,K]", out, xa.T @ x, xa.abs().T @ x.abs(), Tn, 0.0)
    assert _frame_untouched(buf, r, K)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_skinny_weight_gradient_is_bit_identical_from_run_to_run(dtype):
    from cleantransformer_amd import ops
    c = _case(dtype, SHAPES[2])
    dy, xa, x = c["dy"].to(DEV), c["xa"].to(DEV), c["x"].to(DEV)
    assert torch.equal(ops.lora_wgrad(dy, xa, alpha=0.25), ops.lora_wgrad(dy, xa, alpha=0.25))
    assert torch.equal(ops.lora_wgrad(xa, x), ops.lora_wgrad(xa, x))


def test_calls_outside_the_contract_are_refused_before_any_launch():
    import ctypes as C
    from cleantransformer_amd import _lib, ops
    lib = _lib.load()
    p, st = (lambda t: C.c_void_p(t.data_ptr())), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bf = torch.bfloat16
    big = torch.ones((64, 128), dtype=bf, device=DEV)
    w = torch.ones((64, 128), dtype=bf, device=DEV)
    out = torch.full((64, 128), SENTINEL, dtype=bf, device=DEV)
    out32 = torch.full((128, 128), SENTINEL, dtype=torch.float32, device=DEV)
    ws = torch.full((1 << 16,), SENTINEL, dtype=torch.float32, device=DEV)
    UNS = -3                                                                          # CTMI_ERR_UNSUPPORTED
    # r = 12, K = 60 (and N / P / Q = 60): each against otherwise valid arguments
    assert lib.ctmi_lora_project(p(big), 128, p(w), 128, 0, p(out), 128, 64, 64, 12, 1.0, _lib.BF16, st) == UNS
    assert b"r = 12" in lib.ctmi_last_error()
    assert lib.ctmi_lora_project(p(big), 128, p(w), 128, 0, p(out), 128, 64, 60, 16, 1.0, _lib.BF16, st) == UNS
    assert lib.ctmi_lora_project(p(big), 128, p(w), 128, 1, p(out), 128, 64, 60, 16, 1.0, _lib.BF16, st) == UNS
    assert lib.ctmi_lora_project(p(big), 60, p(w), 128, 0, p(out), 128, 64, 64, 16, 1.0, _lib.BF16, st) == UNS          # a leading dimension that breaks 16-byte rows
    assert lib.ctmi_lora_project(p(big), 128, p(w), 128, 0, p(out), 128, 64, 64, 16, 1.0, _lib.F32, st) == UNS
    assert lib.ctmi_lora_expand_add(p(big), 128, p(w), 128, 0, p(out), 128, 64, 64, 12, _lib.BF16, st) == UNS
    assert lib.ctmi_lora_expand_add(p(big), 128, p(w), 128, 0, p(out), 128, 64, 60, 16, _lib.BF16, st) == UNS
    assert lib.ctmi_lora_expand_add(p(big), 128, p(w), 128, 0, p(out), 128, 0, 64, 16, _lib.BF16, st) == UNS
    assert lib.ctmi_lora_wgrad(p(big), 128, p(w), 128, p(out32), 128, 64, 12, 64, 1.0, p(ws), ws.numel() * 4, _lib.BF16, st) == UNS
    assert lib.ctmi_lora_wgrad(p(big), 128, p(w), 128, p(out32), 128, 64, 16, 60, 1.0, p(ws), ws.numel() * 4, _lib.BF16, st) == UNS
    assert lib.ctmi_lora_wgrad(p(big), 128, p(w), 128, p(out32), 128, 64, 128, 128, 1.0, p(ws), ws.numel() * 4, _lib.BF16, st) == UNS   # min(P, Q) > 64
    assert lib.ctmi_lora_wgrad(p(big), 128, p(w), 128, p(out32), 128, 64, 16, 64, 1.0, p(ws), 64, _lib.BF16, st) == UNS               # workspace too small
    torch.cuda.synchronize()
    for t in (out, out32, ws):                                                        # nothing ran: every output still holds the sentinel
        assert bool((t == SENTINEL).all())
    with pytest.raises(_lib.CtmiError, match="status -3"):
        ops.lora_project(torch.ones((4, 64), dtype=bf, device=DEV), torch.ones((12, 64), dtype=bf, device=DEV))


# ------------------------------------------------------------------------------------------------ the model
PATH = {"query_key_value": "self_attention.query_key_value", "dense": "self_attention.dense", "dense_4h_to_h": "mlp.dense_4h_to_h"}
QKV, ALL = ("query_key_value",), ("query_key_value", "dense", "dense_4h_to_h")
R_, ALPHA = 8, 16.0
SCALING = ALPHA / R_


def tiny_shape():
    return [int(v) for v in TINY["cfg"]]


def build(V, H, L, nh, compute_dtype="fp32", params=None):
    from cleantransformer_amd.models.modeling_bloom import BloomConfig, BloomForCausalLM
    cfg = BloomConfig(vocab_size=V, hidden_size=H, n_layer=L, num_attention_heads=nh, compute_dtype=compute_dtype)
    m = BloomForCausalLM(cfg)
    m._tie_weight()
    sd = dict(params if params is not None else R.det_init(R.BloomShape(V, H, L, nh)))
    sd["lm_head.weight"] = sd["bloom.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    m._tie_weight()
    return m.to(DEV).train()


def adapter_values(V, H, L, nh, targets):
    """{key: fp32 CPU tensor}: A and B both random, so that B != 0 and every product of the adapter path carries signal"""
    out = {}
    dims = {"query_key_value": (H, 3 * H), "dense": (H, H), "dense_4h_to_h": (4 * H, H)}
    k = 0
    for i in range(L):
        for t in targets:
            fin, fout = dims[t]
            pre = f"bloom.blocks.{i}.{PATH[t]}"
            out[pre + ".lora_A.weight"] = _rand((R_, fin), torch.float32, 500 + k, fin ** -0.5)
            out[pre + ".lora_B.weight"] = _rand((fout, R_), torch.float32, 600 + k, 0.05)
            k += 1
    return out


def adapted(V, H, L, nh, targets, compute_dtype="fp32", ad=None):
    from cleantransformer_amd.lora import LoraConfig, apply_lora, load_lora_state_dict
    m = apply_lora(build(V, H, L, nh, compute_dtype), LoraConfig(r=R_, lora_alpha=ALPHA, target_modules=targets))
    load_lora_state_dict(m, ad if ad is not None else adapter_values(V, H, L, nh, targets))
    return m


def merged_params(base, ad):
    """fp64 parameters of the equivalent plain model: W' = W + scaling * B A"""
    p = {k: v.double() for k, v in base.items()}
    for k in ad:
        if k.endswith(".lora_A.weight"):
            pre = k[:-len(".lora_A.weight")]
            p[pre + ".weight"] = p[pre + ".weight"] + SCALING * (ad[pre + ".lora_B.weight"].double() @ ad[k].double())
    return p


def expected_adapter_grads(ad, grads):
    out = {}
    for k in ad:
        if k.endswith(".lora_A.weight"):
            pre = k[:-len(".lora_A.weight")]
            dw = grads[pre + ".weight"].double()
            out[k] = SCALING * (ad[pre + ".lora_B.weight"].double().T @ dw)
            out[pre + ".lora_B.weight"] = SCALING * (dw @ ad[k].double().T)
    return out


@functools.lru_cache(maxsize=None)
def tiny_oracle(targets):
    """(adapter values, oracle loss / logits / expected adapter gradients) for the tiny golden shape — computed once per target set"""
    V, H, L, nh, B, S = tiny_shape()
    sh = R.BloomShape(V, H, L, nh)
    ad = adapter_values(V, H, L, nh, targets)
    loss, logits, _, grads = R.loss_and_grads(merged_params(R.det_init(sh), ad), sh, T_(TINY["ids"]), T_(TINY["mask"]))
    return ad, float(loss), logits, expected_adapter_grads(ad, grads)


def close(name, got, ref, rtol, atol=0.0):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert torch.isfinite(got).all(), name
    assert not bad.any(), f"{name}: {int(bad.sum())}/{bad.numel()} off, worst {float(err.max()):.3e}, ref scale {float(ref.abs().max()):.3e}"


def _forward_backward(m, ids, am):
    (loss, logits, _), _ = m(input_ids=ids, attention_mask=am, labels=ids.clone())
    loss.backward()
    return loss.detach(), logits.detach()


@pytest.mark.parametrize("targets", [QKV, ALL], ids=["qkv", "all"])
def test_tiny_fp32_matches_the_merged_weight_oracle(targets):
    V, H, L, nh, B, S = tiny_shape()
    ad, loss_o, logits_o, g_o = tiny_oracle(targets)
    m = adapted(V, H, L, nh, targets, ad=ad)
    ids, am = T_(TINY["ids"]).to(DEV), T_(TINY["mask"]).to(DEV)
    loss, logits = _forward_backward(m, ids, am)
    close("loss", loss, loss_o, 1e-5)
    close("logits", logits, logits_o, 1e-4, 2e-6)
    named = dict(m.named_parameters())
    assert set(g_o) == {n for n, p in named.items() if p.requires_grad}
    for n, p in named.items():
        if n in g_o:
            close("grad " + n, p.grad, g_o[n], 2e-4, 2e-7)
        else:
            assert p.grad is None, n                                                  # the base is frozen: nothing was computed for it


def _bf16_compare(m, ids, am, loss_o, g_o):
    loss, _ = _forward_backward(m, ids, am)
    print(f"bf16 loss {float(loss):.6f} vs {loss_o:.6f}")
    assert abs(float(loss) - loss_o) <= 3e-3 * abs(loss_o), (float(loss), loss_o)
    worst = (0.0, "")
    for n, p in m.named_parameters():
        if n in g_o:
            ref = g_o[n]
            rel = float((p.grad.double().cpu() - ref).abs().max() / ref.abs().max())
            worst = max(worst, (rel, n))
        else:
            assert p.grad is None, n
    print(f"bf16 worst adapter-gradient error relative to the gradient's max: {worst[0]:.3e} ({worst[1]})")
    assert worst[0] <= 4e-2, worst


@pytest.mark.parametrize("targets", [QKV, ALL], ids=["qkv", "all"])
def test_tiny_bf16_matches_the_merged_weight_oracle(targets):
    V, H, L, nh, B, S = tiny_shape()
    ad, loss_o, _, g_o = tiny_oracle(targets)
    m = adapted(V, H, L, nh, targets, "bf16", ad=ad)
    _bf16_compare(m, T_(TINY["ids"]).to(DEV), T_(TINY["mask"]).to(DEV), loss_o, g_o)


def test_one_block_bf16_fast_attention_path_and_ragged_rows():
    """H = 256, nh = 4 (head_dim 64: the 128-row attention kernels), B = 2, S = 250: T = 500 rows, no multiple of any tile"""
    V, H, L, nh, B, S = 512, 256, 1, 4, 2, 250
    sh = R.BloomShape(V, H, L, nh)
    ad = adapter_values(V, H, L, nh, ALL)
    ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(5))
    am = torch.ones(B, S, dtype=torch.long)
    am[1, 231:] = 0
    loss_o, _, _, grads = R.loss_and_grads(merged_params(R.det_init(sh), ad), sh, ids, am)
    m = adapted(V, H, L, nh, ALL, "bf16", ad=ad)
    _bf16_compare(m, ids.to(DEV), am.to(DEV), float(loss_o), expected_adapter_grads(ad, grads))


@pytest.mark.parametrize("targets", [QKV, ALL], ids=["qkv", "all"])
def test_merged_model_on_the_one_call_block_path_gives_the_same_loss(targets):
    from cleantransformer_amd.lora import merge_lora
    from cleantransformer_amd.models import modeling_bloom as MB
    V, H, L, nh, B, S = tiny_shape()
    m = adapted(V, H, L, nh, targets)
    ids, am = T_(TINY["ids"]).to(DEV), T_(TINY["mask"]).to(DEV)
    with torch.no_grad():
        (loss_a, _, _), _ = m(input_ids=ids, attention_mask=am, labels=ids.clone())
    merge_lora(m)
    assert not any(".lora_" in k for k in m.state_dict())
    calls = []
    orig = MB.BloomBlockFn.forward
    try:
        MB.BloomBlockFn.forward = staticmethod(lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
        (loss_m, _, _), _ = m(input_ids=ids, attention_mask=am, labels=ids.clone())
    finally:
        MB.BloomBlockFn.forward = staticmethod(orig)
    assert len(calls) == L                                                            # the plain one-call block path again
    lm, la = float(loss_m.detach()), float(loss_a)
    assert abs(lm - la) <= 1e-5 * abs(la), (lm, la)
    loss_m.backward()
    assert all(p.grad is not None for p in m.parameters())                            # and everything trains again


def test_five_adamw_steps_fp32_follow_the_cpu_trajectory():
    """expected trajectory on the CPU: R.loss_and_grads on the merged weights, the chain rule, R.adamw_update on A and B only"""
    from cleantransformer_amd.optimizer import AdamW
    V, H, L, nh, B, S = tiny_shape()
    sh = R.BloomShape(V, H, L, nh)
    base = R.det_init(sh)
    ad = {k: v.double() for k, v in adapter_values(V, H, L, nh, ALL).items()}
    ids_c, am_c = T_(TINY["ids"]), T_(TINY["mask"])
    lr, wd = 1e-3, 0.01
    m = adapted(V, H, L, nh, ALL)
    trainable = [p for p in m.parameters() if p.requires_grad]
    opt = AdamW(m.parameters(), lr=lr, weight_decay=wd, decoupled=True)               # the whole list: frozen parameters never get a gradient and are skipped
    ids, am = ids_c.to(DEV), am_c.to(DEV)
    mom = {k: torch.zeros_like(v) for k, v in ad.items()}
    var = {k: torch.zeros_like(v) for k, v in ad.items()}
    frozen_before = {n: p.detach().clone() for n, p in m.named_parameters() if not p.requires_grad}
    for t in range(1, 6):
        loss_o, _, _, grads = R.loss_and_grads(merged_params(base, ad), sh, ids_c, am_c)
        g = expected_adapter_grads(ad, grads)
        for k in ad:
            R.adamw_update(ad[k], g[k].clone(), mom[k], var[k], t, lr, 0.9, 0.999, 1e-8, wd, True)
        (loss, _, _), _ = m(input_ids=ids, attention_mask=am, labels=ids.clone())
        opt.zero_grad()
        loss.backward()
        opt.step()
        got = float(loss.detach())
        print(f"step {t}: loss {got:.7f} vs {float(loss_o):.7f}")
        assert abs(got - float(loss_o)) <= 1e-4 * float(loss_o), (t, got, float(loss_o))
    assert len(trainable) == 2 * len(ALL) * L
    for n, p in m.named_parameters():
        if n in frozen_before:
            assert torch.equal(p, frozen_before[n]), n


def test_frozen_base_launches_no_weight_gradient_work(monkeypatch):
    from cleantransformer_amd import ops
    from cleantransformer_amd.optimizer import AdamW
    V, H, L, nh, B, S = tiny_shape()
    assert L == 2
    counts = {}

    def counted(name):
        orig = getattr(ops, name)
        counts[name] = 0

        def f(*a, **k):
            counts[name] += 1
            return orig(*a, **k)
        monkeypatch.setattr(ops, name, f)

    for name in ("linear_wgrad", "wgrad_grouped", "colsum", "embed_bwd"):
        counted(name)
    ids, am = T_(TINY["ids"]).to(DEV), T_(TINY["mask"]).to(DEV)

    def step(m):
        for k in counts:
            counts[k] = 0
        opt = AdamW(m.parameters(), lr=1e-3, decoupled=True)
        (loss, _, _), _ = m(input_ids=ids, attention_mask=am, labels=ids.clone())
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert math.isfinite(float(loss.detach()))
        return dict(counts)

    assert step(adapted(V, H, L, nh, ALL)) == {"linear_wgrad": 0, "wgrad_grouped": 0, "colsum": 0, "embed_bwd": 0}
    # the same model without adapters, every matrix frozen by hand (LayerNorm parameters and biases still train): the LM head computes no [V,H] gradient
    m = build(V, H, L, nh)
    for p in m.parameters():
        if p.dim() == 2:
            p.requires_grad_(False)
    got = step(m)
    assert got["linear_wgrad"] == 0 and got["embed_bwd"] == 0, got
    assert m.lm_head.weight.grad is None
    # and the counters do count: the trainable model takes both
    got = step(build(V, H, L, nh))
    assert got["linear_wgrad"] >= 1 and got["embed_bwd"] == 1, got


def test_greedy_decode_through_the_kv_cache_equals_the_merged_model():
    from cleantransformer_amd.lora import merge_lora
    V, H, L, nh, B, S = tiny_shape()
    # B ten times the size used elsewhere: on the CPU oracle that is what it takes for the merged weights to decode other tokens than the base model
    ad = {k: (v * 10.0 if ".lora_B." in k else v) for k, v in adapter_values(V, H, L, nh, ALL).items()}
    m = adapted(V, H, L, nh, ALL, ad=ad).eval()
    prompt, mask = T_(TINY["greedy_prompt"]).to(DEV), T_(TINY["greedy_mask"]).to(DEV)
    cfg = dict(beam_size=1, max_gen_len=6, do_sample=False, end_ids=None, pad_id=3)       # the reference's loop emits max_gen_len + 2 = 8 new tokens
    out_a = m.generate(prompt, attention_mask=mask, generation_configs=cfg).cpu()
    assert out_a.shape[-1] == prompt.shape[-1] + 8
    base = build(V, H, L, nh).eval().generate(prompt, attention_mask=mask, generation_configs=cfg).cpu()
    out_m = merge_lora(m).eval().generate(prompt, attention_mask=mask, generation_configs=cfg).cpu()
    assert torch.equal(out_a, out_m)
    assert not torch.equal(out_a, base)                                               # the adapters do change what is decoded


def test_what_is_out_of_scope_raises_or_falls_back():
    from cleantransformer_amd.graph import GraphedStep
    from cleantransformer_amd.optimizer import AdamW
    from cleantransformer_amd.trainer.ddp import DistributedDataParallel
    V, H, L, nh, B, S = tiny_shape()
    m = adapted(V, H, L, nh, QKV)
    ids, am = T_(TINY["ids"]).to(DEV), T_(TINY["mask"]).to(DEV)
    with pytest.raises(NotImplementedError, match="adapters"):
        DistributedDataParallel(m)
    step = GraphedStep(m, AdamW(m.parameters(), lr=1e-3, decoupled=True), warmup=1)
    losses = [float(step(ids, am, ids.clone())) for _ in range(3)]
    assert step.replays == 0 and step.graph is None and "adapters" in step.fallback_reason
    assert losses[2] < losses[0]
    for blk in m.bloom.blocks:
        blk.hidden_dropout = 0.1
    with pytest.raises(NotImplementedError, match="dropout"):
        m(input_ids=ids, attention_mask=am, labels=ids.clone())
