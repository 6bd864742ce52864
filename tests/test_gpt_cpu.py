"""CPU (no GPU): the GPT / GPT-2 path (BASELINE configs[3]; reference CleanTransformer/models/modeling_gpt.py).
 1. the oracle restatement (oracle/gpt_ref.py) against golden vectors produced by the reference's own GPTLMHeadModel
    (tests/golden/make_golden.py gpt -> tiny_gpt.npz): logits, every gradient, AdamW trajectory, greedy tokens;
 2. the product's host logic (Conv1D transposed compute copies, q|k|v strides, pre-/post-LN blocks, tied head, KV-cache
    loop) through the torch-CPU emulation of the kernel contracts, against the same goldens."""
import os

import numpy as np
import pytest
import torch

import cpu_kernel_emulation as emu
import golden_npz
from oracle import gpt_ref as GR
from oracle.bloom_ref import AdamState

G = os.path.join(os.path.dirname(__file__), "golden")
GPT = golden_npz.load("tiny_gpt")


def T(a):
    return torch.from_numpy(np.asarray(a))


def close(name, a, b, rtol=1e-5, atol=1e-7):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert torch.allclose(a, b, rtol=rtol, atol=atol), (name, float((a - b).abs().max()))


def close_params(n, a, b, rtol, atol):
    """Parameters after AdamW steps.  The key third of c_attn.bias has a mathematically ZERO gradient (softmax is invariant
    to a per-query constant), so what reaches Adam is rounding noise that m/sqrt(v) normalises into +-lr steps of arbitrary
    sign: that slice is compared with a 3-step*lr allowance, everything else tightly."""
    a, b = torch.as_tensor(a).detach(), torch.as_tensor(b)
    if n.endswith("attn.c_attn.bias"):
        H = a.numel() // 3
        close("p3_" + n + "[k]", a[H:2 * H], b[H:2 * H], 0.0, 7e-5)
        a, b = torch.cat((a[:H], a[2 * H:])), torch.cat((b[:H], b[2 * H:]))
    close("p3_" + n, a, b, rtol, atol)


def shape(version):
    V, H, L, nh, P, B, S = [int(v) for v in GPT["cfg"]]
    return GR.GPTShape(V, H, L, nh, P, version=version)


@pytest.mark.parametrize("version", ["gpt2", "gpt"])
def test_gpt_oracle_matches_reference_golden(version):
    s = shape(version)
    assert list(GPT[f"{version}_names"]) == GR.param_names(s)              # the reference's named_parameters() order
    p = GR.det_init(s)
    ids, am = T(GPT["ids"]), T(GPT["mask"])
    loss, logits, hidden, grads = GR.loss_and_grads(p, s, ids, am)
    close("loss0", loss, GPT[f"{version}_loss0"], 1e-6)
    close("logits0", logits, GPT[f"{version}_logits0"], 1e-5, 1e-6)
    close("hidden0", hidden, GPT[f"{version}_hidden0"], 1e-5, 1e-6)
    for n, g in grads.items():
        close("g0_" + n, g, GPT[f"{version}_g0_" + n], 1e-4, 1e-8)
    st = AdamState(p)
    for t in range(3):
        lo, gn = GR.train_step(p, s, ids, am, st)
        assert abs(lo - GPT[f"{version}_traj"][t, 0]) <= 1e-6 * lo and abs(gn - GPT[f"{version}_traj"][t, 1]) <= 1e-5 * gn, (t, lo, gn)
    for n in p:
        close_params(n, p[n], GPT[f"{version}_p3_" + n], 1e-6, 1e-8)


def test_gpt_oracle_greedy_decode_bit_exact():
    s = shape("gpt2")
    out = GR.greedy_decode(GR.det_init(s), s, T(GPT["greedy_prompt"]), torch.ones(2, 7, dtype=torch.long), max_gen_len=6)
    assert np.array_equal(out.numpy(), GPT["greedy_out"])


def build(version, cd="fp32"):
    from cleantransformer_amd.models.modeling_gpt import GPTConfig, GPTLMHeadModel
    V, H, L, nh, P, B, S = [int(v) for v in GPT["cfg"]]
    cfg = GPTConfig(vocab_size=V, n_embd=H, n_positions=P, n_layer=L, n_head=nh, n_ctx=P, embd_pdrop=0.0, attn_pdrop=0.0,
                    resid_pdrop=0.0, compute_dtype=cd)
    m = GPTLMHeadModel(cfg, version=version)
    sd = dict(GR.det_init(shape(version)))
    sd["lm_head.weight"] = sd["gpt.tokens_embed.weight"]
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("attn.bias") for k in missing), (missing, unexpected)   # only the tril buffers
    m._tie_weights()
    for blk in m.gpt.blocks:
        blk.mlp[3].p = 0.0
    return m.train()


@pytest.mark.parametrize("version", ["gpt2", "gpt"])
def test_gpt_host_logic_vs_reference_golden(monkeypatch, version):
    emu.install(monkeypatch)
    from cleantransformer_amd.optimizer import AdamW
    m = build(version)
    assert [n for n, _ in m.named_parameters()] == list(GPT[f"{version}_names"])   # same names, same order as the reference
    ids, am = T(GPT["ids"]), T(GPT["mask"])
    opt = AdamW(m.parameters(), lr=1e-5, weight_decay=0.01, decoupled=True)
    for t in range(3):
        (loss, logits, hidden), _ = m(ids, attention_mask=am, labels=ids.clone())
        opt.zero_grad()
        loss.backward()
        gn = float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in m.parameters())))
        if t == 0:
            close("logits0", logits, GPT[f"{version}_logits0"], 1e-4, 1e-6)
            close("hidden0", hidden, GPT[f"{version}_hidden0"], 1e-4, 1e-6)
            for n, p in m.named_parameters():
                close("g0_" + n, p.grad, GPT[f"{version}_g0_" + n], 1e-4, 1e-8)
        opt.step()
        assert abs(float(loss) - GPT[f"{version}_traj"][t, 0]) <= 1e-5 * float(loss), (t, float(loss))
        assert abs(gn - GPT[f"{version}_traj"][t, 1]) <= 1e-4 * gn, (t, gn)
    for n, p in m.named_parameters():
        close_params(n, p, GPT[f"{version}_p3_" + n], 1e-5, 2e-7)


def test_gpt_host_logic_greedy_decode_bit_exact(monkeypatch):
    emu.install(monkeypatch)
    m = build("gpt2").eval()
    out = m.generate(T(GPT["greedy_prompt"]), attention_mask=torch.ones(2, 7, dtype=torch.long),
                     generation_configs=dict(beam_size=1, max_gen_len=6, do_sample=False, end_ids=None, pad_id=3))
    assert np.array_equal(out.numpy(), GPT["greedy_out"])


LP = np.load(os.path.join(G, "tiny_gpt_leftpad.npz"))


def test_gpt_left_padding_oracle_and_host_logic_vs_reference_golden(monkeypatch):
    """LEFT-padded batch (tests/golden/make_golden.py gpt_leftpad): rows whose whole causal window is padding attend to the FUTURE
    in the reference (``w*b - 1e4*(1-b)`` leaves -1e4 on future keys, modeling_gpt.py:88-93).  Round 1 documented this as a
    deviation; the attention entry points now take the fill value (ctmi_attn_desc.future_fill = -1e4)."""
    s = shape("gpt2")
    ids, am = T(LP["ids"]), T(LP["mask"])
    p = GR.det_init(s)
    loss, logits, _, grads = GR.loss_and_grads(p, s, ids, am)
    close("oracle.loss", loss, LP["loss0"], 1e-6)
    close("oracle.logits", logits, LP["logits0"], 1e-5, 1e-6)
    for n, g in grads.items():
        close("oracle.g0_" + n, g, LP["g0_" + n], 1e-4, 1e-8)
    emu.install(monkeypatch)
    m = build("gpt2")
    (l2, lg2, _), _ = m(ids, attention_mask=am, labels=ids.clone())
    l2.backward()
    close("host.loss", l2, LP["loss0"], 1e-5)
    close("host.logits", lg2, LP["logits0"], 1e-4, 1e-6)
    for n, prm in m.named_parameters():
        close("host.g0_" + n, prm.grad, LP["g0_" + n], 1e-4, 1e-8)
