"""CPU: tests/attn_reference.py (the fp64 statement of the attention descriptor that tests/test_gpu_attn_general.py measures the HIP kernels
against) agrees with the three independent statements the repository already has: oracle.bloom_ref.attention_core on the seven
ATT_CASES of test_bloom_attention_fwd_bwd (in fp64: 1e-12), oracle.gpt_ref.attention_core on a left-padded GPT-2 case (in fp32, where
`score + finfo.min` is exactly finfo.min: the quirk rows attend uniformly to the future), and tests/cpu_kernel_emulation.py on a
KV-cache geometry (Sq != Sk) and on an additive mask."""
import math
from types import SimpleNamespace

import pytest
import torch

import attn_reference as AR
import cpu_kernel_emulation as emu
from cleantransformer_amd._lib import AttnDesc
from oracle import bloom_ref as R
from oracle import gpt_ref as GR

FMIN = torch.finfo(torch.float32).min
ATT_CASES = [  # B, S, nh, hd, mask kind: the cases of tests/test_gpu_ops.py::test_bloom_attention_fwd_bwd
    (2, 16, 8, 8, "ones"), (3, 10, 8, 8, "mixed"), (2, 70, 4, 16, "mixed"), (2, 128, 2, 64, "right"),
    (1, 200, 2, 64, "left"), (2, 64, 2, 128, "ones"), (2, 130, 3, 32, "mixed")]


def _mask(kind, B, S):
    am = torch.ones(B, S, dtype=torch.long)
    if kind in ("right", "mixed") and B > 1:
        am[1, (S * 3) // 4:] = 0
    if kind in ("left", "mixed"):
        am[B - 1 if kind == "mixed" and B > 2 else 0, :max(1, S // 3)] = 0
    return am


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _desc(B, nh, Sq, Sk, hd, q_str, k_str, v_str, o_str, scale, causal, am_str=(0, 0, 0, 0), future_fill=0.0):
    d = AttnDesc()
    d.B, d.nh, d.Sq, d.Sk, d.hd = B, nh, Sq, Sk, hd
    d.q_bs, d.q_hs, d.q_rs = q_str
    d.k_bs, d.k_hs, d.k_rs = k_str
    d.v_bs, d.v_hs, d.v_rs = v_str
    d.o_bs, d.o_hs, d.o_rs = o_str
    d.am_b, d.am_h, d.am_q, d.am_k = am_str
    d.scale, d.causal, d.future_fill = float(scale), int(causal), float(future_fill)
    return d


def _with_exact_scale(d, scale):
    """the descriptor's fields with `scale` in full precision (the C struct holds an fp32): the 1e-12 comparison needs the oracle's 1/sqrt(hd)"""
    ns = SimpleNamespace(**{n: getattr(d, n) for n, _ in d._fields_})
    ns.scale = scale
    return ns


def _close(name, got, ref, rel):
    err = float((got - ref).abs().max())
    assert err <= rel * float(ref.abs().max()), f"{name}: max abs err {err:.3e} against max |ref| {float(ref.abs().max()):.3e}"


@pytest.mark.parametrize("B,S,nh,hd,kind", ATT_CASES)
def test_reference_equals_bloom_oracle_in_fp64(B, S, nh, hd, kind):
    H = nh * hd
    qkv, go, am = _rnd(B, S, 3 * H, seed=11).double(), _rnd(B, S, H, seed=12).double(), _mask(kind, B, S)
    qr = qkv.clone().requires_grad_(True)
    alibi = (R.alibi_slopes(nh).double()[..., None] * R.alibi_positions(am)[:, None, :]).reshape(B * nh, 1, S)      # build_alibi, in fp64
    ctx = R.attention_core(qr, alibi, R.causal_key_mask(am, S), nh)[0]
    ctx.backward(go)
    st = (S * 3 * H, 3 * hd, 3 * H)
    d = _with_exact_scale(_desc(B, nh, S, S, hd, st, st, st, (S * H, hd, H), 0.0, True), 1.0 / math.sqrt(hd))
    flat = qkv.reshape(-1)
    r = AR.attn_reference(flat, flat[hd:], flat[2 * hd:], d, R.alibi_slopes(nh), am, None, d_o=go.reshape(-1))
    _close("out", r.out.transpose(1, 2).reshape(B, S, H), ctx.detach(), 1e-12)
    g = qr.grad.view(B, S, nh, 3, hd)
    for i, (name, got) in enumerate((("dq", r.dq), ("dk", r.dk), ("dv", r.dv))):
        _close(name, got.transpose(1, 2), g[:, :, :, i], 1e-12)
    full = (am.cumsum(-1) == 0)                                                      # [B,S]: queries whose whole causal window is padding
    assert torch.equal(r.m <= FMIN, full[:, None, :].expand(B, nh, S))
    assert bool((r.tied[r.m <= FMIN] == S).all()) and bool((r.dq[r.m <= FMIN] == 0).all())
    assert bool((r.dk[(am == 0)[:, None, :].expand(B, nh, S)] == 0).all())


def test_reference_equals_gpt_oracle_left_padded():
    B, S, nh, hd = 2, 37, 2, 16
    H = nh * hd
    qkv, go = _rnd(B, S, 3 * H, seed=5), _rnd(B, S, H, seed=6)
    am = torch.ones(B, S, dtype=torch.long)
    am[0, :5] = 0                                                                     # queries 0..4 of row 0 see only padding in their window
    am[1, 30:] = 0
    qr = qkv.clone().requires_grad_(True)
    q, k, v = (t.view(B, S, nh, hd).transpose(1, 2) for t in qr.split(H, dim=-1))     # GPT-2's blocked layout [q | k | v]
    add = ((1 - am).float() * FMIN).view(B, 1, 1, S)
    ref = GR.attention_core(q, k, v, add)                                             # fp32: -1e4 + finfo.min == finfo.min
    ref.backward(go.view(B, S, nh, hd).transpose(1, 2))
    st = (S * 3 * H, hd, 3 * H)
    d = _desc(B, nh, S, S, hd, st, st, st, (S * H, hd, H), 1.0 / math.sqrt(hd), True, future_fill=-1e4)
    flat = qkv.reshape(-1)
    r = AR.attn_reference(flat, flat[H:], flat[2 * H:], d, None, am, None, d_o=go.reshape(-1))
    _close("out", r.out, ref.detach().double(), 2e-6)
    g = qr.grad.double().view(B, S, 3, nh, hd)
    for i, (name, got) in enumerate((("dq", r.dq), ("dk", r.dk), ("dv", r.dv))):
        _close(name, got.transpose(1, 2), g[:, :, i], 1e-5)
    assert bool((r.m[0, :, :5] == -1e4).all()) and bool((r.tied[0, :, 0] == S - 5).all())   # quirk rows: uniform over the non-padding future


def _emu_pair(q, k, v, o_shape, go, d, slopes, am, add_mask):
    """cpu_kernel_emulation's forward and backward on fp32 copies of the same storage"""
    mask = emu.MaskInfo(am) if am is not None else None
    out = torch.zeros(o_shape)
    sm, sl = emu.attn_fwd(q, k, v, out, d, slopes, mask, add_mask)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    emu.attn_bwd(q, k, v, out, go, sm, sl, dq, dk, dv, d, slopes, mask, add_mask)
    return out, sm, sl, dq, dk, dv


def test_reference_agrees_with_kernel_emulation_on_cache_geometry():
    B, nh, hd, Sq, Sk = 2, 2, 16, 5, 23
    H = nh * hd
    qkv, kc, vc, go = _rnd(B * Sq * 3 * H, seed=1), _rnd(B, nh, Sk, hd, seed=2), _rnd(B, nh, Sk, hd, seed=3), _rnd(B * Sq * H, seed=4)
    am = torch.ones(B, Sk, dtype=torch.long)
    am[0, :20] = 0                                                                    # longer than Sk - Sq: queries 0, 1 see only padding
    am[1, 21:] = 0
    cs = (nh * Sk * hd, Sk * hd, hd)
    d = _desc(B, nh, Sq, Sk, hd, (Sq * 3 * H, 3 * hd, 3 * H), cs, cs, (Sq * H, hd, H), 1.0 / math.sqrt(hd), True)
    slopes = R.alibi_slopes(nh)
    out, sm, sl, dq, dk, dv = _emu_pair(qkv, kc, vc, (B * Sq * H,), go, d, slopes, am, None)
    r = AR.attn_reference(qkv, kc, vc, d, slopes, am, None, d_o=go)
    vq, vk, vv, vo = AR.operand_views(d, dq, dk, dv, out)
    for name, got, ref in (("out", vo, r.out), ("dq", vq, r.dq), ("dk", vk, r.dk), ("dv", vv, r.dv)):
        _close(name, got.double(), ref, 1e-5)
    assert torch.equal(sm <= FMIN, r.m <= FMIN) and int((r.m <= FMIN).sum()) == 2 * nh
    _close("lse", (sm.double() + sl.double().log())[r.m > FMIN], r.lse[r.m > FMIN], 1e-5)


def test_reference_agrees_with_kernel_emulation_on_additive_mask():
    B, nh, hd, S = 2, 2, 16, 19
    H = nh * hd
    q, k, v, go = (_rnd(B * S * H, seed=s) for s in (1, 2, 3, 4))
    add = torch.where(_rnd(S, S, seed=9) > 0.5, torch.tensor(-1e4), torch.tensor(0.0))
    add[:, 0] = 0.0
    add[:, 10:] = float("-inf")
    am4 = add.reshape(1, 1, S, S).expand(B, nh, S, S)
    st = (S * H, hd, H)
    d = _desc(B, nh, S, S, hd, st, st, st, st, 1.0 / math.sqrt(hd), False, am_str=tuple(am4.stride()))
    out, sm, sl, dq, dk, dv = _emu_pair(q, k, v, (B * S * H,), go, d, None, None, am4)
    r = AR.attn_reference(q, k, v, d, None, None, am4, d_o=go)
    vq, vk, vv, vo = AR.operand_views(d, dq, dk, dv, out)
    for name, got, ref in (("out", vo, r.out), ("dq", vq, r.dq), ("dk", vk, r.dk), ("dv", vv, r.dv)):
        _close(name, got.double(), ref, 1e-5)
    _close("m", sm.double(), r.m, 1e-5)
    _close("lse", sm.double() + sl.double().log(), r.lse, 1e-5)
