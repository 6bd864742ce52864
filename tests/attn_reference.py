"""TEST INFRASTRUCTURE: a plain fp64 statement of what an attention descriptor (ctmi_attn_desc, include/ctmi355.h) means.

Written from the ABI's meaning and independent of tests/cpu_kernel_emulation.py: the operands are whatever the descriptor's strides
address inside the tensors the caller hands to ops.attn_fwd (``data_ptr`` = element (b=0, h=0, row=0, d=0)), the STORED values — already
rounded to the compute dtype — are upcast to fp64, and

    s[b,h,q,k] = scale * q.k + slope[h] * kpos[b,k] + add_mask[b,h,q,k]          kpos = (cumsum(mask) - 1) * mask
    causal future (k > q + (Sk - Sq)) on a non-padding key  ->  future_fill     (0 means finfo(float32).min)
    padding key (mask == 0)                                  ->  finfo(float32).min
    P = softmax over all Sk keys,  out = P v

Fully masked rows are part of the semantics: with the finfo.min fill they are uniform over all Sk keys, with GPT-2's -1e4 over the
non-padding future keys; their dS is exactly zero (the replaced entries do not depend on q or k).  Gradients come from autograd on the
fp64 leaves."""
from types import SimpleNamespace

import torch

FMIN = torch.finfo(torch.float32).min


def view4(t, B, nh, S, hd, bs, hs, rs):
    """[B,nh,S,hd] view of the elements the descriptor addresses, element (0,0,0,0) at t's first element"""
    return t.as_strided((B, nh, S, hd), (bs, hs, rs, 1), t.storage_offset())


def operand_views(desc, q, k, v, o):
    B, nh, Sq, Sk, hd = desc.B, desc.nh, desc.Sq, desc.Sk, desc.hd
    return (view4(q, B, nh, Sq, hd, desc.q_bs, desc.q_hs, desc.q_rs), view4(k, B, nh, Sk, hd, desc.k_bs, desc.k_hs, desc.k_rs),
            view4(v, B, nh, Sk, hd, desc.v_bs, desc.v_hs, desc.v_rs), None if o is None else view4(o, B, nh, Sq, hd, desc.o_bs, desc.o_hs, desc.o_rs))


def attn_reference(q, k, v, desc, slopes, attention_mask, add_mask, d_o=None):
    """q, k, v (and d_o, laid out like the output): CPU tensors as ops.attn_fwd takes them.  attention_mask: [B,Sk] of 0/1 or None;
    add_mask: the fp32 tensor whose strides are desc.am_*, or None.  Returns out [B,nh,Sq,hd], m and lse [B,nh,Sq] (row maximum and
    logsumexp of the final scores), tied [B,nh,Sq] (how many keys attain the maximum), replaced [B,1,Sq,Sk] (the entries whose score is a
    fill: their dS is exactly zero) and, when d_o is given, dq / dk / dv — all fp64."""
    B, nh, Sq, Sk = desc.B, desc.nh, desc.Sq, desc.Sk
    qv, kv, vv, gv = operand_views(desc, q, k, v, d_o)
    qf, kf, vf = (t.detach().double().clone().requires_grad_(True) for t in (qv, kv, vv))
    s = float(desc.scale) * torch.einsum("bhqd,bhkd->bhqk", qf, kf)
    pad = torch.zeros(B, 1, 1, Sk, dtype=torch.bool)
    if attention_mask is not None:
        am = attention_mask.to(torch.int64)
        assert am.shape == (B, Sk)
        pad = (am == 0).view(B, 1, 1, Sk)
        if slopes is not None:
            kpos = ((am.cumsum(-1) - 1) * am).double()
            s = s + slopes.detach().double().cpu().view(1, nh, 1, 1) * kpos.view(B, 1, 1, Sk)
    else:
        assert slopes is None, "ALiBi positions come from the attention mask"
    if add_mask is not None:
        s = s + add_mask.as_strided((B, nh, Sq, Sk), (desc.am_b, desc.am_h, desc.am_q, desc.am_k), add_mask.storage_offset()).double()
    fill = float(desc.future_fill) if float(desc.future_fill) != 0.0 else FMIN
    replaced = pad.expand(B, 1, Sq, Sk)
    if desc.causal:
        fut = torch.arange(Sk).view(1, Sk) > torch.arange(Sq).view(Sq, 1) + (Sk - Sq)
        s = torch.where(fut.view(1, 1, Sq, Sk) & ~pad, torch.full((), fill, dtype=torch.float64), s)
        replaced = replaced | fut.view(1, 1, Sq, Sk)
    s = torch.where(pad, torch.full((), FMIN, dtype=torch.float64), s)
    out = torch.einsum("bhqk,bhkd->bhqd", torch.softmax(s, dim=-1), vf)
    with torch.no_grad():
        m = s.max(dim=-1).values
        r = SimpleNamespace(out=out.detach(), m=m, lse=torch.logsumexp(s, dim=-1), tied=(s == m[..., None]).sum(-1), replaced=replaced, dq=None, dk=None, dv=None)
    if d_o is not None:
        out.backward(gv.detach().double())
        r.dq, r.dk, r.dv = qf.grad, kf.grad, vf.grad
    return r
