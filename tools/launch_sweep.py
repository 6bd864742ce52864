"""One call per selector arm of the host launch code of layernorm / loss / optim / elementwise, attention, attention_w32 and lora, on fixed
seeded inputs; one line per call: entry, case, return code, sha256 of every output buffer.

Two listings are comparable line for line: the library comes from CTMI_LIB_PATH when set (cleantransformer_amd/_lib.py), so the same script
runs against another build of the sources.  Under a kernel trace the ordered (kernel, grid, workgroup, dynamic LDS) list is comparable too —
that is what shows a changed grid which a grid-stride kernel would hide from the hashes.  One process, a few seconds, everything tiny.

    python tools/launch_sweep.py > sweep.txt
"""
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from cleantransformer_amd import _lib  # noqa: E402
from cleantransformer_amd._lib import BF16, F16, F32, OPT_LEGACY_GRID, OPT_SHADOW_F16, AttnDesc  # noqa: E402

TD = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
DN = {F32: "f32", BF16: "bf16", F16: "f16"}
DEV = "cuda"
lib = _lib.load()


def rnd(seed, *shape, dtype=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def sha(t):
    return hashlib.sha256(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


def emit(entry, case, rc, *outs):
    torch.cuda.synchronize()
    print(entry, case, f"rc={rc}", *[sha(o) for o in outs], flush=True)


def ptrs(ts):
    return C.cast((C.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), C.POINTER(C.c_void_p))


# ---------------------------------------------------------------- LayerNorm, column sums
def layernorm():
    cols_of = {F32: (99, 132, 256, 388, 512, 1024, 2048, 2052), BF16: (100, 264, 512, 776, 1024, 2048, 4096, 4104)}
    cols_of[F16] = cols_of[BF16]
    for dt in (F32, BF16, F16):
        for rows in (5, 37):
            for cols in cols_of[dt]:
                case = f"{DN[dt]} rows={rows} cols={cols}"
                x, w, b = rnd(1, rows, cols, dtype=TD[dt]), rnd(2, cols) + 1.0, rnd(3, cols)
                y, mean, rstd = zeros(rows, cols, dtype=TD[dt]), zeros(rows), zeros(rows)
                rc = lib.ctmi_layernorm_fwd(p(x), p(w), p(b), p(y), p(mean), p(rstd), rows, cols, 1e-5, dt, None)
                emit("layernorm_fwd", case, rc, y, mean, rstd)
                dy, dres = rnd(4, rows, cols, dtype=TD[dt]), rnd(5, rows, cols, dtype=TD[dt])
                ws = zeros(lib.ctmi_layernorm_bwd_ws(rows, cols))
                for res in (None, dres):
                    dx, dw, db = zeros(rows, cols, dtype=TD[dt]), zeros(cols), zeros(cols)
                    rc = lib.ctmi_layernorm_bwd(p(dy), p(x), p(w), p(mean), p(rstd), p(res), p(dx), p(dw), p(db), 0, p(ws), rows, cols, dt, None)
                    emit("layernorm_bwd", case + f" dres={int(res is not None)}", rc, dx, dw, db)


def colsum():
    M = 50
    for dt in (F32, BF16, F16):
        for N in (72, 70):
            for ld in (N, N + 8):
                x, out, ws = rnd(6, M, ld, dtype=TD[dt]), zeros(N), zeros(lib.ctmi_colsum_ws(M, N))
                rc = lib.ctmi_colsum(p(x), ld, p(out), 0, p(ws), M, N, dt, None)
                emit("colsum", f"{DN[dt]} M={M} N={N} ld={ld}", rc, out)


# ---------------------------------------------------------------- dropout, embedding
def dropout():
    for dt in (F32, BF16, F16):
        for n in (1003, 1024):
            x, r = rnd(7, n, dtype=TD[dt]), rnd(8, n, dtype=TD[dt])
            for res in (None, r):
                y = zeros(n, dtype=TD[dt])
                rc = lib.ctmi_dropout(p(x), p(res), p(y), n, 0.25, 1234, dt, None)
                emit("dropout", f"{DN[dt]} n={n} res={int(res is not None)}", rc, y)


def embedding():
    V, ids = 11, torch.tensor([0, 3, 10, 11, 5, 3, 7], dtype=torch.int64, device=DEV)       # 11 is out of range
    n = ids.numel()
    for dt in (F32, BF16, F16):
        for H in (72, 70):
            table, out, flag = rnd(9, V, H, dtype=TD[dt]), zeros(n, H, dtype=TD[dt]), zeros(1, dtype=torch.int32)
            rc = lib.ctmi_embed_fwd(p(table), p(ids), p(out), n, H, V, dt, p(flag), None)
            emit("embed_fwd", f"{DN[dt]} H={H}", rc, out, flag)
            dout, dtable = rnd(10, n, H, dtype=TD[dt]), zeros(V, H)
            rc = lib.ctmi_embed_bwd(p(dout), p(ids), p(dtable), n, H, V, dt, 0.5, None)
            emit("embed_bwd", f"{DN[dt]} H={H}", rc, dtable)                                 # (id 3 twice: two atomic adds onto 0, either order the same sum)


# ---------------------------------------------------------------- cross entropy
def cross_entropy():
    N, seq, shift, ign = 6, 3, 1, -100
    for dt in (F32, BF16, F16):
        vec = 4 if dt == F32 else 8
        for Cc, ld in ((1000, 1000), (1003, 1008), (1003, 1003)):
            case = f"{DN[dt]} C={Cc} ld={ld}"
            g = torch.Generator().manual_seed(11)
            labels = torch.randint(0, Cc, (N,), generator=g)
            labels[4] = ign
            labels = labels.to(DEV)
            logits = rnd(12, N, ld, dtype=TD[dt], scale=3.0)
            lse, rl, lo = zeros(N), zeros(N), zeros(2)
            rc = lib.ctmi_ce_fwd(p(logits), ld, p(labels), p(lse), p(rl), p(lo), N, Cc, seq, shift, ign, 0, 0, dt, None)
            emit("ce_fwd", case, rc, lse, rl, lo)
            dl = zeros(N, ld, dtype=TD[dt])
            rc = lib.ctmi_ce_bwd(p(logits), ld, p(labels), p(lse), p(lo), None, p(dl), ld, N, Cc, seq, shift, ign, dt, None)
            emit("ce_bwd", case, rc, dl)
            if ld % vec == 0:                                                               # the fused form wants 16-byte rows
                lse, rl, lo, dl = zeros(N), zeros(N), zeros(2), zeros(N, ld, dtype=TD[dt])
                rc = lib.ctmi_ce_fwd_bwd(p(logits), ld, p(labels), p(lse), p(rl), p(lo), p(dl), ld, N, Cc, seq, shift, ign, 0, 0, 1.0, None, dt, None)
                emit("ce_fwd_bwd", case, rc, lse, rl, lo, dl)
        for Cc in (1000, 1003):
            logits, target = rnd(13, N, Cc, dtype=TD[dt], scale=3.0), torch.softmax(rnd(14, N, Cc), -1)
            lse, ts, rl, lo = zeros(N), zeros(N), zeros(N), zeros(2)
            rc = lib.ctmi_ce_soft_fwd(p(logits), Cc, p(target), Cc, p(lse), p(ts), p(rl), p(lo), N, Cc, 1, N, dt, None)
            emit("ce_soft_fwd", f"{DN[dt]} C={Cc}", rc, lse, ts, rl, lo)
            dl = zeros(N, Cc, dtype=TD[dt])
            rc = lib.ctmi_ce_soft_bwd(p(logits), Cc, p(target), Cc, p(lse), p(ts), p(lo), None, p(dl), Cc, N, Cc, dt, None)
            emit("ce_soft_bwd", f"{DN[dt]} C={Cc}", rc, dl)
        x, s = rnd(15, N, 1000, dtype=TD[dt]), torch.tensor([0.5], device=DEV)
        rc = lib.ctmi_scale_if(p(x), 1000, N, 1000, p(s), 1.0, None, dt, None)
        emit("scale_if", DN[dt], rc, x)


# ---------------------------------------------------------------- optimizers, GradScaler
def _tensors(seed, scale=1.0):
    """70 tensors of sizes {1, 7, 4096, 16384, 16391}; tensor 3 starts one element into its buffer (not 16-byte aligned)"""
    sizes = [(1, 7, 4096, 16384, 16391)[i % 5] for i in range(70)]
    out = []
    for i, n in enumerate(sizes):
        t = rnd(seed * 1000 + i, n + 1, scale=scale)
        out.append(t[1:] if i == 3 else t[:n])
    return out, (C.c_int64 * len(sizes))(*sizes)


def optimizers():
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.01)
    for form in ("flat", "dev", "legacy"):
        for decoupled in (0, 1):
            for sh_dt in (BF16, F16):
                P, n = _tensors(1)
                G, M, V = _tensors(2, 0.1)[0], _tensors(3, 0.01)[0], [t.abs() for t in _tensors(4, 0.001)[0]]
                S = [zeros(t.numel() + 4, dtype=TD[sh_dt])[:t.numel()] for t in P]
                flags = 1 | (OPT_SHADOW_F16 if sh_dt == F16 else 0) | (OPT_LEGACY_GRID if form == "legacy" else 0)
                if form == "dev":
                    hd = zeros(64)
                    rc = lib.ctmi_adamw_set_hyper(p(hd), *hyper, 3, decoupled, flags, 0.5, None)
                    rc = rc or lib.ctmi_adamw_step_dev(ptrs(P), ptrs(G), ptrs(M), ptrs(V), ptrs(S), n, len(P), p(hd), None)
                else:
                    rc = lib.ctmi_adamw_step(ptrs(P), ptrs(G), ptrs(M), ptrs(V), ptrs(S), n, len(P), *hyper, 3, decoupled, flags, 0.5, None)
                emit("adamw_step", f"{form} decoupled={decoupled} shadow={DN[sh_dt]}", rc, *[torch.cat(L) for L in (P, G, M, V, S)])
    for momentum in (0, 1):
        P, n = _tensors(5)
        G, B = _tensors(6, 0.1)[0], _tensors(7, 0.1)[0]
        S = [zeros(t.numel(), dtype=torch.bfloat16) for t in P]
        rc = lib.ctmi_sgd_step(ptrs(P), ptrs(G), ptrs(B) if momentum else None, ptrs(S), n, len(P), 1e-2, 0.9, 0.1, 0.01, 0, None)
        emit("sgd_step", f"momentum={momentum}", rc, *[torch.cat(L) for L in (P, G, B, S)])
    G, n = _tensors(8)
    G[7][5] = float("inf")
    state = torch.tensor([1024.0, 3.0, 0.0], device=DEV)
    rc = lib.ctmi_amp_unscale(ptrs(G), n, len(G), p(state), None)
    emit("amp_unscale", "one-inf", rc, torch.cat(G), state)
    rc = lib.ctmi_amp_update(p(state), 2.0, 0.5, 4, None)
    emit("amp_update", "after-inf", rc, state)
    rc = lib.ctmi_amp_update(p(state), 2.0, 0.5, 1, None)
    emit("amp_update", "growth", rc, state)


# ---------------------------------------------------------------- casts and friends
def casts():
    for sd, dd in ((F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16), (F32, F16), (F16, F32), (F16, F16)):
        for n in (1003, 1024):
            src, dst = rnd(16, n, dtype=TD[sd]), zeros(n, dtype=TD[dd])
            rc = lib.ctmi_cast(p(src), sd, p(dst), dd, n, None)
            emit("cast", f"{DN[sd]}->{DN[dd]} n={n}", rc, dst)
    src = rnd(17, 70, 130)
    for dd in (F32, BF16, F16):
        dst = zeros(130, 70, dtype=TD[dd])
        rc = lib.ctmi_transpose_cast(p(src), p(dst), dd, 70, 130, None)
        emit("transpose_cast", DN[dd], rc, dst)
    x, acc = rnd(18, 1003), zeros(1, dtype=torch.float64)
    # (one atomic add per workgroup, one workgroup at this size: the sum has one order)
    for accumulate in (0, 1):
        rc = lib.ctmi_sumsq(p(x), 1003, p(acc), accumulate, None)
        emit("sumsq", f"accumulate={accumulate}", rc, acc)
    s = torch.tensor([0.25], device=DEV)
    for sd_ in (None, s):
        y = x.clone()
        rc = lib.ctmi_scale(p(y), 1003, 3.0, p(sd_), None)
        emit("scale", f"s_dev={int(sd_ is not None)}", rc, y)
    y = zeros(1003)
    rc = lib.ctmi_scale_copy(p(x), p(y), 1003, 3.0, None)
    emit("scale_copy", "n=1003", rc, y)


# ---------------------------------------------------------------- decode helpers
def decode():
    rows, cols = 3, 1003
    for dt in (F32, BF16, F16):
        x = rnd(19, rows, cols, dtype=TD[dt], scale=2.0)
        idx = zeros(rows, dtype=torch.int64)
        rc = lib.ctmi_argmax(p(x), cols, p(idx), rows, cols, dt, None)
        emit("argmax", DN[dt], rc, idx)
        stats = zeros(rows, 2)
        rc = lib.ctmi_row_lse(p(x), cols, p(stats), rows, cols, dt, None)
        emit("row_lse", DN[dt], rc, stats)
        add, ov, oi = rnd(20, rows), zeros(4), zeros(4, dtype=torch.int64)
        rc = lib.ctmi_group_topk(p(x), cols, p(stats), p(add), 0.5, p(ov), p(oi), 1, rows, cols, 4, dt, None)
        emit("group_topk", DN[dt], rc, ov, oi)
    x, thr, out = rnd(21, rows, cols), torch.tensor([0.1, -0.2, 0.3], device=DEV), zeros(rows, cols)
    rc = lib.ctmi_scores_filter(p(x), cols, 0.7, p(thr), 1, -1e9, p(out), cols, rows, cols, None)
    emit("scores_filter", "thr", rc, out)
    am = torch.tensor([[0, 0, 0, 1, 1, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1, 1, 1, 1]], dtype=torch.int64, device=DEV)       # left padding
    kpos, kvalid, first = zeros(2, 9), zeros(2, 9, dtype=torch.int32), zeros(2, dtype=torch.int32)
    rc = lib.ctmi_mask_prep(p(am), p(kpos), p(kvalid), p(first), 2, 9, None)
    emit("mask_prep", "B=2 S=9", rc, kpos, kvalid, first)


# ---------------------------------------------------------------- attention
def _attn(case, dt, B, nh, Sq, Sk, hd, mask=False, drop=0.0, future_fill=0.0):
    q, k, v = (rnd(22 + i, B, nh, S, hd, dtype=TD[dt], scale=0.5) for i, S in enumerate((Sq, Sk, Sk)))
    d = AttnDesc()
    d.B, d.nh, d.Sq, d.Sk, d.hd = B, nh, Sq, Sk, hd
    d.q_bs, d.q_hs, d.q_rs = nh * Sq * hd, Sq * hd, hd
    d.o_bs, d.o_hs, d.o_rs = nh * Sq * hd, Sq * hd, hd
    d.k_bs, d.k_hs, d.k_rs = nh * Sk * hd, Sk * hd, hd
    d.v_bs, d.v_hs, d.v_rs = nh * Sk * hd, Sk * hd, hd
    d.scale, d.causal, d.future_fill, d.dropout_p, d.dropout_seed = hd ** -0.5, 1, future_fill, drop, 77
    am = None
    if mask:
        am = rnd(25, B, nh, Sq, Sk, scale=0.3)
        d.am_b, d.am_h, d.am_q, d.am_k = nh * Sq * Sk, Sq * Sk, Sk, 1
    o, sm, sl = zeros(B, nh, Sq, hd, dtype=TD[dt]), zeros(B, nh, Sq), zeros(B, nh, Sq)
    rc = lib.ctmi_attn_fwd(p(q), p(k), p(v), p(o), p(sm), p(sl), None, None, None, None, p(am), C.byref(d), dt, None)
    emit("attn_fwd", case, rc, o, sm, sl)
    do = rnd(26, B, nh, Sq, hd, dtype=TD[dt])
    dq, dk, dv, delta = zeros(B, nh, Sq, hd, dtype=TD[dt]), zeros(B, nh, Sk, hd, dtype=TD[dt]), zeros(B, nh, Sk, hd, dtype=TD[dt]), zeros(B, nh, Sq)
    rc = lib.ctmi_attn_bwd(p(q), p(k), p(v), p(o), p(do), p(sm), p(sl), p(dq), p(dk), p(dv), p(delta), None, None, None, None, p(am), C.byref(d), dt, None)
    emit("attn_bwd", case, rc, dq, dk, dv, delta)


def attention():
    prev = lib.ctmi_attn_set_path(0)                                                         # the general kernels
    arms = (("fast", 64, {}), ("generic", 40, {}), ("mask", 64, {"mask": True}), ("drop", 64, {"drop": 0.1}),
            ("drop+mask", 64, {"drop": 0.1, "mask": True}))
    for dt in (BF16, F32, F16):
        for name, hd, kw in arms + ((("fast", 32, {}), ("fast", 128, {})) if dt == BF16 else ()):
            _attn(f"general {DN[dt]} {name} hd={hd} S=80", dt, 1, 2, 80, 80, hd, **kw)
        _attn(f"general {DN[dt]} decode hd=64 Sq=1 Sk=80", dt, 1, 2, 1, 80, 64)
    lib.ctmi_attn_set_path(3)                                                                # the 128-row kernels
    for dt in (BF16, F16):
        for hd in (64, 128):
            for ff in (0.0, -1e4):
                _attn(f"rows128 {DN[dt]} hd={hd} future_fill={ff}", dt, 1, 2, 128, 128, hd, future_fill=ff)
    lib.ctmi_attn_set_path(prev)


# ---------------------------------------------------------------- adapters
def adapters():
    T = 40
    for dt in (BF16, F16):
        for km in (0, 1):
            K = 64
            for r in (8, 24, 40, 64):
                x, w, out = rnd(27, T, K, dtype=TD[dt]), rnd(28, *((K, r) if km else (r, K)), dtype=TD[dt]), zeros(T, r, dtype=TD[dt])
                rc = lib.ctmi_lora_project(p(x), K, p(w), r if km else K, km, p(out), r, T, K, r, 0.5, dt, None)
                emit("lora_project", f"{DN[dt]} kmajor={km} r={r}", rc, out)
            N = 264
            for r in (8, 64):
                xa, w, y = rnd(29, T, r, dtype=TD[dt]), rnd(30, *((r, N) if km else (N, r)), dtype=TD[dt]), rnd(31, T, N, dtype=TD[dt])
                rc = lib.ctmi_lora_expand_add(p(xa), r, p(w), N if km else r, km, p(y), N, T, N, r, dt, None)
                emit("lora_expand_add", f"{DN[dt]} kmajor={km} r={r}", rc, y)
        Pd, Q = 64, 264
        l, r_, out = rnd(32, T, Pd, dtype=TD[dt]), rnd(33, T, Q, dtype=TD[dt]), zeros(Pd, Q)
        nws = lib.ctmi_lora_wgrad_ws(T, Pd, Q)
        ws = zeros(nws)
        rc = lib.ctmi_lora_wgrad(p(l), Pd, p(r_), Q, p(out), Q, T, Pd, Q, 0.5, p(ws), nws * 4, dt, None)
        emit("lora_wgrad", DN[dt], rc, out)


if __name__ == "__main__":
    for part in (layernorm, colsum, dropout, embedding, cross_entropy, optimizers, casts, decode, attention, adapters):
        part()
