"""GPU: the general attention kernels (csrc/attention.hip: attn_fwd_kernel, attn_bwd_dq_kernel, attn_bwd_dkdv_kernel) against the fp64
reference of the descriptor's meaning (tests/attn_reference.py, proven on the CPU by tests/test_attn_reference_cpu.py) over the layouts
the models reach but no other test compares with a reference:

  A  head sizes off {8, 16, 32, 64, 128} (zero-padded fragments, guarded stores), hd == HDP behind an unaligned base / an odd row pitch
     (vec_ok == false), and the single-stage LDS path (fp32, hd > 64) over four key tiles;
  B  Sq != Sk: Q in the fused / blocked activation, K and V in a contiguous [B,nh,Sk,hd] cache, causal = Sq > 1, both models' spellings;
  C  non-causal with the additive masks transformer.AttentionLayer passes (four broadcast patterns; -1e4, -1e9, finfo.min and -inf);
  D  GPT-2's spelling (blocked layout, -1e4 future fill, either scale) at ragged S and small heads.

Every case calls ops.attn_fwd / ops.attn_bwd directly and compares out, dq, dk, dv, stat_m and stat_m + log(stat_l).  Output and
gradient buffers start as NaN, so a row that is never written shows, and the elements of a strided buffer that the descriptor does
not address must still be NaN afterwards.

Bounds: those of test_bloom_attention_fwd_bwd, which tests these same kernels — out: |err| <= atol + rtol |ref| with (rtol, atol) =
fp32 (2e-5, 2e-6), bf16 (2e-2, 1e-2), fp16 (4e-3, 2e-3); gradients: five times that element-wise plus check_norm (1e-2, 2e-2) bf16,
(2e-3, 4e-3) fp16, (5e-5, 2e-4, 1e-4) fp32; rows that are exact zeros in the reference (dK of padding keys, dQ of fully masked rows)
exactly zero; statistics: the rows with stat_m <= finfo.min are exactly the reference's fully masked rows and carry stat_l = number
of tied keys, elsewhere stat_m and stat_m + log(stat_l) within 1e-5 + 1e-5 |ref| of the fp64 maximum and logsumexp (five times the loss
kernels' LSE bound of test_cross_entropy_shifted: these scores are MFMA sums plus a bias).  check_norm's rows are one token's merged heads,
as in the source test: at one head's hd values an exact-arithmetic emulation with bf16 storage already exceeds the bf16 row bound (1.3x,
a query that sees two keys), so that granularity measures the format, not the kernel.  Q and K are scaled so that scale * q.k has unit
variance in every spelling, the size of the scores in the source test.

Measured on MI355X: 784 comparisons in 5.4 s; worst error / bound — fp32: out 0.83, dq 0.24, dk 0.23, dv 0.18, stat_m 0.06, lse 0.03;
bf16: out 0.29, dq 0.31 (row norm 0.53), dk 0.24 (0.39), dv 0.11 (0.20), stat_m 0.02; fp16: out 0.16, dq 0.08, dk 0.08, dv 0.10."""
import math
import time
from types import SimpleNamespace

import pytest
import torch

import attn_reference as AR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMIN = torch.finfo(torch.float32).min
NINF = float("-inf")
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
OUT_TOL = {F32: (2e-5, 2e-6), BF16: (2e-2, 1e-2), F16: (4e-3, 2e-3)}
NORM_TOL = {F32: (5e-5, 2e-4, 1e-4), BF16: (1e-2, 2e-2, 1e-2), F16: (2e-3, 4e-3, 1e-2)}
STAT_TOL = (1e-5, 1e-5)
DT3 = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16"), pytest.param(F16, id="fp16")]
DT2 = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16")]
WORST = {}                                  # (quantity, dtype) -> worst error / bound over the module's cases (printed at teardown)
T0 = [None, 0]


def ops():
    from cleantransformer_amd import ops as o
    return o


@pytest.fixture(scope="module", autouse=True)
def _report():
    T0[0] = time.time()
    yield
    print(f"\n[attn_general] {T0[1]} kernel comparisons in {time.time() - T0[0]:.1f} s; worst error / bound:")
    for (what, dt), v in sorted(WORST.items(), key=lambda kv: (str(kv[0][1]), kv[0][0])):
        print(f"[attn_general]   {str(dt).replace('torch.', ''):9s} {what:14s} {v:.3f}")


def _note(what, dtype, ratio):
    WORST[(what, dtype)] = max(WORST.get((what, dtype), 0.0), float(ratio))


def _check(what, dtype, got, ref, rtol, atol):
    """tests/test_gpu_ops.py::check"""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())}/{got.numel()} non-finite values"
    err, bound = (got - ref).abs(), atol + rtol * ref.abs()
    _note(what, dtype, (err / bound).max())
    bad = err > bound
    if bad.any():
        idx = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} off; worst err/bound {float((err / bound).max()):.3f}; "
                             f"first bad idx {idx} got {float(got[idx])} ref {float(ref[idx])}")


def _check_norm(what, dtype, got, ref, rel, row_rel, row_abs_frac):
    """tests/test_gpu_ops.py::check_norm"""
    got, ref = got.double(), ref.double()
    g2, r2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    glob = float((g2 - r2).norm() / (r2.norm() + 1e-300))
    rn, dn = r2.norm(dim=1), (g2 - r2).norm(dim=1)
    scale = float(rn.pow(2).mean().sqrt())
    row_bound = row_rel * rn + row_abs_frac * scale
    _note(what + " |.|", dtype, glob / rel)
    if float(row_bound.min()) > 0:
        _note(what + " row|.|", dtype, (dn / row_bound).max())
    assert glob <= rel, f"{what}: relative norm error {glob:.3e} > {rel:.1e}"
    worst = int((dn - row_bound).argmax())
    assert float(dn[worst]) <= float(row_bound[worst]), f"{what}: row {worst}: |got - ref| = {float(dn[worst]):.3e} > {float(row_bound[worst]):.3e}"


def _rnd(n, seed, dtype):
    """n standard normal values rounded to `dtype`, as fp32 (what the kernels will read)"""
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)).to(dtype).float()


# ------------------------------------------------------------------------------------------------ layouts
def _fused(B, S, nh, hd, base=0, pad=0):
    """Bloom's head-interleaved fused QKV [B,S,nh,3,hd] (`base` elements into its allocation, row pitch 3H + pad) and [B,S,H] context"""
    H, pitch = nh * hd, 3 * nh * hd + pad
    st = (S * pitch, 3 * hd, pitch)
    return SimpleNamespace(sizes={"qkv": base + B * S * pitch}, q=("qkv", base), k=("qkv", base + hd), v=("qkv", base + 2 * hd), q_str=st, k_str=st, v_str=st,
                           o_numel=B * S * H, o_str=(S * H, hd, H))


def _blocked(B, S, nh, hd):
    """GPT-2's [B,S,3H] = [q | k | v] and [B,S,H] context"""
    H = nh * hd
    st = (S * 3 * H, hd, 3 * H)
    return SimpleNamespace(sizes={"qkv": B * S * 3 * H}, q=("qkv", 0), k=("qkv", H), v=("qkv", 2 * H), q_str=st, k_str=st, v_str=st,
                           o_numel=B * S * H, o_str=(S * H, hd, H))


def _cached(B, Sq, Sk, nh, hd, blocked):
    """decode: Q inside the step's fused / blocked activation, K and V in contiguous [B,nh,Sk,hd] caches (modeling_bloom.py / modeling_gpt.py)"""
    H = nh * hd
    cs = (nh * Sk * hd, Sk * hd, hd)
    return SimpleNamespace(sizes={"qkv": B * Sq * 3 * H, "kc": B * nh * Sk * hd, "vc": B * nh * Sk * hd}, q=("qkv", 0), k=("kc", 0), v=("vc", 0),
                           q_str=(Sq * 3 * H, hd, 3 * H) if blocked else (Sq * 3 * H, 3 * hd, 3 * H), k_str=cs, v_str=cs, o_numel=B * Sq * H, o_str=(Sq * H, hd, H))


def _separate(B, S, nh, hd):
    """MHAFn: q, k, v and the context each a contiguous [B,S,H]"""
    H = nh * hd
    st = (S * H, hd, H)
    return SimpleNamespace(sizes={"q": B * S * H, "k": B * S * H, "v": B * S * H}, q=("q", 0), k=("k", 0), v=("v", 0), q_str=st, k_str=st, v_str=st,
                           o_numel=B * S * H, o_str=st)


# ------------------------------------------------------------------------------------------------ one comparison
def _run(dtype, L, B, nh, Sq, Sk, hd, scale, causal, *, slopes=None, am=None, add=None, fill=0.0, bwd=True, seed=0):
    """add: the fp32 CPU base tensor of the additive mask and a function that expands a tensor of that shape to [B,nh,Sq,Sk]"""
    o = ops()
    T0[1] += 1
    cpu = {n: _rnd(sz, seed + 17 * i, F32) for i, (n, sz) in enumerate(sorted(L.sizes.items()))}
    # standard normal operands, Q and K shrunk so that scale * q.k has unit variance in every spelling (GPT-2 without `scale` feeds its attention
    # small activations, not unit ones): the bounds come from test_bloom_attention_fwd_bwd, whose scores are of that size
    f = (scale * math.sqrt(hd)) ** -0.5
    for (n, off), S_, st in ((L.q, Sq, L.q_str), (L.k, Sk, L.k_str)):
        AR.view4(cpu[n][off:], B, nh, S_, hd, *st).mul_(f)
    cpu = {n: t.to(dtype).float() for n, t in cpu.items()}
    go = _rnd(L.o_numel, seed + 99, dtype)
    dev = {n: t.to(dtype).to(DEV) for n, t in cpu.items()}
    ins_c = [cpu[n][off:] for n, off in (L.q, L.k, L.v)]
    ins_d = [dev[n][off:] for n, off in (L.q, L.k, L.v)]
    add_c = add_d = None
    am_str = (0, 0, 0, 0)
    if add is not None:
        base, expand = add
        add_c, add_d = expand(base), expand(base.to(DEV))
        am_str = tuple(add_d.stride())
        assert am_str == tuple(add_c.stride())
        assert bool((add_c == 0).any(-1).all()), "every row keeps a key the mask leaves alone"
    desc = o._strided_desc(B, nh, Sq, Sk, hd, L.q_str, L.k_str, L.v_str, L.o_str, scale, causal, am_str, future_fill=fill)
    r = AR.attn_reference(*ins_c, desc, slopes, am, add_c, d_o=go if bwd else None)
    mask = o.MaskInfo(am.to(DEV)) if am is not None else None
    slopes_d = slopes.to(DEV) if slopes is not None else None
    out = torch.full((L.o_numel,), float("nan"), dtype=dtype, device=DEV)
    grads = {n: torch.full_like(t, float("nan")) for n, t in dev.items()}
    gr_d = [grads[n][off:] for n, off in (L.q, L.k, L.v)]
    could_w32 = dtype != F32 and hd in (64, 128) and causal and Sq == Sk and Sk % 64 == 0
    if could_w32:
        o.set_attn_path(0)                                                 # the general kernels, not the 128-row ones
    try:
        sm, sl = o.attn_fwd(*ins_d, out, desc, slopes_d, mask, add_d)
        if bwd:
            o.attn_bwd(*ins_d, out, go.to(dtype).to(DEV), sm, sl, *gr_d, desc, slopes_d, mask, add_d)
        torch.cuda.synchronize()
    except Exception as e:                                                 # a refused launch or a device error: start nothing else on that device
        pytest.exit(f"attention kernel call failed, ending the run: {e}", returncode=3)
    finally:
        if could_w32:
            o.set_attn_path(3)
    rt, at = OUT_TOL[dtype]
    out_c = out.float().cpu()
    _check("out", dtype, AR.view4(out_c, B, nh, Sq, hd, *L.o_str), r.out, rt, at)
    # statistics
    sm, sl = sm.double().cpu(), sl.double().cpu()
    full = r.m <= FMIN
    assert torch.equal(sm <= FMIN, full), f"fully masked rows: kernel {int((sm <= FMIN).sum())}, reference {int(full.sum())}"
    assert torch.equal(sl[full], r.tied[full].double()), "stat_l of a fully masked row is the number of tied keys"
    if bool((~full).any()):
        _check("stat_m", dtype, sm[~full], r.m[~full], *STAT_TOL)
        _check("stat lse", dtype, (sm + sl.log())[~full], r.lse[~full], *STAT_TOL)
    if not bwd:
        return r
    g_c = {n: t.float().cpu() for n, t in grads.items()}
    cover = {n: torch.zeros(t.numel(), dtype=torch.bool) for n, t in g_c.items()}
    cov_v = AR.operand_views(desc, *[cover[n][off:] for n, off in (L.q, L.k, L.v)], None)
    got_v = AR.operand_views(desc, *[g_c[n][off:] for n, off in (L.q, L.k, L.v)], None)
    for c in cov_v[:3]:
        c.fill_(True)
    for n in g_c:
        assert bool(torch.isnan(g_c[n][~cover[n]]).all()), f"gradient buffer {n}: an element outside the descriptor's operands was written"
    nrel, nrow, nabs = NORM_TOL[dtype]
    # rows whose every score is a fill (dQ: fully masked queries, the -1e4 quirk rows included; dK: padding keys) are exact zeros
    zero = {"dq": r.replaced.all(-1).expand(B, nh, Sq), "dk": r.replaced.all(-2).expand(B, nh, Sk)}
    assert bool((zero["dq"] | ~full).all())
    for what, got, ref in zip(("dq", "dk", "dv"), got_v, (r.dq, r.dk, r.dv)):
        _check(what, dtype, got, ref, 5 * rt, 5 * at)
        if float(ref.abs().max()) > 0:          # (Sq = Sk = 1: dS is identically zero, a relative norm has no meaning; the absolute bound above holds)
            # rows as the bounds' source test has them: one token's merged heads (there even its dq, dk and dv together), not one head's hd values
            _check_norm(what, dtype, got.transpose(1, 2).reshape(B, -1, nh * hd), ref.transpose(1, 2).reshape(B, -1, nh * hd), nrel, nrow, nabs)
        if what in zero:
            assert bool((ref[zero[what]] == 0).all())
            assert bool((got[zero[what]] == 0).all()), f"{what}: {int((got[zero[what]] != 0).any(-1).sum())} rows that are exact zeros in the reference are not"
    return r


def _slopes(nh):
    from cleantransformer_amd.models.modeling_bloom import alibi_slopes
    return alibi_slopes(nh).float().cpu()


def _mixed_mask(B, S):
    """tests/test_gpu_ops.py::_mask("mixed") for B = 2: right padding in row 1, left padding in row 0"""
    am = torch.ones(B, S, dtype=torch.long)
    am[1, (S * 3) // 4:] = 0
    am[0, :max(1, S // 3)] = 0
    return am


# ------------------------------------------------------------------------------------------------ A: head size and alignment
@pytest.mark.parametrize("dtype", DT3)
@pytest.mark.parametrize("hd", [20, 24, 40, 48, 80, 96, 120])
def test_head_sizes_between_the_compiled_ones(hd, dtype):
    """hd != HDP: zero-padded fragments (AT::load's slow arm, frag_global<.., false>) and store_own_row's guarded arm; 16-bit hd = 20 also has
    rows that are not 16-byte multiples (vec_ok == false).  Three key tiles, the last one ragged."""
    B, nh, S = 2, 3, 130
    _run(dtype, _fused(B, S, nh, hd), B, nh, S, S, hd, 1.0 / math.sqrt(hd), True, slopes=_slopes(nh), am=_mixed_mask(B, S), seed=hd)


@pytest.mark.parametrize("dtype", DT3)
@pytest.mark.parametrize("how", ["base+1", "pitch+1"])
@pytest.mark.parametrize("hd", [32, 64])
def test_compiled_head_sizes_behind_unaligned_rows(hd, how, dtype):
    """hd == HDP with vec_ok == false: the (N,N,N) variant with fast == false"""
    B, nh, S = 2, 3, 130
    L = _fused(B, S, nh, hd, base=1) if how == "base+1" else _fused(B, S, nh, hd, pad=1)
    _run(dtype, L, B, nh, S, S, hd, 1.0 / math.sqrt(hd), True, slopes=_slopes(nh), am=_mixed_mask(B, S), seed=hd + 1)


@pytest.mark.parametrize("hd", [96, 128])
def test_single_stage_lds_path_over_four_key_tiles(hd):
    """fp32, 64 < hd <= 128: nbuf_for(...) == 1, the two-barrier loop — forward, dQ and dK/dV"""
    B, nh, S = 2, 3, 200
    _run(F32, _fused(B, S, nh, hd), B, nh, S, S, hd, 1.0 / math.sqrt(hd), True, slopes=_slopes(nh), am=_mixed_mask(B, S), seed=hd + 2)


# ------------------------------------------------------------------------------------------------ B: Sq != Sk
SQSK = [(1, 1), (1, 64), (1, 65), (1, 200), (3, 64), (5, 70), (64, 128), (70, 200)]


def _cache_mask(kind, B, Sq, Sk):
    """[B,Sk] key masks of a decode step; every batch row keeps its last key (the token being decoded)"""
    am = torch.ones(B, Sk, dtype=torch.long)
    off = Sk - Sq
    if kind == "right":                                                    # right padding in row 1 (never the whole row)
        am[1, max(1, (Sk * 3) // 4):] = 0
    elif kind == "left_short":                                             # row 0: shorter than Sk - Sq, every query still sees a real key
        am[0, :off // 2] = 0
    elif kind == "left_long":                                              # row 0: longer than Sk - Sq, the leading queries' whole window is padding
        am[0, :min(Sk - 1, off + (Sq + 1) // 2)] = 0
    return am


@pytest.mark.parametrize("dtype", DT3)
@pytest.mark.parametrize("kind", ["ones", "right", "left_short", "left_long"])
@pytest.mark.parametrize("spelling", ["bloom", "gpt"])
@pytest.mark.parametrize("hd", [16, 64])
@pytest.mark.parametrize("Sq,Sk", SQSK)
def test_kv_cache_geometry(Sq, Sk, hd, spelling, kind, dtype):
    """p.off = Sk - Sq in every place the three kernels use it, K / V rows of pitch hd beside a Q of pitch 3H; backward in fp32 and bf16"""
    B, nh = 2, 2
    am = _cache_mask(kind, B, Sq, Sk)
    kw = dict(slopes=_slopes(nh), fill=0.0, scale=1.0 / math.sqrt(hd)) if spelling == "bloom" else dict(slopes=None, fill=-1e4, scale=1.0)
    scale = kw.pop("scale")
    r = _run(dtype, _cached(B, Sq, Sk, nh, hd, blocked=spelling == "gpt"), B, nh, Sq, Sk, hd, scale, Sq > 1, am=am, bwd=dtype != F16,
             seed=Sq * 1000 + Sk + hd, **kw)
    if kind == "left_long" and Sq > 1:                                     # the case is what it says: some, not all, queries of row 0 see only padding
        quirk = (r.m[0, 0] <= FMIN) if spelling == "bloom" else (r.m[0, 0] == -1e4)
        assert 0 < int(quirk.sum()) < Sq


# ------------------------------------------------------------------------------------------------ C: non-causal, additive masks
MASK_SHAPES = {"b11s": lambda B, nh, S: (B, 1, 1, S), "11ss": lambda B, nh, S: (1, 1, S, S), "ss": lambda B, nh, S: (S, S),
               "bhss": lambda B, nh, S: (B, nh, S, S)}


def _expander(B, nh, S):
    """what MHAFn.forward does with the user's mask"""
    def f(am):
        am = am.to(torch.float32)
        return am.expand(B, nh, S, S) if am.dim() == 4 else am.reshape((1,) * (4 - am.dim()) + tuple(am.shape)).expand(B, nh, S, S)
    return f


def _random_mask(shape, value, seed):
    hit = torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < 0.4
    m = torch.where(hit, torch.tensor(value), torch.tensor(0.0))
    m[..., shape[-1] // 2] = 0.0                                            # every row keeps one untouched key
    return m


@pytest.mark.parametrize("dtype", DT3)
@pytest.mark.parametrize("S", [7, 64, 65, 150])
@pytest.mark.parametrize("hd", [16, 64])
def test_non_causal_without_a_mask(hd, S, dtype):
    B, nh = 2, 2
    _run(dtype, _separate(B, S, nh, hd), B, nh, S, S, hd, 1.0 / math.sqrt(hd), False, seed=S + hd)


@pytest.mark.parametrize("dtype", DT3)
@pytest.mark.parametrize("value", [-1e4, -1e9, FMIN], ids=["-1e4", "-1e9", "fmin"])
@pytest.mark.parametrize("shape", list(MASK_SHAPES))
@pytest.mark.parametrize("S", [7, 64, 65, 150])
@pytest.mark.parametrize("hd", [16, 64])
def test_additive_mask_broadcast_patterns(hd, S, shape, value, dtype):
    """the AM variants without dropout, with the strides `expand` gives each of the shapes a user may pass to AttentionLayer"""
    B, nh = 2, 2
    base = _random_mask(MASK_SHAPES[shape](B, nh, S), value, seed=S * 7 + hd)
    _run(dtype, _separate(B, S, nh, hd), B, nh, S, S, hd, 1.0 / math.sqrt(hd), False, add=(base, _expander(B, nh, S)), seed=S + hd + 3)


def _inf_mask(pattern, shape_kind, B, nh, S):
    if pattern == "pad_last_70":                                            # the last key tile is wholly -inf
        m = torch.zeros(B, 1, 1, S)
        m[..., S - 70:] = NINF
    elif pattern == "lead_70":                                              # the leading key tile is wholly -inf, for every row
        m = torch.zeros(1, 1, S, S)
        m[..., :70] = NINF
    else:                                                                   # band: query q sees keys [q - 20, q + 5]
        q, k = torch.arange(S).view(S, 1), torch.arange(S).view(1, S)
        m = torch.where((k >= q - 20) & (k <= q + 5), torch.tensor(0.0), torch.tensor(NINF))
    return m.expand(B, nh, S, S).contiguous() if shape_kind == "bhss" else m


@pytest.mark.parametrize("dtype", DT3)
@pytest.mark.parametrize("shape_kind", ["natural", "bhss"])
@pytest.mark.parametrize("pattern", ["pad_last_70", "lead_70", "band"])
@pytest.mark.parametrize("hd", [16, 64])
def test_additive_mask_with_minus_infinity(hd, pattern, shape_kind, dtype):
    """-inf entries are legal inputs of the reference's `weight + attention_mask; softmax` (transformer.py:43-45).  A row whose mask is -inf on a
    whole leading key tile has no finite running maximum after that tile: the forward must not form -inf - -inf."""
    B, nh, S = 2, 2, 150
    base = _inf_mask(pattern, shape_kind, B, nh, S)
    _run(dtype, _separate(B, S, nh, hd), B, nh, S, S, hd, 1.0 / math.sqrt(hd), False, add=(base, _expander(B, nh, S)), seed=hd + 5)


def test_attention_layer_with_a_band_mask_against_torch_softmax():
    """transformer.AttentionLayer / MHAFn under autograd, against torch's own softmax path in fp64"""
    from cleantransformer_amd.transformer import AttentionLayer
    B, S, H, nh = 2, 150, 64, 2
    cfg = SimpleNamespace(hidden_size=H, num_attention_heads=nh, attention_probs_dropout_prob=0.0)
    torch.manual_seed(3)
    layer = AttentionLayer(cfg).to(DEV)
    x = torch.randn(B, S, H, generator=torch.Generator().manual_seed(4))
    go = torch.randn(B, S, H, generator=torch.Generator().manual_seed(5))
    band = _inf_mask("band", "natural", B, nh, S)
    assert bool((band == 0).any(-1).all())
    xd = x.to(DEV).requires_grad_(True)
    y = layer(xd, attention_mask=band.to(DEV))
    y.backward(go.to(DEV))
    T0[1] += 1
    xr = x.detach().double().requires_grad_(True)
    pr = {n: p.detach().double().cpu().requires_grad_(True) for n, p in layer.named_parameters()}
    q, k, v = ((xr @ pr[f"{n}_linear.weight"].t() + pr[f"{n}_linear.bias"]).view(B, S, nh, H // nh).transpose(1, 2) for n in "qkv")
    w = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(H // nh) + band.double(), dim=-1)
    yr = (w @ v).transpose(1, 2).reshape(B, S, H)
    yr.backward(go.double())
    rt, at = OUT_TOL[F32]
    _check("layer y", F32, y.detach().cpu(), yr.detach(), rt, at)
    _check("layer dx", F32, xd.grad.cpu(), xr.grad, 5 * rt, 5 * at)
    _check_norm("layer dx", F32, xd.grad.cpu(), xr.grad, *NORM_TOL[F32])
    for n, p in layer.named_parameters():
        if n == "k_linear.bias":       # zero in exact arithmetic (a constant added to every key's score of a row): rounding level of its Q twin
            assert float(p.grad.abs().max()) <= 1e-4 * float(pr["q_linear.bias"].grad.abs().max())
            continue
        _check_norm("layer dparam", F32, p.grad.cpu().reshape(-1, p.shape[-1]), pr[n].grad.reshape(-1, p.shape[-1]), *NORM_TOL[F32])


# ------------------------------------------------------------------------------------------------ D: GPT-2's spelling off the 128-row shapes
@pytest.mark.parametrize("dtype", DT2)
@pytest.mark.parametrize("scaled", [False, True], ids=["scale1", "rsqrt"])
@pytest.mark.parametrize("hd", [16, 48])
@pytest.mark.parametrize("S", [70, 130])
def test_gpt_spelling_at_ragged_lengths(S, hd, scaled, dtype):
    """blocked layout, no ALiBi, -1e4 on the causal future; row 0 is left-padded (its leading queries see only padding and attend uniformly
    to the non-padding future), row 1 right-padded"""
    B, nh = 2, 2
    am = torch.ones(B, S, dtype=torch.long)
    am[0, :9] = 0
    am[1, S - 11:] = 0
    r = _run(dtype, _blocked(B, S, nh, hd), B, nh, S, S, hd, 1.0 / math.sqrt(hd) if scaled else 1.0, True, am=am, fill=-1e4, seed=S + hd + 7)
    assert bool((r.m[0, :, :9] == -1e4).all()) and bool((r.tied[0, :, 0] == S - 9).all())
