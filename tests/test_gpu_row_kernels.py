"""GPU (-m gpu): the row kernels past the first pass of their stride loops, and at the edges no operator-level test reached.

LayerNorm, the loss, the embedding and the small utility kernels run on a capped grid with a stride loop behind it.  The shapes here are
the smallest that make a wave (or a workgroup) take a second trip, reach a clamped / invalid second half of a two-row trip, or take the
other kernel of a pair (vector | generic, FULL | guarded, one-pass | two-pass); the training step (8192 rows) lives on those trips.

References are plain torch in fp64 on the CPU, computed from the values the kernel saw (inputs rounded to the storage dtype first).
Tolerances are those of tests/test_gpu_ops.py and tests/test_gpu_block.py for the same operator unless a comment derives another one.
Set CTMI_TEST_VERBOSE=1 to print every measured worst error next to its bound."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_ops import DEV, DT, check, lo, ops, rel_err, rnd, to_dev  # noqa: E402

F = torch.nn.functional
NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
VERBOSE = bool(os.environ.get("CTMI_TEST_VERBOSE"))


def say(*a):
    if VERBOSE:
        print("[row_kernels]", *a, flush=True)


def worst(name, got, ref, rtol, atol):
    """check() with the measured figure reported first: max over elements of |got - ref| / (atol + rtol * |ref|)  (<= 1 passes)."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    say(f"{name}: max |err| {float((g - r).abs().max()):.3e}; worst err/bound {float(((g - r).abs() / (atol + rtol * r.abs())).max()):.3f}")
    check(name, got, ref, rtol, atol)


# ------------------------------------------------------------------------------------------------ 1. LayerNorm backward past one pass
# ln_bwd_vec launches min(ceil(rows / 8), 256) workgroups of 8 waves = at most 2048 waves, two rows (A, B) per wave and trip:
#   rows = 2600: every wave makes one trip; the second half is valid for waves < 552 and the clamped last row for the others
#   rows = 4700: waves < 604 make a second trip (they consume the A set prefetched during the first), with a clamped second half
# widths: guarded (cols < MAXV * 64 * VEC), FULL for MAXV = 1 and 2 (cols == MAXV * 64 * VEC), and MAXV = 2 guarded
LN_WIDTHS = {torch.float32: (64, 256, 512, 260), torch.bfloat16: (64, 512, 1024, 520), torch.float16: (64, 512, 1024, 520)}
LN_CASES = [pytest.param(dt, rt, at, c, id=f"{NAMES[dt]}-{c}") for dt, rt, at in DT for c in LN_WIDTHS[dt]]


def _ln_ref(xs, w, b, gys, eps=1e-5):
    """fp64 LayerNorm forward / backward on the values the kernel saw -> y, mean, rstd, dx, dw, db"""
    xr = xs.double().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.layer_norm(xr, (xs.shape[1],), wr, br, eps)
    y.backward(gys.double())
    mean = xs.double().mean(-1)
    rstd = 1.0 / torch.sqrt(xs.double().var(-1, unbiased=False) + eps)
    return y.detach(), mean, rstd, xr.grad, wr.grad, br.grad


def _ln_fwd_bwd_vs_fp64(x, dy, dres, w, b, dtype, rtol, atol, tag, misalign=False):
    """forward + backward (with and without dres) against fp64, with test_layernorm_fwd_bwd's tolerances; x / dy / dres are fp32 CPU tensors"""
    o = ops()
    rows, cols = x.shape
    rd = lo(dtype)
    xs, gys, drs = rd(x), rd(dy), rd(dres)
    y_ref, mean_ref, rstd_ref, dx_ref, dw_ref, db_ref = _ln_ref(xs, w, b, gys)

    def dev(t):
        if not misalign:
            return to_dev(t, dtype)
        base = torch.zeros(rows * cols + 8, dtype=dtype, device=DEV)             # a view one element past a 16-byte boundary: generic kernels
        v = base[1:1 + rows * cols].view(rows, cols)
        v.copy_(t.to(dtype))
        assert v.data_ptr() % 16 != 0
        return v
    xd, gd, rdv = dev(x), dev(dy), dev(dres)
    y, mean, rstd = o.layernorm_fwd(xd, w.to(DEV), b.to(DEV), 1e-5)
    worst(f"{tag} y", y.float(), y_ref, rtol, atol)
    worst(f"{tag} mean", mean, mean_ref, 1e-5, 1e-6)
    worst(f"{tag} rstd", rstd, rstd_ref, 1e-5, 0.0)                              # fp32 statistics in every dtype (derivation: section 2)
    dx, dw, db = o.layernorm_bwd(gd, xd, w.to(DEV), mean, rstd)
    worst(f"{tag} dx", dx.float(), dx_ref, rtol * 5, atol * 3)
    worst(f"{tag} dw", dw, dw_ref, 2e-4, 1e-4 * max(1, rows ** 0.5))
    worst(f"{tag} db", db, db_ref, 2e-4, 1e-4 * max(1, rows ** 0.5))
    dx2, dw2, db2 = o.layernorm_bwd(gd, xd, w.to(DEV), mean, rstd, dres=rdv)
    worst(f"{tag} dx+dres", dx2.float(), dx_ref + drs.double(), rtol * 5, atol * 4)
    worst(f"{tag} dw (dres form)", dw2, dw_ref, 2e-4, 1e-4 * max(1, rows ** 0.5))
    worst(f"{tag} db (dres form)", db2, db_ref, 2e-4, 1e-4 * max(1, rows ** 0.5))


def _ln_inputs(rows, cols):
    return (rnd(rows, cols, seed=1) * 2 + 0.3, rnd(rows, cols, seed=4), rnd(rows, cols, seed=5),
            1 + 0.1 * rnd(cols, seed=2), 0.05 * rnd(cols, seed=3))


@pytest.mark.parametrize("rows", [2600, 4700])
@pytest.mark.parametrize("dtype,rtol,atol,cols", LN_CASES)
def test_layernorm_bwd_second_half_rows_and_second_trip(rows, dtype, rtol, atol, cols):
    x, dy, dres, w, b = _ln_inputs(rows, cols)
    _ln_fwd_bwd_vs_fp64(x, dy, dres, w, b, dtype, rtol, atol, f"ln {rows}x{cols} {NAMES[dtype]}")


@pytest.mark.parametrize("rows", [2600, 4700])
@pytest.mark.parametrize("dtype,rtol,atol,cols", LN_CASES)
def test_layernorm_bwd_one_hot_rows_count_exactly(rows, dtype, rtol, atol, cols):
    """dy one-hot in the row index (dy[r, r % cols] = 1): db[c] is exactly the number of rows with r % cols == c — small integers, exact in
    fp32 in any summation order — so a row that is dropped, counted twice or counted while invalid changes db by a whole unit.  dw[c] is
    the sum of the same rows' xhat[r, c]."""
    o = ops()
    x = rnd(rows, cols, seed=1) * 2 + 0.3
    w, b = 1 + 0.1 * rnd(cols, seed=2), 0.05 * rnd(cols, seed=3)
    r = torch.arange(rows)
    dy = torch.zeros(rows, cols)
    dy[r, r % cols] = 1.0
    dres = rnd(rows, cols, seed=5)
    rd = lo(dtype)
    xs, drs = rd(x), rd(dres)
    _, _, _, dx_ref, dw_ref, db_ref = _ln_ref(xs, w, b, dy)
    count = torch.bincount(r % cols, minlength=cols).float()
    assert torch.equal(db_ref.float(), count)
    xd, gd = to_dev(x, dtype), to_dev(dy, dtype)
    _, mean, rstd = o.layernorm_fwd(xd, w.to(DEV), b.to(DEV), 1e-5)
    tag = f"ln one-hot {rows}x{cols} {NAMES[dtype]}"
    for res in (None, to_dev(dres, dtype)):
        dx, dw, db = o.layernorm_bwd(gd, xd, w.to(DEV), mean, rstd, dres=res)
        assert torch.equal(db.cpu(), count), (tag, res is not None, (db.cpu() - count).abs().max())
        worst(f"{tag} dw", dw, dw_ref, 2e-4, 1e-4 * max(1, rows ** 0.5))
        worst(f"{tag} dx", dx.float(), dx_ref + (0 if res is None else drs.double()), rtol * 5, atol * (3 if res is None else 4))


@pytest.mark.parametrize("dtype,rtol,atol", DT, ids=[NAMES[d[0]] for d in DT])
@pytest.mark.parametrize("cols,misalign", [(211, False), (64, True)], ids=["211", "64-offset-view"])
def test_layernorm_generic_kernels_with_several_rows_per_partial(dtype, rtol, atol, cols, misalign):
    """ln_bwd_wb_gen: one partial row per `chunk` rows, chunk = ceil(rows / min(rows, 512)) = 3 at rows = 1100 (367 partial rows, the last of
    2 rows).  cols = 211 takes the generic kernels by its width, cols = 64 by a base pointer that is not 16-byte aligned."""
    rows = 1100
    x, dy, dres, w, b = _ln_inputs(rows, cols)
    _ln_fwd_bwd_vs_fp64(x, dy, dres, w, b, dtype, rtol, atol, f"ln generic {rows}x{cols} {NAMES[dtype]}", misalign=misalign)
    o = ops()                                                                    # and the exact row count through the chunked partials
    r = torch.arange(rows)
    dy1 = torch.zeros(rows, cols)
    dy1[r, r % cols] = 1.0
    xd = to_dev(x, dtype)
    _, mean, rstd = o.layernorm_fwd(xd, w.to(DEV), b.to(DEV), 1e-5)
    _, _, db = o.layernorm_bwd(to_dev(dy1, dtype), xd, w.to(DEV), mean, rstd)
    assert torch.equal(db.cpu(), torch.bincount(r % cols, minlength=cols).float())


# ------------------------------------------------------------------------------------------------ 2. LayerNorm forward past one pass; conditioning
@pytest.mark.parametrize("dtype,rtol,atol", DT, ids=[NAMES[d[0]] for d in DT])
@pytest.mark.parametrize("cols", [64, 50], ids=["vector-64", "generic-50"])
def test_layernorm_fwd_past_one_grid_pass(dtype, rtol, atol, cols):
    """2048 workgroups x 4 waves = 8192 rows per pass: at 8200 rows the first 8 waves take a second trip.
    rstd: fp32 statistics of <= 64 values in every dtype: the two-pass variance carries ~ (log2(64) + 3) roundings of 2^-24 = 5e-7 relative,
    rstd half of that plus the square root's and the division's: 1e-5 relative leaves a factor > 10."""
    o = ops()
    rows = 8200
    x = rnd(rows, cols, seed=21) * 2 + 0.3
    w, b = 1 + 0.1 * rnd(cols, seed=2), 0.05 * rnd(cols, seed=3)
    xs = lo(dtype)(x).double()
    y_ref = F.layer_norm(xs, (cols,), w.double(), b.double(), 1e-5)
    y, mean, rstd = o.layernorm_fwd(to_dev(x, dtype), w.to(DEV), b.to(DEV), 1e-5)
    tag = f"ln fwd {rows}x{cols} {NAMES[dtype]}"
    worst(f"{tag} y", y.float(), y_ref, rtol, atol)
    worst(f"{tag} mean", mean, xs.mean(-1), 1e-5, 1e-6)
    worst(f"{tag} rstd", rstd, 1.0 / torch.sqrt(xs.var(-1, unbiased=False) + 1e-5), 1e-5, 0.0)


@pytest.mark.parametrize("cols", [256, 260], ids=["256-full", "260-guarded"])
def test_layernorm_fp32_ill_conditioned_rows(cols):
    """x = 100 + 0.01 randn (|mean| / std = 1e4), one constant row (variance 0: rstd = 1 / sqrt(eps)) and one row with a single 1e4 outlier.
    The fp32 tolerance of the DT table does not apply here: with a mean of 100 one rounding of the mean (2^-18 absolute) is already 4e-4 of
    the row's standard deviation, for ANY fp32 LayerNorm.  So the yardstick is measured in the test: the worst error of torch's own fp32
    layer_norm (and of its autograd backward) on the CPU against fp64 on the same inputs — 1.1e-3 on y at 64 x 256 — and the kernel is allowed
    4 x that: both are two-pass fp32 algorithms that differ only in summation order."""
    o = ops()
    rows = 64
    x = 100.0 + 0.01 * rnd(rows, cols, seed=31)
    x[5] = 100.0
    x[9, 17] = 1e4
    w, b = 1 + 0.1 * rnd(cols, seed=2), 0.05 * rnd(cols, seed=3)
    dy = rnd(rows, cols, seed=4)

    def torch_ln(dt):
        xr = x.to(dt).requires_grad_(True)
        y = F.layer_norm(xr, (cols,), w.to(dt), b.to(dt), 1e-5)
        y.backward(dy.to(dt))
        return y.detach().double(), xr.grad.double()
    y64, dx64 = torch_ln(torch.float64)
    y32, dx32 = torch_ln(torch.float32)
    base_y, base_dx = float((y32 - y64).abs().max()), float((dx32 - dx64).abs().max())
    y, mean, rstd = o.layernorm_fwd(x.to(DEV), w.to(DEV), b.to(DEV), 1e-5)
    dx, _, _ = o.layernorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), mean, rstd)
    err_y, err_dx = float((y.double().cpu() - y64).abs().max()), float((dx.double().cpu() - dx64).abs().max())
    say(f"ln conditioning 64x{cols}: y kernel {err_y:.3e} torch-fp32 {base_y:.3e}; dx kernel {err_dx:.3e} torch-fp32 {base_dx:.3e}")
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    assert err_y <= 4 * base_y, (err_y, base_y)
    assert err_dx <= 4 * base_dx, (err_dx, base_dx)
    # the constant row: its variance is at most one rounding of the mean squared (6e-11) next to eps = 1e-5
    assert abs(float(rstd[5]) * (1e-5 ** 0.5) - 1.0) <= 1e-5


# ------------------------------------------------------------------------------------------------ 4. cross entropy
CE_DT = [pytest.param(torch.float32, 2e-5, id="fp32"), pytest.param(torch.bfloat16, 2e-2, id="bf16")]      # test_ce_fwd_bwd_equals_two_pass_and_oracle


def _ce_ref(xs, labels, seq, shift, ignore, denom_mode=0, denom_rows=0):
    """fp64 reference on the logits the kernel saw; counts the live rows itself -> loss, 1/denom, lse [N], dlogits [N, C], live [N]"""
    N, C = xs.shape
    x = xs.double()
    r = torch.arange(N)
    s = r % seq
    has = s + shift < seq
    t = labels.reshape(-1)[torch.where(has, r + shift, r)]
    live = has & (t != ignore) & (t >= 0) & (t < C)
    lse = torch.logsumexp(x, -1)
    tl = t[live]
    row_loss = lse[live] - x[live, tl]
    denom = float(live.sum()) if denom_mode == 0 else (float(denom_rows) if denom_mode == 1 else 1.0)
    loss = float(row_loss.sum()) / denom if denom != 0 else float("nan")
    p = torch.exp(x - lse[:, None])
    p[r[live], tl] -= 1.0
    d = torch.where(live[:, None], p / denom if denom != 0 else p, torch.zeros((), dtype=torch.float64))
    return loss, (1.0 / denom if denom != 0 else float("inf")), lse, d, live


def _ce_check(tag, got, ref, rtol):
    """(loss_out, row_lse, dlogits) of one form against _ce_ref's tuple, with test_ce_fwd_bwd_equals_two_pass_and_oracle's bounds"""
    lo_, lse, dl = got
    loss_ref, inv_ref, lse_ref, d_ref, live = ref
    torch.cuda.synchronize()
    say(f"{tag}: loss rel {abs(float(lo_[0]) - loss_ref) / abs(loss_ref):.2e} (2e-5); 1/denom rel {abs(float(lo_[1]) - inv_ref) / inv_ref:.2e} (1e-7); "
        f"lse {rel_err(lse, lse_ref):.2e} (1e-6); dlogits {rel_err(dl, d_ref):.2e} ({rtol:.0e})")
    assert abs(float(lo_[0]) - loss_ref) <= 2e-5 * abs(loss_ref), (tag, float(lo_[0]), loss_ref)
    assert abs(float(lo_[1]) - inv_ref) <= 1e-7 * inv_ref, (tag, float(lo_[1]), inv_ref)
    assert torch.isfinite(lse).all() and rel_err(lse, lse_ref) < 1e-6, tag
    assert torch.isfinite(dl).all() and rel_err(dl, d_ref) < rtol, (tag, rel_err(dl, d_ref))
    if (~live).any():
        assert float(dl.float().cpu()[~live].abs().max()) == 0.0, f"{tag}: rows without a target carry a gradient"


def _ce_forms(xd, labels_dev, seq, shift, ignore=-100, denom_mode=0, denom_rows=0):
    """the forms that apply to these logits: two-pass always, one-pass when the rows are 16-byte aligned"""
    o = ops()
    lo2, lse2 = o.ce_fwd(xd, labels_dev, seq=seq, shift=shift, ignore_index=ignore, denom_mode=denom_mode, denom_rows=denom_rows)
    dl2 = o.ce_bwd(xd, labels_dev, lse2, lo2, None, seq=seq, shift=shift, ignore_index=ignore)
    forms = {"two-pass": (lo2, lse2, dl2)}
    if o.ce_fused_ok(xd):
        forms["one-pass"] = o.ce_fwd_bwd(xd, labels_dev, seq=seq, shift=shift, ignore_index=ignore, denom_mode=denom_mode, denom_rows=denom_rows)
    return forms


def _ce_module(xd, labels_dev, reduction, ignore_index):
    """cleantransformer_amd.loss.CrossEntropyLoss forward + backward -> (loss, dlogits)"""
    from cleantransformer_amd.loss import CrossEntropyLoss
    x = xd.detach().clone().requires_grad_(True)
    loss = CrossEntropyLoss(reduction, ignore_index=ignore_index)(x, labels_dev)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), x.grad


def _labels(N, C, seed, ignored, frac=0.3):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, C, (N,), generator=g)
    lab[torch.rand(N, generator=g) < frac] = ignored
    return lab


@pytest.mark.parametrize("dtype,rtol", CE_DT)
@pytest.mark.parametrize("C", [24, 21], ids=["C24-vector", "C21-two-pass-only"])
@pytest.mark.parametrize("seq,shift", [(2500, 0), (50, 1)], ids=["seq2500-shift0", "seq50-shift1"])
def test_cross_entropy_row_loops_past_1024_rows(dtype, rtol, C, seq, shift):
    """ce_count_k / ce_finalize_k stride by 1024 over the rows: N = 2500 makes every thread take two or three trips; ~30 % of the labels are
    ignored, so the live count (the denominator, and loss_out[1]) is a number the reference has to count for itself."""
    N = 2500
    x = rnd(N, C, seed=3, scale=2.0)
    lab = _labels(N, C, 4, -100)
    xd = to_dev(x, dtype)
    ref = _ce_ref(xd.float().cpu(), lab, seq, shift, -100)
    assert 0 < int(ref[4].sum()) < N * 0.8
    forms = _ce_forms(xd, lab.to(DEV), seq, shift)
    assert ("one-pass" in forms) == (C == 24)
    for name, got in forms.items():
        _ce_check(f"ce {name} N={N} C={C} seq={seq} {NAMES[dtype]}", got, ref, rtol)
    if shift == 0:
        loss, grad = _ce_module(xd, lab.to(DEV), "mean", -100)
        assert abs(float(loss) - ref[0]) <= 2e-5 * abs(ref[0])
        assert rel_err(grad, ref[3]) < rtol and float(grad.float().cpu()[~ref[4]].abs().max()) == 0.0


@pytest.mark.parametrize("dtype,rtol", CE_DT)
@pytest.mark.parametrize("C", [24, 21])
@pytest.mark.parametrize("reduction,ignore_index", [("mean", None), ("sum", None), ("mean", 7), ("sum", 7)])
def test_cross_entropy_module_denominators_and_in_range_ignore_index(dtype, rtol, C, reduction, ignore_index):
    """CrossEntropyLoss('mean' | 'sum', ignore_index=None | 7) = denom_mode 1 | 2 | 0 | 2 of the kernels, at N = 2500 with ~30 % of the rows dead.
    ignore_index = 7 is a class inside [0, C): torch.nn.functional.cross_entropy is the reference.  ignore_index = None is loss.py's rule: the sum
    over the rows that have a class, divided by ALL N rows for 'mean' — dead rows are labels outside [0, C) there."""
    N = 2500
    x = rnd(N, C, seed=5, scale=2.0)
    xd = to_dev(x, dtype)
    xs = xd.float().cpu().double().requires_grad_(True)
    if ignore_index is None:
        lab = _labels(N, C, 6, -100)
        live = lab >= 0
        lref = F.cross_entropy(xs[live], lab[live], reduction="sum") / (N if reduction == "mean" else 1)
        mode, ign = (1 if reduction == "mean" else 2), -(1 << 62)
    else:
        lab = _labels(N, C, 6, ignore_index)
        live = lab != ignore_index
        lref = F.cross_entropy(xs, lab, reduction=reduction, ignore_index=ignore_index)
        mode, ign = (0 if reduction == "mean" else 2), ignore_index
    lref.backward()
    lref = lref.detach()
    assert 0 < int(live.sum()) < N * 0.8
    loss, grad = _ce_module(xd, lab.to(DEV), reduction, ignore_index)
    tag = f"ce module {reduction} ignore={ignore_index} C={C} {NAMES[dtype]}"
    say(f"{tag}: loss rel {abs(float(loss) - float(lref)) / abs(float(lref)):.2e} (2e-5); dlogits {rel_err(grad, xs.grad):.2e} ({rtol:.0e})")
    assert abs(float(loss) - float(lref)) <= 2e-5 * abs(float(lref)), (tag, float(loss), float(lref))
    assert rel_err(grad, xs.grad) < rtol, tag
    assert float(grad.float().cpu()[~live].abs().max()) == 0.0, tag
    # the same denominators through both kernel forms (ce_count_k has its own copy of the rule), against the fp64 reference of this file
    ref = _ce_ref(xd.float().cpu(), lab, N, 0, ign, mode, N)
    assert abs(ref[0] - float(lref)) <= 1e-12 * abs(float(lref))
    for name, got in _ce_forms(xd, lab.to(DEV), N, 0, ign, mode, N).items():
        _ce_check(f"{tag} {name}", got, ref, rtol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [24, 21])
def test_cross_entropy_all_rows_ignored(dtype, C):
    """no row has a target: the mean over zero rows is NaN, as torch's is, and the gradient is exactly zero — not 0 * inf."""
    N = 2500
    xd = to_dev(rnd(N, C, seed=7, scale=2.0), dtype)
    ref = F.cross_entropy(xd.float().cpu().double(), torch.full((N,), 7), ignore_index=7)
    assert torch.isnan(ref)
    for lab, ign in ((torch.full((N,), -100), -100), (torch.full((N,), 7), 7)):
        for name, (lo_, lse, dl) in _ce_forms(xd, lab.to(DEV), N, 0, ign).items():
            assert torch.isnan(lo_[0]), (name, ign)
            assert torch.isfinite(lse).all() and rel_err(lse, torch.logsumexp(xd.float().cpu().double(), -1)) < 1e-6
            assert not torch.isnan(dl).any() and float(dl.float().abs().max()) == 0.0, (name, ign)
    loss, grad = _ce_module(xd, torch.full((N,), 7).to(DEV), "mean", 7)
    assert torch.isnan(loss) and not torch.isnan(grad).any() and float(grad.float().abs().max()) == 0.0


CE_WIDE = [4104, 24584]     # 513 / 3073 16-byte chunks of bf16: one vector trip for half the threads; the smallest row that enters ce_fused_k's 4-deep loop


@pytest.mark.parametrize("dtype,rtol", CE_DT)
@pytest.mark.parametrize("C", CE_WIDE)
def test_cross_entropy_large_magnitudes(dtype, rtol, C):
    """logits 30 * randn (row maxima around 120), one row whose target is 60 above every other logit (p -> 1, gradient p - 1 -> 0) and one row
    shifted by +80.  lse = M + log(S): the reference's magnitude sets the bound, 2 ulp of fp32 at |lse_ref| (one rounding of the final sum, one
    of the row maximum's spacing inside exp) + 1e-6 for log(S) itself."""
    N = 8
    x = rnd(N, C, seed=9, scale=30.0)
    lab = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(10))
    x[1, int(lab[1])] = x[1].max() + 60.0
    x[2] += 80.0
    xd = to_dev(x, dtype)
    ref = _ce_ref(xd.float().cpu(), lab, N, 0, -100)
    lse_ref = ref[2]
    ulp = torch.tensor([float(torch.nextafter(v.abs().float(), torch.tensor(float("inf"))) - v.abs().float()) for v in lse_ref], dtype=torch.float64)
    forms = _ce_forms(xd, lab.to(DEV), N, 0)
    assert "one-pass" in forms
    for name, got in forms.items():
        tag = f"ce magnitude {name} C={C} {NAMES[dtype]}"
        err = (got[1].double().cpu() - lse_ref).abs()
        say(f"{tag}: lse worst err/(2 ulp + 1e-6) {float((err / (2 * ulp + 1e-6)).max()):.3f}")
        assert bool((err <= 2 * ulp + 1e-6).all()), (tag, err.tolist(), ulp.tolist())
        _ce_check(tag, got, ref, rtol)
    loss, grad = _ce_module(xd, lab.to(DEV), "mean", None)
    assert abs(float(loss) - ref[0]) <= 2e-5 * abs(ref[0]) and rel_err(grad, ref[3]) < rtol


def _ce_masked_case(dtype, rtol, C, masked, tag, padded=False):
    N = 8
    x = rnd(N, C, seed=11, scale=2.0)
    x[:, masked] = float("-inf")
    keep = (~masked).nonzero()[:, 0]
    lab = keep[torch.randint(0, keep.numel(), (N,), generator=torch.Generator().manual_seed(12))]      # the targets stay unmasked
    xd = to_dev(x, dtype)
    if padded:                                                                                           # rows of ops.pad_rows(C), as LMHeadFn keeps an odd vocabulary
        buf = torch.full((N, ops().pad_rows(C)), float("nan"), dtype=dtype, device=DEV)
        buf[:, :C].copy_(xd)
        xd = buf[:, :C]
    ref = _ce_ref(xd.float().cpu(), lab, N, 0, -100)
    xs = xd.float().cpu().double().requires_grad_(True)
    lt = F.cross_entropy(xs, lab)                                                                        # torch: finite loss, exact zeros
    lt.backward()
    lt = lt.detach()
    assert torch.isfinite(lt) and abs(float(lt) - ref[0]) <= 1e-12 * abs(ref[0]) and float(xs.grad[:, masked].abs().max()) == 0.0
    forms = dict(_ce_forms(xd, lab.to(DEV), N, 0))
    loss, grad = _ce_module(xd, lab.to(DEV), "mean", None)
    for name, got in forms.items():
        _ce_check(f"{tag} {name}", got, ref, rtol)
        assert float(got[2].float().cpu()[:, masked].abs().max()) == 0.0, f"{tag} {name}: a masked class carries a gradient"
    assert torch.isfinite(loss) and abs(float(loss) - ref[0]) <= 2e-5 * abs(ref[0]), (tag, float(loss))
    assert torch.isfinite(grad).all() and rel_err(grad, ref[3]) < rtol and float(grad.float().cpu()[:, masked].abs().max()) == 0.0, tag


@pytest.mark.parametrize("dtype,rtol", CE_DT)
@pytest.mark.parametrize("C", CE_WIDE)
@pytest.mark.parametrize("kind", ["first-4096", "every-7th"])
def test_cross_entropy_minus_inf_logits(dtype, rtol, C, kind):
    """a masked vocabulary slice (logits = -inf): torch gives a finite loss and exact zeros in the masked columns, and so must the kernels.
    Columns [0, 4096) masked: whole 16-byte chunks — and, in the one-pass kernel at C = 24584, a thread's whole first 4-deep trip — are -inf
    while the thread's running maximum is still -inf.  Every column = 3 mod 7 masked: -inf next to finite values in every chunk."""
    c = torch.arange(C)
    masked = (c < 4096) if kind == "first-4096" else (c % 7 == 3)
    _ce_masked_case(dtype, rtol, C, masked, f"ce -inf {kind} C={C} {NAMES[dtype]}")


@pytest.mark.parametrize("dtype,rtol", CE_DT)
def test_cross_entropy_minus_inf_last_class_scalar_path(dtype, rtol):
    """C = 21 (rows not 16-byte aligned: two-pass form, one class per thread): the last class masked"""
    masked = torch.arange(21) == 20
    _ce_masked_case(dtype, rtol, 21, masked, f"ce -inf last-class C=21 {NAMES[dtype]}")


@pytest.mark.parametrize("dtype,rtol", CE_DT)
def test_cross_entropy_minus_inf_then_finite_in_the_scalar_loops(dtype, rtol):
    """the one-class-at-a-time loops see -inf FIRST and a finite class later (a state whose maximum is still -inf at the end is dropped by the
    cross-lane merge, NaN or not, so the case above passes with or without the per-thread guard; these do not):
    C = 277 (two-pass form, 256 threads): columns [0, 256) masked — threads 0 .. 20 read -inf, then a finite class;
    C = 4099 at the padded pitch (both forms): the scalar tail [4096, 4099) — read before the vector body — masked."""
    _ce_masked_case(dtype, rtol, 277, torch.arange(277) < 256, f"ce -inf first-256 C=277 {NAMES[dtype]}")
    _ce_masked_case(dtype, rtol, 4099, torch.arange(4099) >= 4096, f"ce -inf tail C=4099 padded {NAMES[dtype]}", padded=True)


# ------------------------------------------------------------------------------------------------ 6. embedding
EMB_N, EMB_V = 16400, 211           # 4096 workgroups x 4 waves = 16384 tokens per pass: the first 16 waves take a second trip


def _ids(bad=False, seed=6):
    ids = torch.randint(0, EMB_V, (EMB_N,), generator=torch.Generator().manual_seed(seed))
    if bad:
        ids[3], ids[16390], ids[777] = -1, EMB_V, EMB_V + 5
    return ids


@pytest.mark.parametrize("dtype,H", [(torch.float32, 64), (torch.bfloat16, 64), (torch.float32, 50), (torch.bfloat16, 50)],
                         ids=["fp32-64", "bf16-64", "fp32-50-scalar", "bf16-50-scalar"])
def test_embedding_gather_past_one_pass_and_bad_ids(dtype, H):
    o = ops()
    td = to_dev(rnd(EMB_V, H, seed=5), dtype)
    for bad in (False, True):
        ids = _ids(bad)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = o.embed_fwd(td, ids.to(DEV), err_flag=flag)
        safe = torch.where((ids < 0) | (ids >= EMB_V), torch.zeros_like(ids), ids)      # an id outside the table reads row 0 and raises the flag
        assert torch.equal(out.cpu(), td.cpu()[safe]), (bad, "gather is bit-exact")
        assert int(flag.item()) == int(bad)
    out = o.embed_fwd(td, _ids(True).to(DEV))                                           # no flag given: same rows, nothing written
    assert torch.equal(out.cpu(), td.cpu()[safe])


def _embed_bwd_check(tag, dtable, prefill, dout_seen, ids, scale):
    """fp64 index_add_; bound = the existing 1e-5 relative + 1e-6, plus the order of the fp32 atomic adds: an entry that receives n_dup
    contributions is a chain of n_dup fp32 additions in any order: at most n_dup * 2^-24 * (|prefill| + sum |contribution|)."""
    ok = (ids >= 0) & (ids < EMB_V)
    contrib = (scale * dout_seen.double())[ok]
    ref = prefill.double().clone().index_add_(0, ids[ok], contrib)
    mag = prefill.double().abs().index_add_(0, ids[ok], contrib.abs())
    ndup = torch.bincount(ids[ok], minlength=EMB_V).double()[:, None]
    bound = 1e-6 + 1e-5 * ref.abs() + ndup * 2.0 ** -24 * mag
    err = (dtable.double().cpu() - ref).abs()
    say(f"{tag}: max |err| {float(err.max()):.3e}; worst err/bound {float((err / bound).max()):.3f}")
    assert torch.isfinite(dtable).all() and bool((err <= bound).all()), (tag, float((err / bound).max()))
    untouched = ndup[:, 0] == 0
    assert torch.equal(dtable.cpu()[untouched], prefill[untouched]), f"{tag}: a row no id names was written"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["dout-fp32", "dout-bf16"])
@pytest.mark.parametrize("H", [64, 50])
def test_embedding_scatter_add_past_one_pass_scaled_onto_a_filled_table(dtype, H):
    o = ops()
    ids = _ids(True, seed=8)
    dout = to_dev(rnd(EMB_N, H, seed=7), dtype)
    prefill = rnd(EMB_V, H, seed=9)
    dt = prefill.to(DEV)
    o.embed_bwd(dout, ids.to(DEV), dt, scale=0.25)
    _embed_bwd_check(f"embed.bwd H={H} {NAMES[dtype]}", dt, prefill, dout.float().cpu(), ids, 0.25)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["dout-fp32", "dout-bf16"])
def test_embedding_scatter_add_every_token_on_one_row(dtype):
    """16400 atomic adds per element of ONE row; every other row of the table keeps its bits"""
    o = ops()
    H = 64
    ids = torch.full((EMB_N,), 5)
    dout = to_dev(rnd(EMB_N, H, seed=7), dtype)
    prefill = rnd(EMB_V, H, seed=9)
    dt = prefill.to(DEV)
    o.embed_bwd(dout, ids.to(DEV), dt, scale=0.25)
    _embed_bwd_check(f"embed.bwd contention {NAMES[dtype]}", dt, prefill, dout.float().cpu(), ids, 0.25)


# ------------------------------------------------------------------------------------------------ 7. utilities
CAST_OK = [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.float32, torch.float16), (torch.bfloat16, torch.float32),
           (torch.float16, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16)]


def _same_bits(a, b):
    """bit-exact, except that any NaN equals any NaN"""
    a, b = a.cpu(), b.cpu()
    assert a.dtype == b.dtype and a.shape == b.shape
    nan = torch.isnan(b)
    assert torch.equal(torch.isnan(a), nan)
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return torch.equal(a.view(it)[~nan], b.view(it)[~nan])


@pytest.mark.parametrize("sd,dd", CAST_OK, ids=[f"{NAMES[a]}-to-{NAMES[b]}" for a, b in CAST_OK])
def test_cast_every_pair_odd_unaligned_and_past_one_pass(sd, dd):
    """n = 4099: odd (the float4 fp32 -> bf16 kernel does not apply; cast_k's last trip is partial); the same on views one element past a 16-byte
    boundary; n = 4 * 2^20 + 12: 4096 workgroups x 256 threads x 4 elements is one pass of the float4 kernel, and four of cast_k."""
    o = ops()
    for n, off in ((4099, 0), (4099, 1), (4 * (1 << 20) + 12, 0)):
        src = (rnd(n + 8, seed=n + off) * 3).to(sd).to(DEV)[off:off + n]
        out = torch.zeros(n + 8, dtype=dd, device=DEV)
        got = o.cast(src, dd, out=out[off:off + n])
        assert _same_bits(got, src.cpu().to(dd)), (n, off)
        assert float(out[:off].float().abs().sum()) == 0.0 and float(out[off + n:].float().abs().sum()) == 0.0     # nothing outside [off, off + n)
    assert _same_bits(o.cast(src[:4099], dd), src[:4099].cpu().to(dd))                 # and into a tensor the library allocates


def test_cast_between_the_two_16_bit_types_is_an_error():
    o = ops()
    from cleantransformer_amd._lib import CtmiError
    for sd, dd in ((torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16)):
        with pytest.raises(CtmiError, match="unsupported"):
            o.cast(torch.ones(64, dtype=sd, device=DEV), dd)


@pytest.mark.parametrize("dd", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_cast_special_values_round_to_nearest_even(dd):
    o = ops()
    bits = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF,            # bf16: ties between neighbours (to even: down, up), just above / below a tie
            0x3F801000, 0x3F803000, 0x3F801001, 0x3F802FFF]            # fp16: the same at 1 + 2^-11, 1 + 3 * 2^-11
    vals = torch.tensor(bits, dtype=torch.int32).view(torch.float32).tolist()
    f32max = torch.finfo(torch.float32).max
    vals += [0.0, -0.0, f32max, -f32max, 65504.0, 65519.996, 65520.0, -65520.0, 70000.0, 3.3895e38, 3.3961775e38,
             2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 * 1.0001, 1e-7, 5e-6, 6.0e-5, 2.0 ** -14,                    # fp16 subnormals, ties among them
             2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -127, 1e-39, -1e-40, 2.0 ** -126,                              # bf16 subnormals
             float("inf"), float("-inf"), float("nan")]
    src = torch.tensor(vals, dtype=torch.float32)
    assert src.numel() % 4 != 0
    src4 = torch.cat([src, src.flip(0)[: 4 - src.numel() % 4]])          # a multiple of 4: the float4 kernel for bf16
    for s in (src, src4):
        base = torch.zeros(s.numel() + 8, device=DEV)
        for off in (0, 1):
            v = base[off:off + s.numel()]
            v.copy_(s)
            assert _same_bits(o.cast(v, dd), s.to(dd)), (dd, off, o.cast(v, dd).cpu().tolist(), s.to(dd).tolist())
    big = o.cast(torch.tensor([f32max, 65520.0, 70000.0], device=DEV), dd).cpu().float()
    assert torch.isinf(big).tolist() == ([True, False, False] if dd == torch.bfloat16 else [True, True, True])


def test_sumsq_past_one_pass_accumulate_and_empty():
    """1024 workgroups x 256 threads x 8 = 2^21 elements per pass.  fp64 accumulation: relative 1e-12 against torch in fp64."""
    o = ops()
    n = (1 << 21) + 4099
    x = rnd(n, seed=13)
    xd = x.to(DEV)
    ref = x.double().pow(2).sum().reshape(1)
    worst("sumsq", o.sumsq(xd), ref, 1e-12, 0.0)
    out = torch.full((1,), 12345.678, dtype=torch.float64, device=DEV)
    assert o.sumsq(xd, out=out, accumulate=True).data_ptr() == out.data_ptr()
    worst("sumsq accumulate", out, ref + 12345.678, 1e-12, 0.0)
    out = torch.full((1,), 9e9, dtype=torch.float64, device=DEV)
    o.sumsq(xd, out=out, accumulate=False)
    worst("sumsq overwrite", out, ref, 1e-12, 0.0)
    out = torch.full((1,), 3.5, dtype=torch.float64, device=DEV)
    o.sumsq(xd[:0], out=out, accumulate=True)
    assert float(out) == 3.5
    o.sumsq(xd[:0], out=out, accumulate=False)
    assert float(out) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", [64, 211, 1032])
def test_colsum_row_counts_tails_and_accumulate(dtype, N):
    """M = 1, 15, 17, 61, 1100: fewer rows than the 4 waves of a workgroup; one part whose 4-loads-in-flight loop never runs; one row past a part;
    a tail of every length; several parts of 16+ rows with a shorter last one.  N = 211: the scalar-load kernel; 1032: a partial last column block."""
    o = ops()
    for M in (1, 15, 17, 61, 1100):
        x = rnd(M, N, seed=M + N)
        xd = to_dev(x, dtype)
        ref = xd.float().cpu().double().sum(0)
        scm = 1.0 / M ** 0.5
        worst(f"colsum {M}x{N} {NAMES[dtype]}", o.colsum(xd) * scm, ref * scm, 1e-5, 1e-5)
        pre = rnd(N, seed=77)
        out = pre.to(DEV)
        assert o.colsum(xd, out=out, accumulate=True).data_ptr() == out.data_ptr()
        worst(f"colsum accumulate {M}x{N} {NAMES[dtype]}", out * scm, (ref + pre.double()) * scm, 1e-5, 1e-5)
        r = torch.arange(M)                                                      # one-hot rows: exact counts, whatever the summation order
        one = torch.zeros(M, N)
        one[r, r % N] = 1.0
        count = torch.bincount(r % N, minlength=N).float()
        assert torch.equal(o.colsum(to_dev(one, dtype)).cpu(), count), (M, N)
        out = torch.full((N,), 3.0, device=DEV)
        o.colsum(to_dev(one, dtype), out=out, accumulate=True)
        assert torch.equal(out.cpu(), count + 3.0), (M, N)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_scale_if_on_a_padded_pitch_past_one_pass(dtype):
    """min(rows, 4096) workgroups: rows 4096 .. 4099 are a second trip.  The tensor is a column slice of a wider buffer."""
    o = ops()
    rows, cols, pitch = 4100, 50, 72
    buf = to_dev(rnd(rows, pitch, seed=15), dtype)
    keep = buf.clone()
    x = buf[:, :cols]
    before = o.scale_if_passes()
    o.scale_if_(x, torch.ones(1, device=DEV))
    o.scale_if_(x, torch.full((1,), 0.5, device=DEV), applied=0.25, applied_dev=torch.full((1,), 2.0, device=DEV))      # 0.5 / (0.25 * 2): exactly 1
    torch.cuda.synchronize()
    assert torch.equal(buf, keep) and o.scale_if_passes() == before
    o.scale_if_(x, torch.full((1,), 0.25, device=DEV))
    assert o.scale_if_passes() == before + 1
    assert torch.equal(buf[:, :cols].float(), keep[:, :cols].float() * 0.25)           # a power of two: exact in both dtypes
    assert torch.equal(buf[:, cols:], keep[:, cols:])                                   # the pad columns are untouched
    o.scale_if_(x, torch.full((1,), 2.0, device=DEV), applied=0.25, applied_dev=torch.full((1,), 2.0, device=DEV))      # 2 / 0.5 = 4: back to the start
    assert torch.equal(buf, keep) and o.scale_if_passes() == before + 2
