"""CPU: every exported entry that takes a storage-type code refuses an unknown one (99) before any launch, with the
return code and the message recorded from the library as it was before the entries shared one dispatcher
(csrc/common.h ctmi_by_dtype).  No GPU is touched: the pointers are addresses inside a small host buffer, the entry
returns from its argument checks (a ProfScope is inert while profiling is off, csrc/prof.h).

Not covered: ctmi_bloom_block_fwd/bwd (the code is a field of their struct), ctmi_wgrad_grouped and
ctmi_bloom_block_wgrad_grouped (one "unsupported problem set" answer for everything outside their envelope),
ctmi_ddp_all_reduce / broadcast (need a communicator), and the int64 layout helpers (no error path)."""
import ctypes as C

import pytest

ARG, UNSUPPORTED = -1, -3
BAD = 99


@pytest.fixture(scope="module")
def lib():
    from cleantransformer_amd import _build, _lib
    _build.build(verbose=False)
    return _lib.load()


_buf = C.create_string_buffer(4096 + 64)
P = (C.addressof(_buf) + 63) & ~63                    # a 64-byte aligned host address: never dereferenced


def _desc():
    from cleantransformer_amd import _lib
    d = _lib.AttnDesc()
    d.B, d.nh, d.Sq, d.Sk, d.hd = 1, 1, 4, 4, 8
    d.q_bs = d.k_bs = d.v_bs = d.o_bs = 32
    d.q_hs = d.k_hs = d.v_hs = d.o_hs = 32
    d.q_rs = d.k_rs = d.v_rs = d.o_rs = 8
    d.scale, d.causal = 1.0, 1
    return d


# entry (without the ctmi_ prefix) -> (arguments, return code, message); None = a NULL pointer / the default stream
CASES = {
    "layernorm_fwd": ((P, P, P, P, P, P, 2, 8, 1e-5, BAD, None), UNSUPPORTED, "layernorm_fwd: unsupported dtype 99"),
    "layernorm_bwd": ((P, P, P, P, P, None, P, P, P, 0, P, 2, 8, BAD, None), UNSUPPORTED, "layernorm_bwd: unsupported dtype 99"),
    "colsum": ((P, 8, P, 0, P, 2, 8, BAD, None), UNSUPPORTED, "colsum: unsupported dtype 99"),
    "dropout": ((P, None, P, 8, 0.25, 1, BAD, None), UNSUPPORTED, "dropout: unsupported dtype 99"),
    "embed_fwd": ((P, P, P, 2, 8, 4, BAD, None, None), UNSUPPORTED, "embed_fwd: unsupported dtype 99"),
    "embed_bwd": ((P, P, P, 2, 8, 4, BAD, 1.0, None), UNSUPPORTED, "embed_bwd: unsupported dtype 99"),
    "ce_fwd": ((P, 8, P, P, P, P, 2, 8, 2, 1, -100, 0, 0, BAD, None), UNSUPPORTED, "ce_fwd: unsupported dtype 99"),
    "ce_bwd": ((P, 8, P, P, P, None, P, 8, 2, 8, 2, 1, -100, BAD, None), UNSUPPORTED, "ce_bwd: unsupported dtype 99"),
    "ce_fwd_bwd": ((P, 8, P, P, P, P, P, 8, 2, 8, 2, 1, -100, 0, 0, 1.0, None, BAD, None), ARG, "ce_fwd_bwd: unsupported dtype 99"),
    "scale_if": ((P, 8, 2, 8, P, 1.0, None, BAD, None), UNSUPPORTED, "scale_if: unsupported dtype 99"),
    "ce_soft_fwd": ((P, 8, P, 8, P, P, P, P, 2, 8, 1, 2, BAD, None), UNSUPPORTED, "ce_soft_fwd: unsupported dtype 99"),
    "ce_soft_bwd": ((P, 8, P, 8, P, P, P, None, P, 8, 2, 8, BAD, None), UNSUPPORTED, "ce_soft_bwd: unsupported dtype 99"),
    "cast": ((P, BAD, P, 0, 8, None), UNSUPPORTED, "cast: unsupported dtypes 99->0"),
    "cast:dst": ((P, 0, P, BAD, 8, None), UNSUPPORTED, "cast: unsupported dtypes 0->99"),
    "cast:bf16->fp16": ((P, 1, P, 2, 8, None), UNSUPPORTED, "cast: unsupported dtypes 1->2"),
    "cast:fp16->bf16": ((P, 2, P, 1, 8, None), UNSUPPORTED, "cast: unsupported dtypes 2->1"),
    "transpose_cast": ((P, P, BAD, 2, 8, None), UNSUPPORTED, "transpose_cast: unsupported dtype 99"),
    "argmax": ((P, 8, P, 2, 8, BAD, None), UNSUPPORTED, "argmax: unsupported dtype 99"),
    "row_lse": ((P, 8, P, 2, 8, BAD, None), UNSUPPORTED, "row_lse: unsupported dtype 99"),
    "group_topk": ((P, 8, None, None, 1.0, P, P, 1, 2, 8, 2, BAD, None), UNSUPPORTED, "group_topk: unsupported dtype 99"),
    "attn_fwd": ((P, P, P, P, P, P, None, None, None, None, None, "desc", BAD, None), ARG, "attn_fwd: unsupported dtype 99"),
    "attn_bwd": ((P, P, P, P, P, P, P, P, P, P, P, None, None, None, None, None, "desc", BAD, None), ARG, "attn_bwd: unsupported dtype 99"),
    "lora_project": ((P, 64, P, 64, 0, P, 8, 4, 64, 8, 1.0, BAD, None), UNSUPPORTED,
                     "lora_project: dtype 99 (bf16 / fp16 only; fp32 goes through ctmi_gemm)"),
    "lora_project:fp32": ((P, 64, P, 64, 0, P, 8, 4, 64, 8, 1.0, 0, None), UNSUPPORTED,
                          "lora_project: dtype 0 (bf16 / fp16 only; fp32 goes through ctmi_gemm)"),
    "lora_expand_add": ((P, 8, P, 8, 1, P, 64, 4, 64, 8, BAD, None), UNSUPPORTED,
                        "lora_expand_add: dtype 99 (bf16 / fp16 only; fp32 goes through ctmi_gemm)"),
    "lora_wgrad": ((P, 8, P, 64, P, 64, 4, 8, 64, 1.0, P, 4096, BAD, None), UNSUPPORTED,
                   "lora_wgrad: dtype 99 (bf16 / fp16 only; fp32 goes through ctmi_gemm)"),
    "gemm": ((P, 8, 0, P, 8, 0, P, 8, 2, 8, 8, 1.0, 0, None, None, 0, None, None, 0, BAD, None, 0, None), ARG, "gemm: unsupported dtype 99"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_unknown_dtype_is_refused_before_any_launch(lib, case):
    args, want_rc, want_msg = CASES[case]
    entry = case.split(":")[0]
    desc = _desc()
    args = tuple(C.byref(desc) if a == "desc" else a for a in args)
    rc = getattr(lib, "ctmi_" + entry)(*args)
    msg = lib.ctmi_last_error().decode()
    assert rc == want_rc, (rc, msg)
    assert msg.startswith(entry + ":"), msg
    assert msg == want_msg


def test_every_dtype_entry_of_the_header_is_listed():
    """an entry that gains a dtype argument has to be added to CASES (or to the docstring's exceptions)"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ctmi355.h")).read(), flags=re.S)
    with_dtype = {m.group(1) for m in re.finditer(r"\bint\s+ctmi_(\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S) if re.search(r"\bint (\w+_)?dtype\b", m.group(2))}
    exceptions = {"ddp_all_reduce", "ddp_broadcast", "bloom_block_wgrad_grouped", "wgrad_grouped"}
    assert with_dtype - exceptions == {c.split(":")[0] for c in CASES}, with_dtype ^ {c.split(":")[0] for c in CASES}
