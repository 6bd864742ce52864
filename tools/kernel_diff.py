#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds of libctmi355.so the same code?  (no GPU needed)

usage: python tools/kernel_diff.py A.so B.so

Compares, per kernel of the bundled gfx950 code objects: the symbol names, every field of the AMDGPU metadata record (registers, spills, LDS,
scratch, kernarg size, the argument list) and the disassembly.  What differs between two links of the same code is dropped from the disassembly
first (normalise): instruction addresses and encodings, branch-target labels, the nop padding behind a kernel, and the pc-relative offsets of
named globals.  Prints the names that differ and exits 1 if any do.  A plain diff: it looks for no particular instruction.

The acceptance test of a source-only refactor: build the parent and the change with the project's build() and compare the two libraries.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources  # noqa: E402

LLVM = kernel_resources.LLVM
_PAD = re.compile(r"s_nop 0$|s_code_end$|\.\.\.$|v_illegal$")
_PCREL = re.compile(r"(s_addc?_u32 (s\d+), \2, )(?:0x[0-9a-f]+|\d+)$")


def normalise(listing):
    """Disassembly lines of ONE kernel (llvm-objdump -d, without its `<symbol>:` header) -> the instruction text that has to match."""
    out, pcrel = [], 0
    for line in listing:
        text = line.split("//")[0].strip()                                    # the comment holds the address, the encoding and a branch's target label
        if not text or re.match(r"(?:[0-9a-f]+ )?<[^>]+>:$", text):           # blank, or a label line
            continue
        text = re.sub(r"\s+", " ", text)
        if text.startswith("s_getpc_b64"):
            pcrel = 2                                                          # the add / addc pair behind it forms the address of a named global
        elif pcrel:
            m = _PCREL.match(text)
            text, pcrel = (m.group(1) + "<pcrel>", pcrel - 1) if m else (text, 0)
        out.append(text)
    while out and _PAD.match(out[-1]):
        out.pop()
    return out


def _code_objects(lib_path, tmp):
    local = os.path.join(tmp, "lib.so")
    shutil.copy(lib_path, local)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], cwd=tmp, check=True, capture_output=True)
    return [os.path.join(tmp, f) for f in sorted(os.listdir(tmp)) if "gfx950" in f]


def _run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def metadata_records(notes):
    """llvm-readelf --notes text -> {mangled kernel name: the lines of its record, argument list included}."""
    recs, cur = {}, None
    for line in notes.splitlines():
        if re.match(r"\s+- \.agpr_count:", line):                             # (a kernel record starts with "- .agpr_count")
            cur = []
        elif cur is not None and not re.match(r"\s{4,}\S", line):             # back at the top level: amdhsa.target, amdhsa.version, ...
            cur = None
        if cur is not None:
            cur.append(re.sub(r"\s+", " ", line.strip()))
            m = re.match(r"\s{4}\.name:\s+(\S+)$", line)                        # (indent 4: the kernel's own field, not an argument's)
            if m:
                recs[m.group(1)] = cur
    return recs


def disassembly(listing):
    """llvm-objdump -d text -> {symbol: normalised instruction list}."""
    out, cur = {}, None
    for line in listing.splitlines():
        m = re.match(r"[0-9a-f]+ <([^>]+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None:
            cur.append(line)
    return {k: normalise(v) for k, v in out.items()}


def read(lib_path):
    """-> (resources by demangled name [kernel_resources.read], metadata records by mangled name, normalised disassembly by mangled name)"""
    meta, code = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in _code_objects(lib_path, tmp):
            meta.update(metadata_records(_run("llvm-readelf", "--notes", co)))
            code.update(disassembly(_run("llvm-objdump", "-d", co)))
    return kernel_resources.read(lib_path), meta, code


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (res_a, meta_a, code_a), (res_b, meta_b, code_b) = read(sys.argv[1]), read(sys.argv[2])
    bad = 0
    print(f"kernels: {len(meta_a)} / {len(meta_b)};  code symbols: {len(code_a)} / {len(code_b)}")
    for what, a, b in (("kernel", meta_a, meta_b), ("code symbol", code_a, code_b)):
        for n in sorted(set(a) ^ set(b)):
            bad += 1
            print(f"{what} only in {'A' if n in a else 'B'}: {n}")
    for n in sorted(set(res_a) & set(res_b)):
        d = [f"{f} {res_a[n].get(f)} -> {res_b[n].get(f)}" for f in kernel_resources.FIELDS if res_a[n].get(f) != res_b[n].get(f)]
        if d:
            print(f"resources differ: {n}: " + ", ".join(d))
    for n in sorted(set(meta_a) & set(meta_b)):
        if meta_a[n] != meta_b[n]:
            bad += 1
            d = [f"{x} -> {y}" for x, y in zip(meta_a[n], meta_b[n]) if x != y]
            print(f"metadata differs: {n}: " + "; ".join(d[:6]) + (f" (records of {len(meta_a[n])} / {len(meta_b[n])} lines)" if len(meta_a[n]) != len(meta_b[n]) else ""))
    ndis = 0
    for n in sorted(set(code_a) & set(code_b)):
        if code_a[n] != code_b[n]:
            ndis += 1
            first = next((i for i, (x, y) in enumerate(zip(code_a[n], code_b[n])) if x != y), min(len(code_a[n]), len(code_b[n])))
            print(f"disassembly differs: {n}: {len(code_a[n])} -> {len(code_b[n])} instructions, first difference at instruction {first}")
    print(f"{ndis} kernels with differing disassembly; {bad} differences in symbols and metadata")
    sys.exit(1 if bad or ndis else 0)


if __name__ == "__main__":
    main()
