"""Adapter step vs full fine-tuning step on one MI355X: Bloom-560M, B = 8, S = 1024, bf16, r = 16 on query_key_value.

    python tools/bench_lora.py [--pairs 5] [--steps 10] [--warmup 4] [--out profiles/lora_step.txt]

Both models live in one process and are timed as INTERLEAVED pairs (full, adapter, full, adapter, ...): each sample is `--steps` steps of the
ft_bloom.py loop (forward -> zero_grad -> backward -> fused AdamW) between two device events, ended by a synchronise.  The full step is this tree's
one-call block path (the code the adapters leave untouched).  A non-finite loss aborts the run.  Then each of the six adapter launches of one block
(the three kernel families of csrc/lora.hip, forward and backward layouts) is timed on its own — back-to-back launches between two events — and
printed beside the bytes it has to move:  project reads T*K*2,  expand-add moves 2*T*N*2,  the weight gradient reads T*(P+Q)*2.
Needs the GPU; there is no CPU fallback."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, H, L, NH = 250880, 1024, 24, 16


def build_model(device, compute_dtype):
    from cleantransformer_amd.models.modeling_bloom import BloomConfig, BloomForCausalLM
    cfg = BloomConfig(vocab_size=V, hidden_size=H, n_layer=L, num_attention_heads=NH, compute_dtype=compute_dtype)
    with torch.device("meta"):
        m = BloomForCausalLM(cfg)
    m = m.to_empty(device=device)
    m._tie_weight()
    g = torch.Generator(device=device).manual_seed(1234)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() > 1:
                p.normal_(0.0, 0.02, generator=g)
            elif n.endswith("layernorm.weight") or n.endswith("ln_f.weight"):
                p.fill_(1.0)
            else:
                p.zero_()
    return m.train()


def kernel_table(T, r, reps, dev):
    """[(name, shape text, bytes, microseconds per launch)] for the six adapter launches of one block at r on query_key_value"""
    from cleantransformer_amd import ops
    bf = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev).to(bf)  # noqa: E731
    K, N = H, 3 * H
    x, y, dy, dx = rnd(T, K), rnd(T, N), rnd(T, N), rnd(T, K)
    a, b, xa = rnd(r, K), rnd(N, r), rnd(T, r)
    o = torch.empty((T, r), dtype=bf, device=dev)
    cases = [
        ("project      fwd  x A^T      ", f"[{T},{K}] x [{r},{K}]^T", T * K * 2, lambda: ops.lora_project(x, a, False, out=o)),
        ("expand-add   fwd  qkv += xa B^T", f"[{T},{N}] += [{T},{r}] [{N},{r}]^T", 2 * T * N * 2, lambda: ops.lora_expand_add(xa, b, y, False)),
        ("project      bwd  dqkv B     ", f"[{T},{N}] x [{N},{r}]", T * N * 2, lambda: ops.lora_project(dy, b, True, out=o)),
        ("weight grad  dB = dqkv^T xa  ", f"[{T},{N}]^T [{T},{r}]", T * (N + r) * 2, lambda: ops.lora_wgrad(dy, xa)),
        ("weight grad  dA = dxa^T x    ", f"[{T},{r}]^T [{T},{K}]", T * (r + K) * 2, lambda: ops.lora_wgrad(xa, x)),
        ("expand-add   bwd  dx += dxa A", f"[{T},{K}] += [{T},{r}] [{r},{K}]", 2 * T * K * 2, lambda: ops.lora_expand_add(xa, a, dx, True)),
    ]
    rows = []
    for name, shape, nbytes, fn in cases:
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        rows.append((name, shape, nbytes, e0.elapsed_time(e1) * 1e3 / reps))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_step.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora.py needs an MI355X: nothing here is measured on a CPU")
    from cleantransformer_amd.lora import LoraConfig, apply_lora
    from cleantransformer_amd.optimizer import AdamW
    dev = torch.device("cuda:0")
    B, S = args.batch, args.seq
    ids = torch.randint(0, V, (B, S), generator=torch.Generator(device=dev).manual_seed(99), device=dev)
    am = torch.ones((B, S), dtype=torch.long, device=dev)
    labels = ids.clone()

    runs = {}
    for name in ("full", "lora"):
        m = build_model(dev, "bf16")
        if name == "lora":
            apply_lora(m, LoraConfig(r=args.rank, lora_alpha=2 * args.rank, target_modules=("query_key_value",)))
        opt = AdamW(m.parameters(), lr=1e-5, weight_decay=0.01, decoupled=True)
        runs[name] = (m, opt)

    def steps(name, n):
        m, opt = runs[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(n):
            outputs, _ = m(input_ids=ids, attention_mask=am, labels=labels)
            loss = outputs[0]
            opt.zero_grad()
            loss.backward()
            opt.step()
        e1.record()
        torch.cuda.synchronize(dev)
        val = float(loss.detach())
        if not math.isfinite(val):
            raise SystemExit(f"bench_lora.py: non-finite loss ({val}) in the {name} step: refusing to report a time")
        return e0.elapsed_time(e1) / n, val

    for name in runs:
        steps(name, args.warmup)
    samples = {"full": [], "lora": []}
    last = {}
    for _ in range(args.pairs):
        for name in ("full", "lora"):
            ms, last[name] = steps(name, args.steps)
            samples[name].append(ms)
    med = {k: statistics.median(v) for k, v in samples.items()}
    diffs = [f - a for f, a in zip(samples["full"], samples["lora"])]
    trainable = sum(p.numel() for p in runs["lora"][0].parameters() if p.requires_grad)
    lines = []
    for name, what in (("full", "full fine-tuning step (one-call block path)"), ("lora", f"adapter step, r = {args.rank} on query_key_value")):
        lines.append(json.dumps({"what": what, "model": "bloom-560m", "B": B, "S": S, "dtype": "bf16", "ms_per_step": round(med[name], 3),
                                 "samples_ms": [round(x, 3) for x in samples[name]], "steps_per_sample": args.steps, "loss": round(last[name], 5),
                                 **({"trainable_parameters": trainable} if name == "lora" else {})}))
    rows = kernel_table(B * S, args.rank, args.kernel_reps, dev)
    per_block_us = sum(r[3] for r in rows)
    share = per_block_us * L / (med["lora"] * 1e3)
    txt = [f"# tools/bench_lora.py --pairs {args.pairs} --steps {args.steps} --warmup {args.warmup} (interleaved pairs, medians; {torch.cuda.get_device_name(0)})"]
    txt += lines
    txt.append(f"adapter step below the full step by {med['full'] - med['lora']:.3f} ms ({100 * (1 - med['lora'] / med['full']):.1f} %); "
               f"paired differences min {min(diffs):.3f} / max {max(diffs):.3f} ms")
    txt.append("")
    txt.append(f"# the six adapter launches of one block (T = {B * S}, r = {args.rank}), {args.kernel_reps} back-to-back launches between two events")
    txt.append(f"{'kernel':34s} {'shape':38s} {'MiB':>8s} {'us':>9s} {'GB/s':>8s}")
    for name, shape, nbytes, us in rows:
        txt.append(f"{name:34s} {shape:38s} {nbytes / 2 ** 20:8.1f} {us:9.1f} {nbytes / us / 1e3:8.0f}")
    txt.append(f"per block {per_block_us:.1f} us, x {L} blocks = {per_block_us * L / 1e3:.3f} ms = {100 * share:.1f} % of the adapter step")
    out = "\n".join(txt) + "\n"
    print(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
