"""Low-rank adapters (LoRA) for Bloom supervised fine-tuning.

    y = x W^T + b + scaling * (x A^T) B^T          A [r, in], B [out, r], scaling = lora_alpha / r

next to the frozen ``query_key_value`` / ``dense`` / ``dense_4h_to_h`` Linears of every block, with peft's parameter names
(``<linear>.lora_A.weight``, ``<linear>.lora_B.weight``).  The adapters are fp32 master parameters like every other parameter of the package; the
products run on the three kernel families of csrc/lora.hip (project, expand-add, skinny weight gradient) from the per-op block of ``models.modeling_bloom``
(``BloomBlockOpsFn``: one forward and one backward routine shared with the dropout path; KV-cache decode calls the same forward routine), whose backward
launches nothing for a frozen parameter.

    model = apply_lora(model, LoraConfig(r=16, lora_alpha=32))
    optimizer = AdamW(model.parameters(), ...)          # parameters without a gradient are skipped
    ...
    torch.save(lora_state_dict(model), "adapter.pt")
    merge_lora(model)                                   # W += scaling * B @ A; the model is a plain Bloom again (one-call block path)

Out of scope (each raises where a wrong result would otherwise be silent): GPT models, ``DistributedDataParallel`` around an adapted model, adapter
dropout, ``dense_h_to_4h`` adapters (its GELU is fused into the GEMM epilogue), block dropout together with adapters; ``GraphedStep`` runs an adapted
model eagerly (``fallback_reason`` says so); the Trainer's checkpoints do not know adapters beyond ``lora_state_dict`` / ``load_lora_state_dict``.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Iterable, Tuple

import torch

TARGETS = ("query_key_value", "dense", "dense_4h_to_h")


class LoraConfig:
    def __init__(self, r: int = 8, lora_alpha: float = 16, target_modules: Iterable[str] = ("query_key_value",), lora_dropout: float = 0.0):
        if isinstance(target_modules, str):
            target_modules = (target_modules,)
        target_modules = tuple(target_modules)
        if not isinstance(r, int) or isinstance(r, bool) or r < 8 or r > 64 or r % 8 != 0:
            raise ValueError(f"LoraConfig: r = {r!r}; the low-rank kernels take a multiple of 8 with 8 <= r <= 64")
        if "dense_h_to_4h" in target_modules:
            raise NotImplementedError("LoraConfig: dense_h_to_4h cannot carry an adapter: its GELU is fused into the GEMM epilogue, so an adapter there "
                                      "needs an un-fused activation")
        unknown = [t for t in target_modules if t not in TARGETS]
        if unknown or not target_modules or len(set(target_modules)) != len(target_modules):
            raise ValueError(f"LoraConfig: target_modules = {target_modules!r}; a non-empty subset of {TARGETS}")
        if lora_dropout > 0:
            raise NotImplementedError("LoraConfig: adapter dropout (lora_dropout > 0) is not implemented")
        if lora_dropout < 0:
            raise ValueError(f"LoraConfig: lora_dropout = {lora_dropout!r}")
        self.r = r
        self.lora_alpha = lora_alpha
        self.target_modules = target_modules
        self.lora_dropout = float(lora_dropout)

    @property
    def scaling(self) -> float:
        return float(self.lora_alpha) / self.r


def _is_bloom(model) -> bool:
    from .models.modeling_bloom import BloomForCausalLM
    return isinstance(model, BloomForCausalLM)


def _linears(model, targets) -> "list[Tuple[str, torch.nn.Linear]]":
    out = []
    for i, blk in enumerate(model.bloom.blocks):
        for t in TARGETS:                                                   # module order, whatever order the config names them in
            if t in targets:
                owner, path = (blk.mlp, "mlp") if t == "dense_4h_to_h" else (blk.self_attention, "self_attention")
                out.append((f"bloom.blocks.{i}.{path}.{t}", getattr(owner, t)))
    return out


def _adapted(model) -> "list[Tuple[str, torch.nn.Linear]]":
    return [(n, lin) for n, lin in _linears(model, TARGETS) if hasattr(lin, "lora_A")]


def apply_lora(model, config: LoraConfig):
    """Freeze `model` and give every targeted Linear of every block its two adapter parameters (A: kaiming-uniform from torch's generator, B: zeros,
    so the adapted model starts out equal to the base model)."""
    if not _is_bloom(model):
        raise TypeError("apply_lora: adapters are implemented for BloomForCausalLM only (GPT models are out of scope)")
    if getattr(model, "_ct_lora", None) is not None:
        raise RuntimeError("apply_lora: this model already carries adapters (merge_lora() first)")
    for p in model.parameters():
        p.requires_grad_(False)
    for _, lin in _linears(model, config.target_modules):
        w = lin.weight
        a = torch.nn.Linear(lin.in_features, config.r, bias=False, device=w.device, dtype=torch.float32)
        b = torch.nn.Linear(config.r, lin.out_features, bias=False, device=w.device, dtype=torch.float32)
        with torch.no_grad():
            torch.nn.init.kaiming_uniform_(a.weight, a=math.sqrt(5))
            b.weight.zero_()
        lin.lora_A, lin.lora_B = a, b
        lin.lora_scaling = config.scaling
    model._ct_lora = config
    return model


def lora_state_dict(model) -> "OrderedDict[str, torch.Tensor]":
    """The adapter tensors only, under their state_dict keys."""
    out = OrderedDict()
    for name, lin in _adapted(model):
        out[name + ".lora_A.weight"] = lin.lora_A.weight.detach().clone()
        out[name + ".lora_B.weight"] = lin.lora_B.weight.detach().clone()
    return out


def load_lora_state_dict(model, sd, strict: bool = True):
    """Copy adapter tensors into an adapted model.  Returns (missing, unexpected); with strict=True either raises."""
    from . import ops
    own = OrderedDict()
    for name, lin in _adapted(model):
        own[name + ".lora_A.weight"] = lin.lora_A.weight
        own[name + ".lora_B.weight"] = lin.lora_B.weight
    missing = [k for k in own if k not in sd]
    unexpected = [k for k in sd if k not in own]
    if strict and (missing or unexpected):
        raise KeyError(f"load_lora_state_dict: missing {missing}, unexpected {unexpected}")
    with torch.no_grad():
        for k, p in own.items():
            if k in sd:
                if tuple(sd[k].shape) != tuple(p.shape):
                    raise ValueError(f"load_lora_state_dict: {k} has shape {tuple(sd[k].shape)}, the model's is {tuple(p.shape)}")
                p.copy_(sd[k])
                ops.invalidate_compute_copies(p)
    return missing, unexpected


def merge_lora(model):
    """W += scaling * B @ A on the fp32 master weights; the adapters are removed and every parameter is trainable again."""
    from . import ops
    if getattr(model, "_ct_lora", None) is None:
        raise RuntimeError("merge_lora: this model carries no adapters")
    with torch.no_grad():
        for _, lin in _adapted(model):
            lin.weight.addmm_(lin.lora_B.weight, lin.lora_A.weight, alpha=float(lin.lora_scaling))
            ops.invalidate_compute_copies(lin.weight)
            del lin.lora_A, lin.lora_B, lin.lora_scaling
    model._ct_lora = None
    for p in model.parameters():
        p.requires_grad_(True)
    return model
