"""CPU (no GPU): the per-op block path of models/modeling_bloom.py — adapters and KV-cache decode — on the torch emulation of the kernel
contracts (cpu_kernel_emulation.install).  In fp32 the adapter ops of cleantransformer_amd/ops.py (lora_project / lora_expand_add / lora_wgrad)
go through ops.gemm, which the emulation replaces, so the real autograd node and the real decode path run here.  The oracle, the adapter
values and the tolerances are the ones of tests/test_gpu_lora.py (test_tiny_fp32_matches_the_merged_weight_oracle and
test_greedy_decode_through_the_kv_cache_equals_the_merged_model), imported from there: adapted model == base model with W' = W + scaling * B A.
"""
import pytest
import torch

import cpu_kernel_emulation as emu
from test_gpu_lora import ALL, ALPHA, QKV, R_, TINY, T_, adapter_values, close, tiny_oracle, tiny_shape
from test_host_logic_cpu import build


def adapted(targets, ad):
    from cleantransformer_amd.lora import LoraConfig, apply_lora, load_lora_state_dict
    V, H, L, nh, B, S = tiny_shape()
    m = apply_lora(build(V, H, L, nh), LoraConfig(r=R_, lora_alpha=ALPHA, target_modules=targets))
    load_lora_state_dict(m, ad)
    return m


@pytest.mark.parametrize("targets", [QKV, ALL], ids=["qkv", "all"])
def test_adapter_path_fp32_matches_the_merged_weight_oracle(monkeypatch, targets):
    emu.install(monkeypatch)
    ad, loss_o, logits_o, g_o = tiny_oracle(targets)
    m = adapted(targets, ad)
    ids, am = T_(TINY["ids"]), T_(TINY["mask"])
    (loss, logits, _), _ = m(input_ids=ids, attention_mask=am, labels=ids.clone())
    loss.backward()
    close("loss", loss, loss_o, 1e-5)
    close("logits", logits, logits_o, 1e-4, 2e-6)
    named = dict(m.named_parameters())
    assert set(g_o) == {n for n, p in named.items() if p.requires_grad}
    for n, p in named.items():
        if n in g_o:
            close("grad " + n, p.grad, g_o[n], 2e-4, 2e-7)
        else:
            assert p.grad is None, n                                                  # the base is frozen: nothing was computed for it


def test_greedy_decode_through_the_kv_cache_equals_the_merged_model(monkeypatch):
    from cleantransformer_amd.lora import merge_lora
    emu.install(monkeypatch)
    V, H, L, nh, B, S = tiny_shape()
    # B ten times the size used elsewhere, as in the GPU test: that is what it takes for the merged weights to decode other tokens than the base model
    ad = {k: (v * 10.0 if ".lora_B." in k else v) for k, v in adapter_values(V, H, L, nh, ALL).items()}
    m = adapted(ALL, ad).eval()
    prompt, mask = T_(TINY["greedy_prompt"]), T_(TINY["greedy_mask"])
    cfg = dict(beam_size=1, max_gen_len=6, do_sample=False, end_ids=None, pad_id=3)       # the reference's loop emits max_gen_len + 2 = 8 new tokens
    out_a = m.generate(prompt, attention_mask=mask, generation_configs=cfg)
    assert out_a.shape[-1] == prompt.shape[-1] + 8
    base = build(V, H, L, nh).eval().generate(prompt, attention_mask=mask, generation_configs=cfg)
    out_m = merge_lora(m).eval().generate(prompt, attention_mask=mask, generation_configs=cfg)
    assert torch.equal(out_a, out_m)
    assert not torch.equal(out_a, base)                                               # the adapters do change what is decoded


def test_dropout_together_with_adapters_still_raises(monkeypatch):
    emu.install(monkeypatch)
    V, H, L, nh, B, S = tiny_shape()
    m = adapted(QKV, adapter_values(V, H, L, nh, QKV))
    ids, am = T_(TINY["ids"]), T_(TINY["mask"])
    for blk in m.bloom.blocks:
        blk.hidden_dropout = 0.1
    with pytest.raises(NotImplementedError, match="dropout"):
        m(input_ids=ids, attention_mask=am, labels=ids.clone())
    for blk in m.bloom.blocks:
        blk.hidden_dropout = 0.0
        blk.self_attention.attention_dropout.p = 0.2
    with pytest.raises(NotImplementedError, match="dropout"):
        m(input_ids=ids, attention_mask=am, labels=ids.clone())
