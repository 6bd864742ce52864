"""Single-device adapter fine-tuning: the ft_bloom.py loop (forward -> optimizer.zero_grad() -> loss.backward() -> optimizer.step()) on a model
that carries low-rank adapters (cleantransformer_amd/lora.py).  The base model is frozen; what is saved is the adapter state dict only."""
from __future__ import annotations

import os

import torch

from ..lora import LoraConfig, apply_lora, lora_state_dict
from ..optimizer import AdamW
from .ft_bloom import collate, train_step  # noqa: F401  (same batches, same step)


def train(model, train_loader, epoches, lora_config: LoraConfig = None, save_interval=1000, print_interval=10, save_dir="./", optimizer=None, lr=1e-4):
    """`model`: a BloomForCausalLM with its checkpoint loaded.  Returns the number of steps taken; `adapter_step_<n>.pt` files hold
    lora_state_dict(model) (load them with lora.load_lora_state_dict after apply_lora with the same config; merge_lora() folds them into the base)."""
    device = torch.device("cuda:0")
    model = model.to(device)
    if getattr(model, "_ct_lora", None) is None:
        apply_lora(model, lora_config if lora_config is not None else LoraConfig(r=16, lora_alpha=32, target_modules=("query_key_value",)))
    if optimizer is None:
        # the whole parameter list is fine: the frozen parameters never get a gradient and the fused AdamW skips them
        optimizer = AdamW(model.parameters(), lr=lr, weight_decay=0.01, decoupled=True)
    model.train()
    steps = 0
    os.makedirs(save_dir, exist_ok=True)
    for _ in range(epoches):
        for batch in train_loader:
            batch = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
            loss = train_step(model, batch, optimizer)
            steps += 1
            if steps % print_interval == 0:
                print("step: {}, loss: {}".format(steps, loss.cpu().item()))
            if steps % save_interval == 0:
                torch.save(lora_state_dict(model), os.path.join(save_dir, f"adapter_step_{steps}.pt"))
    torch.save(lora_state_dict(model), os.path.join(save_dir, "adapter_final.pt"))
    return steps
