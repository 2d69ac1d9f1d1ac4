"""Routing of the ResNet glue in the stand-in UNet: the one-launch time-embedding addends (``ops.TEMB_ONE_LAUNCH``) against
the per-block twin.

On CPU the switch falls back to the ATen sequence in the same operation order: bit-equal output and input gradient, with and
without gradient checkpointing.  On the GPU (channels_last bf16) the switch changes roundings only: output and LoRA gradients
inside the bf16 bound of tests/test_gpu_hostops.py, one temb launch per forward covering every block, and a trained
``time_emb_proj`` keeps the per-block path and receives its gradient.
"""
from __future__ import annotations

import pytest
import torch
import torch.nn as nn

import lora_amd as L
from lora_amd import _C, ops
from lora_amd.standin import tiny_unet

DEV = "cuda:0"


def _switch(monkeypatch, temb: bool):
    monkeypatch.setattr(ops, "TEMB_ONE_LAUNCH", temb)


@pytest.mark.parametrize("ckpt", [False, True])
def test_cpu_the_switch_falls_back_bit_for_bit(monkeypatch, ckpt):
    torch.manual_seed(0)
    unet = tiny_unet()
    if ckpt:
        unet.enable_gradient_checkpointing()
        unet.train()
    lat = torch.randn(2, 4, 16, 16, requires_grad=True)
    ctx, t = torch.randn(2, 7, 32), torch.tensor([10, 500])

    def run(on):
        _switch(monkeypatch, on)
        y = unet(lat, t, ctx).sample
        (g,) = torch.autograd.grad(y.square().sum(), lat)
        return y.detach(), g

    y1, g1 = run(True)
    assert unet._temb_table is None
    y0, g0 = run(False)
    assert torch.equal(y1, y0) and torch.equal(g1, g0)


def _gpu_unet():
    torch.manual_seed(0)
    unet = tiny_unet().to(DEV).to(torch.bfloat16)
    unet.requires_grad_(False)
    L.inject_trainable_lora(unet, r=4)
    for m in unet.modules():
        if isinstance(m, L.LoraInjectedLinear):
            nn.init.normal_(m.lora_up.weight, std=0.05)
    unet.to(memory_format=torch.channels_last)
    lat = torch.randn(2, 4, 16, 16, device=DEV, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    ctx = torch.randn(2, 7, 32, device=DEV, dtype=torch.bfloat16)
    return unet, lat, ctx, torch.tensor([10, 500], device=DEV)


def _step(unet, lat, t, ctx):
    for p in unet.parameters():
        p.grad = None
    y = unet(lat, t, ctx).sample
    y.float().pow(2).mean().backward()
    grads = torch.cat([p.grad.flatten().float() for p in unet.parameters() if p.requires_grad])
    return y.detach().float(), grads


def _counted(monkeypatch, name):
    calls, real = [], getattr(_C, name)

    def wrapper(*a, **k):
        calls.append(name)
        return real(*a, **k)

    monkeypatch.setattr(_C, name, wrapper)
    return calls


@pytest.mark.gpu
def test_gpu_switch_on_against_off(monkeypatch):
    from tests.test_gpu_hostops import _close

    unet, lat, ctx, t = _gpu_unet()
    temb_calls = _counted(monkeypatch, "temb_addends")
    _switch(monkeypatch, True)
    y1, g1 = _step(unet, lat, t, ctx)
    n_res = sum(1 for m in unet.modules() if type(m).__name__ == "ResnetBlock2D")
    assert len(temb_calls) == 1 and len(unet._temb_table.widths) == n_res
    _switch(monkeypatch, False)
    y0, g0 = _step(unet, lat, t, ctx)
    assert len(temb_calls) == 1
    print(f"output: max |on - off| = {float((y1 - y0).abs().max()):.3e} of {float(y0.abs().max()):.3e}; "
          f"gradients: {float((g1 - g0).abs().max()):.3e} of {float(g0.abs().max()):.3e}")
    _close(y1, y0, torch.bfloat16, scale=float(y0.abs().max()), msg="UNet output, switch on against off")
    _close(g1, g0, torch.bfloat16, scale=float(g0.abs().max()), msg="LoRA gradients, switch on against off")


@pytest.mark.gpu
def test_gpu_trained_time_projection_keeps_the_per_block_path(monkeypatch):
    unet, lat, ctx, t = _gpu_unet()
    _switch(monkeypatch, True)
    blocks = [m for m in unet.modules() if type(m).__name__ == "ResnetBlock2D"]
    blocks[0].time_emb_proj.weight.requires_grad_(True)
    _step(unet, lat, t, ctx)
    g = blocks[0].time_emb_proj.weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert len(unet._temb_table.widths) == len(blocks) - 1  # every other block stays in the one launch
