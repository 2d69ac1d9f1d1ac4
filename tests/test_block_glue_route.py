"""Routing of the block glue in the stand-in UNet: the one-launch ResnetBlock2D tail (``ops.RESNET_TAIL``) and the norm forks
that add a second input gradient inside the norm's backward launch (``ops.NORM_FORK``), each against its twin.

On CPU both switches fall back to the ATen sequence in the same operation order: bit-equal output and input gradient, with
and without gradient checkpointing.  On the GPU (channels_last bf16, LoRA injected as tests/test_resnet_glue_route.py sets it
up) the tail reproduces the roundings of the adds it replaces, so the UNet output is bit-equal with RESNET_TAIL alone; the
LayerNorm fork rounds once where the separate add rounds twice, so with both switches output and LoRA gradients are held to
the bf16 bound of tests/test_gpu_hostops.py.  Call counts pin the routing: one tail per ResnetBlock2D, gsum in one GroupNorm
backward per ResnetBlock2D and Transformer2DModel, one add_layernorm_bwd more per transformer block (the latents take a
gradient in that test, so that the first block has a backward to count).  A convolution with a trained bias, or with a hook
on it, is called as the module it is.
"""
from __future__ import annotations

import pytest
import torch

from lora_amd import _C, ops
from lora_amd.standin import tiny_unet
from tests.test_resnet_glue_route import _gpu_unet, _step


def _switch(monkeypatch, tail: bool, fork: bool):
    monkeypatch.setattr(ops, "RESNET_TAIL", tail)
    monkeypatch.setattr(ops, "NORM_FORK", fork)


def test_switches_default_on_and_belong_to_the_ab_mechanism():
    assert ops.RESNET_TAIL is True and ops.NORM_FORK is True
    ns = {}
    assert ops.apply_ab_overrides("RESNET_TAIL=0,NORM_FORK=0", ns) == {"RESNET_TAIL": False, "NORM_FORK": False}
    assert ops.apply_ab_overrides("RESNET_TAIL=1", {}) == {"RESNET_TAIL": True}


@pytest.mark.parametrize("ckpt", [False, True])
@pytest.mark.parametrize("tail,fork", [(True, False), (False, True), (True, True)])
def test_cpu_the_switches_fall_back_bit_for_bit(monkeypatch, ckpt, tail, fork):
    torch.manual_seed(0)
    unet = tiny_unet()
    if ckpt:
        unet.enable_gradient_checkpointing()
        unet.train()
    lat = torch.randn(2, 4, 16, 16, requires_grad=True)
    ctx, t = torch.randn(2, 7, 32), torch.tensor([10, 500])

    def run(tail_, fork_):
        _switch(monkeypatch, tail_, fork_)
        y = unet(lat, t, ctx).sample
        (g,) = torch.autograd.grad(y.square().sum(), lat)
        return y.detach(), g

    y1, g1 = run(tail, fork)
    y0, g0 = run(False, False)
    assert torch.equal(y1, y0) and torch.equal(g1, g0)


def _counted(monkeypatch, name, pick=lambda a, k: True):
    calls, real = [], getattr(_C, name)

    def wrapper(*a, **k):
        if pick(a, k):
            calls.append(name)
        return real(*a, **k)

    monkeypatch.setattr(_C, name, wrapper)
    return calls


def _blocks(unet, cls):
    return [m for m in unet.modules() if type(m).__name__ == cls]


@pytest.mark.gpu
def test_gpu_resnet_tail_alone_is_bit_equal(monkeypatch):
    """The library's 1x1 convolution of the shortcut is not bit-reproducible from call to call under its default solver
    choice (one element of a [2, 64, 16, 16] output changed in 2 of 20 repeats on the same input, and the whole step has
    two outcomes whatever the switch says), so both settings run with the library's deterministic solvers requested: the
    comparison is of the tail against the adds, not of one library call against the next."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    unet, lat, ctx, t = _gpu_unet()
    tails = _counted(monkeypatch, "resnet_tail")
    _switch(monkeypatch, True, False)
    y1, g1 = _step(unet, lat, t, ctx)
    assert len(tails) == len(_blocks(unet, "ResnetBlock2D"))
    _switch(monkeypatch, False, False)
    y0, g0 = _step(unet, lat, t, ctx)
    assert len(tails) == len(_blocks(unet, "ResnetBlock2D"))
    _switch(monkeypatch, True, False)
    y2, g2 = _step(unet, lat, t, ctx)
    assert torch.equal(y1, y0), f"UNet output: {int((y1 != y0).sum())} of {y0.numel()} elements differ"
    assert torch.equal(g1, g0), "LoRA gradients"
    assert torch.equal(y2, y0) and torch.equal(g2, g0), "the second run with the tail"


@pytest.mark.gpu
@pytest.mark.parametrize("ckpt", [False, True])
def test_gpu_both_switches_on_against_off(monkeypatch, ckpt):
    from tests.test_gpu_hostops import _close

    unet, lat, ctx, t = _gpu_unet()
    if ckpt:
        unet.enable_gradient_checkpointing()
        unet.train()
    _switch(monkeypatch, True, True)
    y1, g1 = _step(unet, lat, t, ctx)
    _switch(monkeypatch, False, False)
    y0, g0 = _step(unet, lat, t, ctx)
    print(f"output: max |on - off| = {float((y1 - y0).abs().max()):.3e} of {float(y0.abs().max()):.3e}; "
          f"gradients: {float((g1 - g0).abs().max()):.3e} of {float(g0.abs().max()):.3e}")
    _close(y1, y0, torch.bfloat16, scale=float(y0.abs().max()), msg="UNet output, switches on against off")
    _close(g1, g0, torch.bfloat16, scale=float(g0.abs().max()), msg="LoRA gradients, switches on against off")


@pytest.mark.gpu
def test_gpu_call_counts(monkeypatch):
    unet, lat, ctx, t = _gpu_unet()
    lat = lat.clone(memory_format=torch.preserve_format).requires_grad_(True)  # the first block gets a backward as well
    n_res, n_t2d = len(_blocks(unet, "ResnetBlock2D")), len(_blocks(unet, "Transformer2DModel"))
    n_tb = len(_blocks(unet, "BasicTransformerBlock"))
    assert n_res and n_t2d and n_tb
    tails = _counted(monkeypatch, "resnet_tail")
    gsums = _counted(monkeypatch, "groupnorm_nhwc_bwd", lambda a, k: (a[6] if len(a) > 6 else k.get("gsum")) is not None)
    lnb = _counted(monkeypatch, "add_layernorm_bwd")
    _switch(monkeypatch, False, False)
    _step(unet, lat, t, ctx)
    assert len(tails) == 0 and len(gsums) == 0
    ln_off = len(lnb)
    del lnb[:]
    _switch(monkeypatch, True, True)
    _step(unet, lat, t, ctx)
    assert len(tails) == n_res, f"{len(tails)} tail launches for {n_res} blocks"
    assert len(gsums) == n_res + n_t2d, f"gsum in {len(gsums)} GroupNorm backward calls, expected {n_res + n_t2d}"
    assert len(lnb) == ln_off + n_tb, f"{len(lnb)} add_layernorm_bwd calls, {ln_off} without the fork, {n_tb} blocks"


@pytest.mark.gpu
def test_gpu_trained_conv2_bias_keeps_the_old_path(monkeypatch):
    unet, lat, ctx, t = _gpu_unet()
    _switch(monkeypatch, True, True)
    blocks = _blocks(unet, "ResnetBlock2D")
    blocks[1].conv2.bias.requires_grad_(True)
    tails = _counted(monkeypatch, "resnet_tail")
    _step(unet, lat, t, ctx)
    g = blocks[1].conv2.bias.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert len(tails) == len(blocks) - 1  # every other block keeps the one launch


@pytest.mark.gpu
def test_gpu_a_hooked_convolution_is_called_as_a_module(monkeypatch):
    unet, lat, ctx, t = _gpu_unet()
    _switch(monkeypatch, True, True)
    blocks = _blocks(unet, "ResnetBlock2D")
    hooked = next(b for b in blocks if b.conv_shortcut is not None)
    seen = []
    handles = [hooked.conv2.register_forward_hook(lambda m, i, o: seen.append("conv2")),
               hooked.conv_shortcut.register_forward_hook(lambda m, i, o: seen.append("conv_shortcut"))]
    tails = _counted(monkeypatch, "resnet_tail")
    with torch.no_grad():
        y1 = unet(lat, t, ctx).sample
    assert sorted(seen) == ["conv2", "conv_shortcut"] and len(tails) == len(blocks) - 1
    for h in handles:
        h.remove()
    with torch.no_grad():
        unet(lat, t, ctx)
    assert len(seen) == 2 and len(tails) == 2 * len(blocks) - 1 and bool(torch.isfinite(y1).all())


@pytest.mark.gpu
def test_gpu_under_capture(monkeypatch):
    """One forward + backward of the frozen tiny_unet (gradient of the latents: every tail and every fork runs, and nothing
    of an adapter's host-side bookkeeping is inside the capture) captured and replayed equals the eager run inside the
    eager run's own repeat spread (with the library's deterministic solvers requested, as above, that spread is zero: the
    replay has to give the eager run's bits)."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    _switch(monkeypatch, True, True)
    torch.manual_seed(0)
    unet = tiny_unet().to("cuda:0").to(torch.bfloat16).requires_grad_(False).to(memory_format=torch.channels_last)
    lat = torch.randn(2, 4, 16, 16, device="cuda:0", dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    lat.requires_grad_(True)
    ctx, t = torch.randn(2, 7, 32, device="cuda:0", dtype=torch.bfloat16), torch.tensor([10, 500], device="cuda:0")
    tails = _counted(monkeypatch, "resnet_tail")

    def step():
        y = unet(lat, t, ctx).sample
        (g,) = torch.autograd.grad(y.float().pow(2).mean(), lat)
        return y.detach(), g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        e1 = [o.clone() for o in step()]
        e2 = [o.clone() for o in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert len(tails) == 2 * len(_blocks(unet, "ResnetBlock2D"))
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        outs = step()
    for o in outs:
        o.zero_()
    gr.replay()
    torch.cuda.synchronize()
    for name, a, b, got in zip(("output", "latent gradient"), e1, e2, outs):
        spread = float((a.float() - b.float()).abs().max())
        diff = float((got.float() - a.float()).abs().max())
        print(f"{name}: eager repeat spread {spread:.3e}, replay against eager {diff:.3e}")
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
        assert diff <= spread, f"{name}: replay differs from eager by {diff:.3e} (eager repeat spread {spread:.3e})"
