"""Routing of the short-key attention backward: what ``lora_amd_attn_short_bwd_supported`` / ``..._plan`` accept (pure host),
and the stand-in's CrossAttention with ``ops.ATTN_SHORT_BWD`` on and off — same forward bits, gradients within the library's
own error against an f64 run of the module, and the library's backward wherever the kernel does not take the problem."""
from __future__ import annotations

import copy
import ctypes as C

import pytest
import torch

from lora_amd import _C, ops
from lora_amd.standin import attention
from lora_amd.standin.unet import CrossAttention
from tests import test_gpu_attn_short_bwd as K  # the kernel's cases (and its footprint case, registered on import)

BF = torch.bfloat16
DEV = "cuda:0"

# worst ‖on − f64‖ / ‖off − f64‖ over the module's input and parameter gradients, measured on MI355X (first GPU visit):
# 1.005 (to_k.weight; context 1.002, x 0.997, to_q.weight 0.995, to_v / to_out 1.000); bound = measured + 10 %
MODULE_RATIO_BOUND = 1.11


def _strides(*triples):
    flat = [s for t in triples for s in t]
    return (C.c_int64 * len(flat))(*flat), len(flat)


def test_supported_accepts_the_tested_shapes_and_refuses_the_rest():
    lib = _C.require()
    ok = lib.lora_amd_attn_short_bwd_supported
    for Sq, Sk, D, B, H, _ in K.CASES.values():
        dense, n = _strides((H * Sq * D, Sq * D, D), (H * Sk * D, Sk * D, D))     # [B, H, S, D]
        heads, _ = _strides((Sq * H * D, D, H * D), (Sk * H * D, D, H * D))        # [B, S, H, D] transposed
        assert ok(Sq, Sk, D, _C.BF16, dense, n) == 1 and ok(Sq, Sk, D, _C.BF16, heads, n) == 1, (Sq, Sk, D)
    for Sq, Sk, D in [(4096, 77, 64), (1024, 77, 80), (256, 77, 160), (64, 77, 160)]:  # the timed step's cross-attention
        assert ok(Sq, Sk, D, _C.BF16, None, 0) == 1
    assert ok(64, 81, 64, _C.BF16, None, 0) == 0 and ok(64, 0, 64, _C.BF16, None, 0) == 0
    assert ok(64, 77, 40, _C.BF16, None, 0) == 0 and ok(64, 77, 72, _C.BF16, None, 0) == 0
    assert ok(64, 77, 64, _C.F32, None, 0) == 0 and ok(64, 77, 64, _C.F16, None, 0) == 0
    bad, n = _strides((2 * 64 * 64, 64 * 64, 68))   # rows 136 bytes apart: not 16-byte aligned
    assert ok(64, 77, 64, _C.BF16, bad, n) == 0
    # the same through the tensor-level wrapper
    q = torch.zeros(1, 2, 64, 64, dtype=BF)
    assert _C.attn_short_bwd_supported(64, 77, 64, BF, q, q.transpose(1, 2).contiguous().transpose(1, 2))
    assert not _C.attn_short_bwd_supported(64, 77, 64, BF, torch.zeros(1, 2, 64, 68, dtype=BF)[..., :64])
    assert not _C.attn_short_bwd_supported(64, 77, 64, torch.float32, q.float())


def test_plan_slabs_times_slab_bytes_is_the_workspace():
    lib = _C.require()
    for B, H, Sq, Sk, D in [(4, 8, 4096, 77, 64), (4, 8, 1024, 77, 80), (4, 8, 256, 77, 160), (4, 8, 64, 77, 160),
                            (3, 1, 327, 77, 64), (1, 2, 33, 1, 64), (1, 1, 1, 80, 128)]:
        run, slabs, slab_bytes, ws = _C.attn_short_bwd_plan(B, H, Sq, Sk, D)
        nblk = -(-Sq // 64)
        assert slab_bytes == 2 * 80 * D * 4 and ws == B * H * slabs * slab_bytes
        assert 1 <= run <= nblk and slabs == -(-nblk // run) and (slabs - 1) * run < nblk
    assert _C.attn_short_bwd_plan(4, 8, 4096, 77, 64)[:2] == (8, 8)     # one workgroup per CU, slabs 10 MB against 50 MB of rows
    assert _C.attn_short_bwd_plan(3, 1, 327, 77, 64)[:2] == (4, 2)
    plan = _C.AttnShortPlan()
    assert lib.lora_amd_attn_short_bwd_plan(4, 8, 4096, 81, 64, C.byref(plan)) == -5
    assert b"Sk = 81" in lib.lora_amd_last_error()


def test_the_switch_is_a_module_constant_of_the_ab_spec():
    assert isinstance(ops.ATTN_SHORT_BWD, bool)
    assert ops.apply_ab_overrides("ATTN_SHORT_BWD=0", {}) == {"ATTN_SHORT_BWD": False}


# ----------------------------------------------------------------------------- the module, on the GPU
def _module_run(mod, x, ctx, gy):
    x, ctx = x.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    mod.zero_grad(set_to_none=True)
    y = mod(x, ctx)
    y.backward(gy)
    grads = {"x": x.grad, "context": ctx.grad}
    grads.update({n: p.grad for n, p in mod.named_parameters()})
    return y.detach(), grads


def _with_choice(keys, fn):
    """Run ``fn`` with the attention kernel of ``keys`` pinned to the head size padded to 64 (no timing pass)."""
    for key in keys:
        dict.__setitem__(attention._CHOICE, key, ["EFFICIENT_ATTENTION", 64])
    try:
        return fn()
    finally:
        for key in keys:
            dict.pop(attention._CHOICE, key, None)


@pytest.fixture
def switch():
    saved = ops.ATTN_SHORT_BWD
    yield lambda on: setattr(ops, "ATTN_SHORT_BWD", on)
    ops.ATTN_SHORT_BWD = saved


@pytest.mark.gpu
def test_cross_attention_same_forward_bits_and_gradients_within_the_library_error(switch):
    torch.manual_seed(7)
    B, T, Sk = 2, 100, 77
    mod = CrossAttention(64, 48, heads=2, dim_head=32).to(DEV).to(BF)
    x, ctx = torch.randn(B, T, 64, device=DEV).to(BF), torch.randn(B, Sk, 48, device=DEV).to(BF)
    gy = torch.randn(B, T, 64, device=DEV).to(BF)
    keys = [repr((B, 2, T, Sk, 32, str(BF), True))]
    runs = {}
    for on in (True, False):
        switch(on)
        before = dict(attention.ROUTES)
        runs[on] = _with_choice(keys, lambda: _module_run(mod, x, ctx, gy))
        took = {k: attention.ROUTES[k] - before[k] for k in before}
        assert took == ({"native_bwd": 1, "library": 0} if on else {"native_bwd": 0, "library": 1}), took
    assert torch.equal(runs[True][0], runs[False][0]), "the forward output changed with the backward's route"
    mod64 = copy.deepcopy(mod).double()
    _, ref = _module_run(mod64, x.double(), ctx.double(), gy.double())
    worst = 0.0
    for name in sorted(ref):
        e_on = float((runs[True][1][name].double() - ref[name]).norm())
        e_off = float((runs[False][1][name].double() - ref[name]).norm())
        print(f"[attn_short route] {name:20s} on {e_on:.4e} off {e_off:.4e} ratio {e_on / e_off:.3f}")
        worst = max(worst, e_on / e_off)
        assert e_on <= MODULE_RATIO_BOUND * e_off, f"{name}: ‖on − f64‖ {e_on:.4e} > {MODULE_RATIO_BOUND} x ‖off − f64‖ {e_off:.4e}"
    print(f"[attn_short route] worst ratio {worst:.3f}")


@pytest.mark.gpu
def test_more_than_80_keys_take_the_library_backward(switch):
    switch(True)
    torch.manual_seed(8)
    B, T, Sk = 2, 100, 81
    mod = CrossAttention(64, 48, heads=2, dim_head=32).to(DEV).to(BF)
    x, ctx = torch.randn(B, T, 64, device=DEV).to(BF), torch.randn(B, Sk, 48, device=DEV).to(BF)
    before = dict(attention.ROUTES)
    _, grads = _with_choice([repr((B, 2, T, Sk, 32, str(BF), True))],
                            lambda: _module_run(mod, x, ctx, torch.randn(B, T, 64, device=DEV).to(BF)))
    assert attention.ROUTES["library"] == before["library"] + 1 and attention.ROUTES["native_bwd"] == before["native_bwd"]
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
