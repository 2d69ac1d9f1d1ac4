"""The short-key attention backward (csrc/attn_short.hip) against f64, next to the library's bf16 backward.

Ladder rule: per tensor ``‖native − f64‖ <= c · ‖library − f64‖`` with the library's flash backward on the same
bf16 tensors as the reference point.  Both kernels round P and dS to bf16 once and accumulate in f32, so the ratio sits
near 1; a ratio above 1.5 would be a defect (a mask, delta, the scale), not a constant to record.  ``RATIO_BOUND`` is the
worst ratio measured over all cases and both layouts plus 10 %.

The exactness half: zero pad columns stay exactly zero, two calls and a captured graph's replays give the same bits,
nothing at or past row Sk / Sq is read (NaN tails), and the launch's footprint (guards around dq, dk, dv and the workspace,
poisoned inputs) — registered as the footprint case of ``lora_amd_attn_short_bwd`` with tests/test_gpu_footprint.py's
registry, which tests/test_capi_cpu.py reads.
"""
from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

from lora_amd import _C
from tests import memguard as MG
from tests import test_gpu_footprint as FP

DEV = "cuda:0"
BF = torch.bfloat16

# (Sq, Sk, D, B, H, true head size): what each exercises is in the id
CASES = {
    "one_full_block": (64, 77, 64, 1, 2, 64),
    "ragged_tail": (80, 77, 64, 1, 2, 64),
    "several_blocks_several_slabs": (327, 77, 64, 3, 1, 64),
    "half_k_step": (100, 77, 80, 1, 2, 80),
    "widest_head": (70, 77, 160, 1, 2, 160),
    "no_masked_key": (64, 80, 64, 1, 2, 64),
    "mostly_masked_tiles": (64, 7, 64, 1, 2, 64),
    "one_key": (33, 1, 64, 1, 2, 64),
    "padded_head_40_in_64": (80, 77, 64, 2, 2, 40),
}
LAYOUTS = ("bhsd", "bshd")

# worst ‖native − f64‖ / ‖library − f64‖ over CASES x LAYOUTS, measured on MI355X (first GPU visit): dq 0.991
# (one_full_block), dk 0.992 (ragged_tail, padded_head_40_in_64), dv 1.000 (1.0632e-01 against 1.0631e-01,
# several_blocks_several_slabs); the lowest: 0.85 with 7 keys; one key: dq = dk = 0 exactly.  Bound = measured + 10 %
RATIO_BOUND = {"dq": 1.09, "dk": 1.09, "dv": 1.10}


def _lay(t: torch.Tensor, layout: str) -> torch.Tensor:
    """``t`` [B, H, S, D] as contiguous memory of that shape, or as the transposed view of [B, S, H, D] memory."""
    if layout == "bhsd":
        return t.contiguous()
    return t.transpose(1, 2).contiguous().transpose(1, 2)


@functools.lru_cache(maxsize=None)
def _problem(name: str):
    """bf16 q, k, v, dO of a case (seeded), the f64 gradients on the same values and the library's bf16 gradients."""
    Sq, Sk, D, B, H, d = CASES[name]
    g = torch.Generator().manual_seed(1234 + sorted(CASES).index(name))
    q, k, v, go = (torch.randn(B, H, S, D, generator=g).to(BF).to(DEV) for S in (Sq, Sk, Sk, Sq))
    if d < D:  # the head-padded operands of the step: pad columns of q, k (and v, dO) are zeros
        for t in (q, k, v, go):
            t[..., d:] = 0
    scale = d ** -0.5
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    p = torch.softmax(scale * q64 @ k64.transpose(-1, -2), dim=-1)
    (p @ v64).backward(go.double())
    ref = {"dq": q64.grad, "dk": k64.grad, "dv": v64.grad}
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    F.scaled_dot_product_attention(ql, kl, vl, scale=scale).backward(go)
    lib = {"dq": ql.grad, "dk": kl.grad, "dv": vl.grad}
    return (q, k, v, go), scale, ref, lib


def _native(name: str, layout: str, **kw):
    (q, k, v, go), scale, _, _ = _problem(name)
    return _C.attn_short_bwd(*(_lay(t, layout) for t in (q, k, v, go)), scale, **kw)


def _err(x: torch.Tensor, ref: torch.Tensor) -> float:
    return float((x.double() - ref).norm())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_gradients_within_the_library_error_against_f64(name, layout):
    Sq, Sk, D, B, H, d = CASES[name]
    if name == "several_blocks_several_slabs":
        run, slabs, _, _ = _C.attn_short_bwd_plan(B, H, Sq, Sk, D)
        assert run >= 2 and slabs >= 2, f"the case must walk several blocks and fold several slabs: run {run}, slabs {slabs}"
    _, _, ref, lib = _problem(name)
    got = dict(zip(("dq", "dk", "dv"), _native(name, layout)))
    for t in ("dq", "dk", "dv"):
        assert got[t].dtype == BF and got[t].shape == ref[t].shape
        assert bool(torch.isfinite(got[t]).all()), f"{name} {layout} {t}: non-finite values"
        e_nat, e_lib, size = _err(got[t], ref[t]), _err(lib[t], ref[t]), float(ref[t].norm())
        print(f"[attn_short] {name:30s} {layout} {t}: native {e_nat:.4e} library {e_lib:.4e} "
              f"ratio {e_nat / e_lib if e_lib else float('nan'):.3f} (‖f64‖ {size:.3e})")
        assert e_nat <= RATIO_BOUND[t] * e_lib, \
            f"{name} {layout} {t}: ‖native − f64‖ {e_nat:.4e} > {RATIO_BOUND[t]} x ‖library − f64‖ {e_lib:.4e}"


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_without_key_value_gradients_dq_is_the_same_bits(layout):
    dq, dk, dv = _native("ragged_tail", layout)
    dq2, dk2, dv2 = _native("ragged_tail", layout, need_kv=False)
    assert dk2 is None and dv2 is None and torch.equal(dq, dq2)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_zero_pad_columns_give_exactly_zero_pad_gradients(layout):
    """True head size 40 inside D = 64: the pad columns of dQ and dK are sums of exact zeros."""
    dq, dk, _ = _native("padded_head_40_in_64", layout)
    assert int((dq[..., 40:] != 0).sum()) == 0 and int((dk[..., 40:] != 0).sum()) == 0
    assert float(dq[..., :40].abs().max()) > 0 and float(dk[..., :40].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["several_blocks_several_slabs", "widest_head"])
def test_two_calls_and_graph_replays_give_the_same_bits(name):
    (q, k, v, go), scale, _, _ = _problem(name)
    first = _C.attn_short_bwd(q, k, v, go, scale)
    second = _C.attn_short_bwd(q, k, v, go, scale)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    B, H, Sq, D = q.shape
    ws = torch.empty(_C.attn_short_bwd_plan(B, H, Sq, k.shape[2], D)[3], dtype=torch.uint8, device=DEV)
    outs = [torch.empty_like(t) for t in (q, k, v)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _C.attn_short_bwd(q, k, v, go, scale, dq=outs[0], dk=outs[1], dv=outs[2], workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _C.attn_short_bwd(q, k, v, go, scale, dq=outs[0], dk=outs[1], dv=outs[2], workspace=ws)
    for _ in range(3):
        for o in outs:
            o.fill_(float("nan"))
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, outs):
            assert torch.equal(a, b), "a replay differs from the eager launch"


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["kv", "q_dout"])
@pytest.mark.parametrize("name", ["ragged_tail", "half_k_step", "one_key"])
def test_nothing_past_the_last_row_is_read(name, which):
    """Operands as leading slices of larger buffers whose tails hold NaN: finite outputs, the bits of a run on clean copies."""
    (q, k, v, go), scale, _, _ = _problem(name)
    clean = _C.attn_short_bwd(q, k, v, go, scale)

    def tailed(t):
        B, H, S, D = t.shape
        big = torch.full((B, H, S + 9, D), float("nan"), dtype=t.dtype, device=DEV)
        big[:, :, :S] = t
        return big[:, :, :S]

    ops = [q, k, v, go]
    for i in ((1, 2) if which == "kv" else (0, 3)):
        ops[i] = tailed(ops[i])
    got = _C.attn_short_bwd(*ops, scale)
    for a, b in zip(clean, got):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b.contiguous())


# ----------------------------------------------------------------------------- footprint
@FP.case("lora_amd_attn_short_bwd")
def case_attn_short_bwd(names=("ragged_tail", "several_blocks_several_slabs", "half_k_step", "widest_head", "one_key")):
    """Guards around dq, dk, dv and the workspace, inputs in the middle of NaN-filled allocations (transposed views of
    [B, S, H, D] memory and contiguous [B, H, S, D]), the written sets, and the values of the unguarded launch bit for bit."""
    for name in names:
        (q, k, v, go), scale, _, _ = _problem(name)
        B, H, Sq, D = q.shape
        Sk = k.shape[2]
        plain = _C.attn_short_bwd(q, k, v, go, scale)
        for layout in LAYOUTS:
            def place(t):
                if layout == "bhsd":
                    return MG.poisoned(t)
                return MG.poisoned(t.transpose(1, 2).contiguous()).transpose(1, 2)

            def guarded(t):
                shape = t.shape if layout == "bhsd" else (t.shape[0], t.shape[2], t.shape[1], t.shape[3])
                gd = MG.Guarded(shape, t.dtype, DEV)
                return gd, (gd.data if layout == "bhsd" else gd.data.transpose(1, 2))

            ins = [place(t) for t in (q, k, v, go)]
            (gq, dq), (gk, dk), (gv, dv) = guarded(q), guarded(k), guarded(v)
            ws_bytes = _C.attn_short_bwd_plan(B, H, Sq, Sk, D)[3]
            gw = MG.Guarded((ws_bytes // 4,), torch.float32, DEV)
            _C.attn_short_bwd(*ins, scale, dq=dq, dk=dk, dv=dv, workspace=gw.data)
            torch.cuda.synchronize()
            what = f"attn_short_bwd {name} {layout}"
            for i, gd in enumerate((gq, gk, gv, gw)):
                gd.check(f"{what} operand {i}")
            for t, want in zip((dq, dk, dv), plain):
                MG.assert_written(t, what)
                assert torch.equal(t, want), f"{what}: values differ from the unguarded launch"
            MG.assert_written(gw.data, what + " workspace")
            # no key / value gradient: dk, dv and the workspace are not touched
            (gq2, dq2) = guarded(q)
            _C.attn_short_bwd(*ins, scale, need_kv=False, dq=dq2)
            torch.cuda.synchronize()
            gq2.check(what + " dq alone")
            assert torch.equal(dq2, plain[0])


@pytest.mark.gpu
def test_footprint_case():
    assert "lora_amd_attn_short_bwd" in FP.covered()
    torch.cuda.synchronize()
    case_attn_short_bwd()
    torch.cuda.synchronize()
