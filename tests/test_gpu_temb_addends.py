"""``lora_amd_temb_addends``: the norm2 addend of every ResnetBlock2D from one ragged launch, against the ATen sequence it
replaces (silu -> F.linear -> + conv bias -> .float()).

Bound.  The kernel reproduces the sequence's roundings (silu rounded to the activation dtype, r1 = rn(dot + bias),
r2 = rn(r1 + conv bias)) but sums the dot product in another order, so a value that sits at a rounding boundary may round
the other way at r1 and again at r2: one unit in the last place each.  For bf16 (8 significand bits) a unit in the last
place of r is at most 2^-7 |r|, hence |out - seq| <= 2^-7 (|r1| + |r2|) per element with r1, r2 from an f64 evaluation; f16
units are smaller, the same bound holds.  f32 has no intermediate rounding: compared with f64 under the f32 bound of
tests/test_gpu_hostops.py.

The footprint case is registered with tests/test_gpu_footprint.py's registry (tests/test_capi_cpu.py reads it).
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
WIDTHS = (1, 24, 320, 1283)   # one row, less than a wave's rows, whole row groups, rows that straddle a workgroup's end
NO_CONV_BIAS = 1              # index of the site without a conv bias


@functools.lru_cache(maxsize=None)
def _problem(K: int, B: int, dt: torch.dtype):
    g = torch.Generator().manual_seed(K * 10 + B)
    temb = (torch.randn(B, K, generator=g) * 1.5).to(dt).to(DEV)
    sites = []
    for i, N in enumerate(WIDTHS):
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dt).to(DEV)
        b = (torch.randn(N, generator=g) * 0.5).to(dt).to(DEV)
        cb = None if i == NO_CONV_BIAS else (torch.randn(N, generator=g) * 0.5).to(dt).to(DEV)
        sites.append((w, b, cb))
    return temb, tuple(sites)


def _sequence(temb, sites):
    out = []
    for w, b, cb in sites:
        t = F.linear(F.silu(temb), w, b)
        out.append((t if cb is None else t + cb).float())
    return out


def _f64(temb, sites):
    """(r1, r2) per site in f64, from silu rounded to the activation dtype as the sequence's is."""
    x = F.silu(temb.double()).to(temb.dtype).double()
    out = []
    for w, b, cb in sites:
        r1 = x @ w.double().t() + b.double()
        out.append((r1, r1 if cb is None else r1 + cb.double()))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("K", [128, 1280])
def test_against_the_sequence_it_replaces(K, B, dt):
    from tests.test_gpu_hostops import _close

    temb, sites = _problem(K, B, dt)
    assert _C.temb_addends_supported(B, K, dt)
    table = _C.TembTable(list(sites), B)
    got = table.slices(_C.temb_addends(table, temb))
    for i, (o, seq, (r1, r2)) in enumerate(zip(got, _sequence(temb, sites), _f64(temb, sites))):
        assert o.dtype == torch.float32 and o.is_contiguous() and tuple(o.shape) == (B, WIDTHS[i])
        if dt == torch.float32:
            _close(o, r2, dt, scale=float(r2.abs().max()), msg=f"site {i} against f64")
            continue
        err, bound = (o.double() - seq.double()).abs(), 2.0 ** -7 * (r1.abs() + r2.abs())
        print(f"K={K} B={B} {dt} site {i}: worst |out - seq| / bound = {float((err / (bound + 1e-30)).max()):.3f}")
        assert bool((err <= bound).all()), f"site {i}: {int((err > bound).sum())} of {err.numel()} outside the bound"
        assert torch.equal(o, o.to(dt).float()), "values are not representable in the activation dtype"


@pytest.mark.gpu
def test_supported_query_and_refusals():
    assert _C.temb_addends_supported(8, 1280, torch.bfloat16)      # prior preservation at SD1.5
    assert _C.temb_addends_supported(4, 1280, torch.float32)
    assert not _C.temb_addends_supported(4, 1284, torch.bfloat16)  # K % 8 != 0
    assert not _C.temb_addends_supported(16, 1280, torch.bfloat16)  # B * K past the LDS image
    assert _C.temb_addends_supported(12, 1280, torch.bfloat16) and not _C.temb_addends_supported(13, 1280, torch.bfloat16)
    temb, sites = _problem(128, 3, torch.bfloat16)
    table = _C.TembTable(list(sites), 3)
    with pytest.raises(ValueError):
        _C.temb_addends(table, temb[:, :120].contiguous())
    with pytest.raises(RuntimeError, match="not supported"):
        _C._check(_C.require().lora_amd_temb_addends(table.table.data_ptr(), table.n, table.rows, temb.data_ptr(),
                                                     temb.data_ptr(), 3, 124, _C.BF16, FP.stream()), "temb_addends")


@FP.case("lora_amd_temb_addends")
def case_temb_addends():
    """Guards around the flat output, the gaps between and behind the site blocks untouched, every input in the middle of a
    NaN-filled allocation; values bit-equal to the unguarded launch."""
    for K, B, dt in ((128, 3, torch.bfloat16), (1280, 8, torch.bfloat16), (128, 1, torch.float32)):
        temb, sites = _problem(K, B, dt)
        psites = [tuple(None if t is None else FP.inp(t) for t in s) for s in sites]
        ptemb = FP.inp(temb)
        table = _C.TembTable(psites, B)
        plain = _C.temb_addends(_C.TembTable(list(sites), B), temb)
        tail = 24  # floats behind the last block that the launch must leave alone
        g = FP.out(table.out_floats + tail)
        _C.temb_addends(table, ptemb, out=g.data)
        FP.check(g, what=f"temb_addends K={K} B={B} {dt}")
        owned = torch.zeros(table.out_floats + tail, dtype=torch.bool, device=DEV)
        for o, n in zip(table.offsets, table.widths):
            owned[o:o + B * n] = True
        MG.assert_written(g.data[owned], "temb_addends site blocks")
        MG.assert_untouched(g.data[~owned], "temb_addends gaps between and behind the site blocks")
        if B % 8:
            assert bool((~owned[:table.out_floats]).any()), "the case needs a gap between two blocks"
        assert torch.equal(g.data[owned], plain[owned[:table.out_floats]])


@pytest.mark.gpu
def test_footprint_case():
    assert "lora_amd_temb_addends" in FP.covered()
    torch.cuda.synchronize()
    case_temb_addends()
    torch.cuda.synchronize()
