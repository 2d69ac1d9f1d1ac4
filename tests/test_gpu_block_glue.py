"""The ResnetBlock2D tail (csrc/hostops.hip resnet_tail_kernel) and the channels_last GroupNorm backward with a second
gradient (``gsum``), through the wrappers of ``_C`` and ``standin/fused.py``.

Both replace ATen adds whose roundings they reproduce, so every comparison is ``torch.equal``: the tail against
``(r + bs) + (h + b2)`` on the same tensors, the backward against ``groupnorm_nhwc_bwd(...) + gsum`` (and, without gsum,
against the old entry point), streaming and resident.  Shapes are the smallest at which the indexing can go wrong: one
chunk, a chunk count that does not divide the workgroup, fewer rows than slots, 5 channels per group, one pixel, and per
dtype the largest pixel count the resident backward takes at C = 640 with the next one up (found through the route query).
The footprint cases run both kernels between guards at odd pixel counts; they are registered with
tests/test_gpu_footprint.py's registry (tests/test_capi_cpu.py reads it).
"""
import pytest
import torch

from lora_amd import _C
from lora_amd.standin import fused
from tests import memguard as MG
from tests import test_gpu_footprint as FP
from tests.test_gpu_gn_resident import largest_resident_hw, make_inputs, nhwc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
TAIL_SHAPES = [(1, 8, 1, 1), (3, 24, 1, 5), (2, 40, 3, 3), (2, 320, 8, 8)]
GN_SHAPES = [(1, 40, 3, 3, 8), (2, 32, 4, 4, 8), (1, 64, 1, 1, 32)]
EDGE_C, EDGE_G = 640, 32


@pytest.fixture(autouse=True)
def _restore_flag():
    prev = _C.groupnorm_nhwc_resident(-1)
    try:
        yield
    finally:
        _C.groupnorm_nhwc_resident(prev)


def _aten_tail(h, r, b2, bs):
    h = h + b2.view(1, -1, 1, 1)
    return (r if bs is None else r + bs.view(1, -1, 1, 1)) + h


def _tail_inputs(B, C, H, W, dt, seed=0):
    g = torch.Generator().manual_seed(seed + C + H * W)
    mk = lambda *s: torch.randn(*s, generator=g).to(dt).to(DEV)  # noqa: E731
    return nhwc(mk(B, C, H, W) * 2.0), nhwc(mk(B, C, H, W) * 2.0), mk(C), mk(C)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,C,H,W", TAIL_SHAPES)
def test_resnet_tail_values(B, C, H, W, dt):
    h, r, b2, bs = _tail_inputs(B, C, H, W, dt)
    for name, rr, bb in (("shortcut bias", r, bs), ("no shortcut bias", r, None), ("r is h", h, None), ("r is h, bias", h, bs)):
        assert _C.resnet_tail_supported(h, rr, b2, bb)
        got = _C.resnet_tail(h, rr, b2, bb)
        want = _aten_tail(h, rr, b2, bb)
        assert got.shape == want.shape and got.stride() == torch.empty_like(want, memory_format=torch.channels_last).stride()
        assert torch.equal(got, want), f"{(B, C, H, W)} {dt} {name}: {int((got != want).sum())} elements differ"
        assert torch.equal(fused.resnet_tail(h, rr, b2, bb), want)


@pytest.mark.parametrize("dt", DTYPES)
def test_resnet_tail_views_and_fallback(dt):
    B, C, H, W, pad = 2, 40, 3, 5, 16
    g = torch.Generator().manual_seed(5)
    big_h = (torch.randn(B, H, W, C + pad, generator=g) * 2).to(dt).to(DEV)
    big_r = (torch.randn(B, H, W, C + 2 * pad, generator=g) * 2).to(dt).to(DEV)
    b2, bs = torch.randn(C, generator=g).to(dt).to(DEV), torch.randn(C, generator=g).to(dt).to(DEV)
    # dense channels_last rows inside wider rows, at an offset of 16 elements (32 or 64 bytes)
    h = big_h[..., pad:].permute(0, 3, 1, 2)
    r = big_r[..., pad:pad + C].permute(0, 3, 1, 2)
    assert h.data_ptr() % 32 == 0 and not h.is_contiguous(memory_format=torch.channels_last)
    assert _C.resnet_tail_supported(h, r, b2, bs)
    assert torch.equal(_C.resnet_tail(h, r, b2, bs), _aten_tail(h, r, b2, bs))
    assert torch.equal(fused.resnet_tail(h, r, b2, None), _aten_tail(h, r, b2, None))
    # an offset of one element: not 16-byte aligned, the ATen adds run and give the same values
    hm = big_h[..., 1:1 + C].permute(0, 3, 1, 2)
    assert hm.data_ptr() % 16 != 0 and not _C.resnet_tail_supported(hm, r, b2, bs)
    with pytest.raises(ValueError):
        _C.resnet_tail(hm, r, b2, bs)
    assert torch.equal(fused.resnet_tail(hm, r, b2, bs), _aten_tail(hm, r, b2, bs))
    # NCHW operands and a bias that trains take the fallback as well
    hc = h.contiguous()
    assert not _C.resnet_tail_supported(hc, hc, b2, bs)
    assert torch.equal(fused.resnet_tail(hc, hc, b2, bs), _aten_tail(hc, hc, b2, bs))
    bt = b2.clone().requires_grad_(True)
    out = fused.resnet_tail(h, r, bt, bs)
    assert torch.equal(out.detach(), _aten_tail(h, r, b2, bs))
    out.float().sum().backward()
    assert bt.grad is not None and torch.equal(bt.grad, torch.full_like(bt, B * H * W))


def test_resnet_tail_backward_passes_the_gradient_on():
    h, r, b2, bs = _tail_inputs(2, 24, 3, 3, torch.bfloat16)
    h.requires_grad_(True)
    r.requires_grad_(True)
    out = fused.resnet_tail(h, r, b2, bs)
    assert type(out.grad_fn).__name__.startswith("_ResnetTail")
    g = nhwc(torch.randn(2, 24, 3, 3).to(torch.bfloat16).to(DEV))
    out.backward(g)
    assert torch.equal(h.grad, g) and torch.equal(r.grad, g)


def _gn_case(B, C, H, W, G, dt, act, resident, want_route=None):
    x, gamma, beta, gout, add = make_inputs(B, C, H, W, G, dt)
    gsum = nhwc((torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(C + H)) * 0.7).to(dt).to(DEV))
    _C.groupnorm_nhwc_resident(resident)
    route = _C.groupnorm_nhwc_route_add(B, C, H * W, G, dt)
    assert route == _C.groupnorm_nhwc_route(B, C, H * W, G, dt, True), "every resident form holds the third operand"
    if want_route is not None:
        assert route == want_route
    if not resident:
        assert not route
    _, aff = _C.groupnorm_nhwc_fwd(x, gamma, beta, G, 1e-5, act, add)
    base = _C.groupnorm_nhwc_bwd(x, gout, gamma, aff, G, act)
    tag = f"{(B, C, H, W, G)} {dt} act={act} resident={resident} (route {route})"
    # null gsum by a raw call, whatever row stride comes with it: the wrapper's bits
    lib = _C.require()
    nbytes = _C.groupnorm_nhwc_workspace(B, C, H * W, G)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    dx0 = torch.empty_like(x)
    _C._check(lib.lora_amd_groupnorm_nhwc_bwd(x.data_ptr(), gout.data_ptr(), None, 0, gamma.data_ptr(), aff.data_ptr(),
                                              dx0.data_ptr(), ws.data_ptr(), nbytes, B, C, H * W, G, 1 if act else 0,
                                              _C.dtype_code(dt), torch.cuda.current_stream().cuda_stream), tag)
    assert torch.equal(dx0, base), f"{tag}: gsum null with row stride 0 differs from the wrapper's call"
    got = _C.groupnorm_nhwc_bwd(x, gout, gamma, aff, G, act, gsum)
    want = base + gsum
    assert torch.equal(got, want), f"{tag}: {int((got != want).sum())} of {want.numel()} elements differ from bwd + gsum"
    # gsum as a channel slice of a wider channels_last gradient (what the backward of a concatenation hands out)
    wide = torch.full((B, H, W, C + 24), float("nan"), dtype=dt, device=DEV)
    wide[..., 16:16 + C] = gsum.permute(0, 2, 3, 1)
    sl = wide[..., 16:16 + C].permute(0, 3, 1, 2)
    assert _C.gsum_takes(x, sl) and sl.stride() != x.stride()
    got = _C.groupnorm_nhwc_bwd(x, gout, gamma, aff, G, act, sl)
    assert torch.equal(got, want), f"{tag}: gsum as a slice: {int((got != want).sum())} of {want.numel()} elements differ"
    return route


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("resident", [0, 1])
@pytest.mark.parametrize("B,C,H,W,G", GN_SHAPES)
def test_groupnorm_bwd_gsum(B, C, H, W, G, resident, act, dt):
    route = _gn_case(B, C, H, W, G, dt, act, resident)
    assert route == bool(resident), "these geometries fit the resident backward"


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("act", [True, False])
def test_groupnorm_bwd_gsum_largest_resident_geometry_and_next(act, dt):
    hw = largest_resident_hw(dt, True)
    for resident in (0, 1):
        _gn_case(1, EDGE_C, 1, hw, EDGE_G, dt, act, resident, want_route=bool(resident))
        _gn_case(1, EDGE_C, 1, hw + 1, EDGE_G, dt, act, resident, want_route=False)


FOOT_SHAPES = ((1, 8, 1, 7, 8), (2, 96, 3, 3, 3), (1, 40, 3, 5, 5), (2, 80, 5, 7, 8))   # odd pixel counts


def _foot_inputs(B, Cc, Hh, Ww, dt):
    g = torch.Generator().manual_seed(Cc + Hh * Ww)
    mk = lambda shape, s=1.0: MG.poisoned((torch.randn(*shape, generator=g) * s).to(dt).to(DEV))  # noqa: E731
    return mk((B, Hh, Ww, Cc), 1.5), mk((B, Hh, Ww, Cc)), mk((B, Hh, Ww, Cc)), mk((Cc,), 0.5), mk((Cc,), 0.3)


@FP.case("lora_amd_groupnorm_nhwc_bwd")
def case_groupnorm_nhwc_bwd_add():
    """dx and the workspace between guards, x, gout, gsum and gamma inside poison, streaming and resident; the resident
    launch leaves the workspace alone; values bit-equal to the unguarded backward + gsum."""
    lib, st = _C.require(), torch.cuda.current_stream().cuda_stream
    prev = _C.groupnorm_nhwc_resident(-1)
    try:
        for resident in (0, 1):
            for B, Cc, Hh, Ww, G in FOOT_SHAPES:
                HW = Hh * Ww
                for dt in (torch.float32, torch.bfloat16):
                    xl, gl_, sl, gamma, beta = _foot_inputs(B, Cc, Hh, Ww, dt)
                    what = f"{(B, Cc, Hh, Ww, G)} {dt} resident={resident}"
                    _C.groupnorm_nhwc_resident(resident)
                    assert _C.groupnorm_nhwc_route_add(B, Cc, HW, G, dt) == bool(resident)
                    x4, g4, s4 = (t.permute(0, 3, 1, 2) for t in (xl, gl_, sl))
                    _, aff = _C.groupnorm_nhwc_fwd(x4, gamma, beta, G, 1e-5, True, None)
                    wsb = _C.groupnorm_nhwc_workspace(B, Cc, HW, G)
                    ws, dx = MG.Guarded(wsb // 4, torch.float32, DEV), MG.Guarded((B, Hh, Ww, Cc), dt, DEV)
                    _C._check(lib.lora_amd_groupnorm_nhwc_bwd(xl.data_ptr(), gl_.data_ptr(), sl.data_ptr(), Cc,
                                                              gamma.data_ptr(), aff.data_ptr(), dx.ptr, ws.ptr, wsb, B, Cc,
                                                              HW, G, 1, _C.dtype_code(dt), st), what)
                    torch.cuda.synchronize()
                    dx.check(what + " dx")
                    ws.check(what + " workspace")
                    MG.assert_written(dx.data, what + " dx")
                    MG.assert_finite(dx.data, what=what + " dx")
                    if resident:
                        MG.assert_untouched(ws.data, what + " workspace")
                    want = _C.groupnorm_nhwc_bwd(x4, g4, gamma, aff, G, True) + s4
                    assert torch.equal(dx.data.permute(0, 3, 1, 2), want), what
    finally:
        _C.groupnorm_nhwc_resident(prev)


@FP.case("lora_amd_resnet_tail")
def case_resnet_tail():
    """out between guards, h, r and both biases inside poison, with and without the shortcut bias; values bit-equal to the
    three ATen adds."""
    lib, st = _C.require(), torch.cuda.current_stream().cuda_stream
    for B, Cc, Hh, Ww, _ in FOOT_SHAPES:
        for dt in (torch.float32, torch.bfloat16):
            hl, _, rl, b2, bs = _foot_inputs(B, Cc, Hh, Ww, dt)
            h4, r4 = hl.permute(0, 3, 1, 2), rl.permute(0, 3, 1, 2)
            out = MG.Guarded((B, Hh, Ww, Cc), dt, DEV)
            for bias_s in (bs, None):
                what = f"tail {(B, Cc, Hh, Ww)} {dt} shortcut bias={bias_s is not None}"
                MG.fill_sentinel(out.data)
                _C._check(lib.lora_amd_resnet_tail(hl.data_ptr(), Cc, rl.data_ptr(), Cc, b2.data_ptr(),
                                                   None if bias_s is None else bias_s.data_ptr(), out.ptr, Cc, B * Hh * Ww, Cc,
                                                   _C.dtype_code(dt), st), what)
                torch.cuda.synchronize()
                out.check(what)
                MG.assert_written(out.data, what)
                MG.assert_finite(out.data, what=what)
                assert torch.equal(out.data.permute(0, 3, 1, 2), _aten_tail(h4, r4, b2, bias_s)), what


@pytest.mark.parametrize("case", [case_groupnorm_nhwc_bwd_add, case_resnet_tail])
def test_footprint_cases(case):
    assert {"lora_amd_groupnorm_nhwc_bwd", "lora_amd_resnet_tail"} <= FP.covered()
    torch.cuda.synchronize()
    case()
    torch.cuda.synchronize()
