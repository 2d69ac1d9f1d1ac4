"""Resident (one-launch) channels_last GroupNorm (csrc/hostops.hip gn_nhwc_res_*_kernel) through the C ABI, next to the three
streaming launches it replaces (`lora_amd_groupnorm_nhwc_resident` off) and the ATen / float64 references.

Shapes: the smallest at which the bundle arithmetic can go wrong (several groups in one chunk, groups of several chunks,
fewer pixels than slots, odd pixel counts, two bundles), the flagship step's own shapes at one or two samples, and per
direction and dtype the largest resident pixel count at C = 640 (found through `lora_amd_groupnorm_nhwc_route`) with the
next one up, which must run streaming and still be right.

Values: `TOL` of tests/test_gpu_hostops.py against the f32 ATen reference (gradient scaled by max|grad|); the resident route's
relative L2 error against the float64 reference may exceed the streaming route's on the same inputs by at most RATIO_MAX =
the largest ratio measured on the first GPU run + 10 % (profiles/gn_resident_kbench.txt lists the ratios).
Measured (MI355X, all 233 comparisons of this file): bf16 and f16 1.0000 everywhere (both routes' error is the output
rounding); f32 0.19 .. 1.5338 for y, 0.17 .. 1.5162 for dx, the largest at (1, 40, 1, 3, 4) and (1, 48, 2, 2, 16) where both errors
are 5e-8 .. 1.1e-7, i.e. half an ulp of f32: the two routes differ in the order of a 12- to 30-term sum.
"""
import pytest
import torch
import torch.nn.functional as F

from lora_amd import _C
from tests import memguard as MG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: (1e-4, 2e-5), torch.bfloat16: (2.0 ** -7, 2e-2), torch.float16: (2.0 ** -10, 2e-3)}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
# largest (resident L2 error) / (streaming L2 error) of y and dx over every case of test_values, per dtype, as first measured
MEASURED_RATIOS = {torch.bfloat16: 1.0, torch.float16: 1.0, torch.float32: 1.5338}
RATIO_MAX = {dt: 1.10 * r for dt, r in MEASURED_RATIOS.items()}

SHAPES = [(1, 40, 1, 3, 4), (2, 80, 5, 7, 8), (1, 120, 4, 4, 4), (3, 32, 8, 8, 32), (1, 48, 2, 2, 16), (1, 88, 5, 7, 11),
          (2, 96, 3, 5, 3), (2, 1280, 8, 8, 32), (1, 2560, 16, 16, 32), (1, 640, 32, 32, 32)]
EDGE_C, EDGE_G = 640, 32


@pytest.fixture(autouse=True)
def _restore_flag():
    prev = _C.groupnorm_nhwc_resident(-1)
    try:
        yield
    finally:
        _C.groupnorm_nhwc_resident(prev)


def largest_resident_hw(dt, backward):
    """Largest pixel count at (1, EDGE_C, ., EDGE_G) that `route` sends to the resident kernel (the rule is monotone in HW)."""
    _C.groupnorm_nhwc_resident(1)
    hw = 0
    for n in range(1, 4097):
        if not _C.groupnorm_nhwc_route(1, EDGE_C, n, EDGE_G, dt, backward):
            break
        hw = n
    assert 0 < hw < 4096
    return hw


def nhwc(t):
    """[B, C, H, W] values in [B][H][W][C] memory, as the channels_last view the wrappers take."""
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def make_inputs(B, C, H, W, G, dt):
    g = torch.Generator().manual_seed(B * 1000 + C + H)
    # per-channel offsets several sigma wide: the statistics must not lose them to cancellation
    x = (torch.randn(B, C, H, W, generator=g) * 1.5 + torch.randn(1, C, 1, 1, generator=g) * 3.0).to(dt).to(DEV)
    gamma = (torch.randn(C, generator=g) * 0.5 + 1.0).to(dt).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.3).to(dt).to(DEV)
    gout = torch.randn(B, C, H, W, generator=g).to(dt).to(DEV)
    add = (torch.randn(B, C, generator=g) * 2.0).to(DEV)
    return nhwc(x), gamma, beta, nhwc(gout), add


def reference(x, gamma, beta, gout, add, G, act, ft):
    xr = x.to(ft).contiguous().requires_grad_(True)
    xin = xr if add is None else xr + add.to(ft)[:, :, None, None]
    yr = F.group_norm(xin, G, gamma.to(ft), beta.to(ft), 1e-5)
    if act:
        yr = F.silu(yr)
    yr.backward(gout.to(ft).contiguous())
    return yr.detach(), xr.grad


def run(x, gamma, beta, gout, add, G, act, fwd_resident, bwd_resident):
    """Forward and backward with the flag set per direction; asserts through `route` that the intended kernel ran."""
    B, C = x.shape[:2]
    HW = x.shape[2] * x.shape[3]
    _C.groupnorm_nhwc_resident(1 if fwd_resident else 0)
    assert _C.groupnorm_nhwc_route(B, C, HW, G, x.dtype, False) == fwd_resident
    y, aff = _C.groupnorm_nhwc_fwd(x, gamma, beta, G, 1e-5, act, add)
    _C.groupnorm_nhwc_resident(1 if bwd_resident else 0)
    assert _C.groupnorm_nhwc_route(B, C, HW, G, x.dtype, True) == bwd_resident
    dx = _C.groupnorm_nhwc_bwd(x, gout, gamma, aff, G, act)
    return y, aff, dx


def close(got, want, dt, scale=1.0, msg=""):
    rtol, atol = TOL[dt]
    torch.testing.assert_close(got.float(), want.float(), rtol=rtol, atol=atol * scale, msg=lambda m: f"{msg}: {m}")


def l2(got, want):
    return float((got.double() - want).norm() / want.norm())


def routes(B, C, HW, G, dt):
    _C.groupnorm_nhwc_resident(1)
    return _C.groupnorm_nhwc_route(B, C, HW, G, dt, False), _C.groupnorm_nhwc_route(B, C, HW, G, dt, True)


def check_shape(B, C, H, W, G, dt, want_routes=None, graph=True):
    x, gamma, beta, gout, add_t = make_inputs(B, C, H, W, G, dt)
    rf, rb = routes(B, C, H * W, G, dt)
    if want_routes is not None:
        assert (rf, rb) == want_routes, f"route {(rf, rb)}, expected {want_routes}"
    ratios = []
    for act in (True, False):
        for add in (add_t, None):
            tag = f"{(B, C, H, W, G)} {dt} act={act} addend={add is not None}"
            y32, dx32 = reference(x, gamma, beta, gout, add, G, act, torch.float32)
            y64, dx64 = reference(x, gamma, beta, gout, add, G, act, torch.float64)
            gscale = float(dx32.abs().max()) + 1e-6
            ys, affs, dxs = run(x, gamma, beta, gout, add, G, act, False, False)   # the streaming kernels
            yo, affo, dxo = run(x, gamma, beta, gout, add, G, act, rf, rb)         # the route as shipped
            for name, (y, dx) in (("streaming", (ys, dxs)), ("routed", (yo, dxo))):
                close(y, y32, dt, msg=f"{tag} {name} forward")
                close(dx, dx32, dt, scale=gscale, msg=f"{tag} {name} input gradient")
            for what, got, ref_, base, res in (("y", yo, y64, ys, rf), ("dx", dxo, dx64, dxs, rb)):
                if res:
                    e_res, e_str = l2(got, ref_), l2(base, ref_)
                    print(f"L2 {tag} {what}: resident {e_res:.4e} streaming {e_str:.4e} ratio {e_res / e_str:.4f}")
                    ratios.append((e_res / e_str, f"{tag} {what}: resident L2 error {e_res:.4e}, streaming {e_str:.4e}"))
            # either backward consumes either forward's aff
            if rf or rb:
                _, _, dx_a = run(x, gamma, beta, gout, add, G, act, rf, False)
                _, _, dx_b = run(x, gamma, beta, gout, add, G, act, False, rb)
                close(dx_a, dx32, dt, scale=gscale, msg=f"{tag} routed forward -> streaming backward")
                close(dx_b, dx32, dt, scale=gscale, msg=f"{tag} streaming forward -> routed backward")
            # two launches give the same bits
            for res_f, res_b, first in ((False, False, (ys, affs, dxs)), (rf, rb, (yo, affo, dxo))):
                again = run(x, gamma, beta, gout, add, G, act, res_f, res_b)
                for a, b in zip(first, again):
                    assert torch.equal(a, b), f"{tag}: two launches differ (resident {res_f, res_b})"
    worst = max(ratios, default=(0.0, ""))
    assert worst[0] <= RATIO_MAX[dt], f"{worst[1]}: ratio {worst[0]:.4f} > {RATIO_MAX[dt]:.4f}"
    if graph:   # one capture of forward + backward, replayed twice, against the eager launch
        for res_f, res_b in ((False, False), (rf, rb)):
            eager = run(x, gamma, beta, gout, add_t, G, True, res_f, res_b)
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                run(x, gamma, beta, gout, add_t, G, True, res_f, res_b)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                outs = run(x, gamma, beta, gout, add_t, G, True, res_f, res_b)
            for _ in range(2):
                for t in outs:
                    t.zero_()
                gr.replay()
                torch.cuda.synchronize()
                for a, b in zip(eager, outs):
                    assert torch.equal(a, b), f"{(B, C, H, W, G)} {dt}: graph replay differs from the eager launch"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,C,H,W,G", SHAPES)
def test_values(B, C, H, W, G, dt):
    # every shape of the list is resident forward, and backward up to 8x8 (the larger maps' backward depends on the dtype's
    # register bytes: tests/test_gn_resident_route.py holds the step's table)
    rf, rb = routes(B, C, H * W, G, dt)
    assert rf and (rb or H * W > 64)
    check_shape(B, C, H, W, G, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("backward", [False, True])
def test_largest_resident_geometry_and_next(dt, backward):
    hw = largest_resident_hw(dt, backward)
    rf, rb = routes(1, EDGE_C, hw, EDGE_G, dt)
    assert (rb if backward else rf)
    check_shape(1, EDGE_C, 1, hw, EDGE_G, dt, graph=False)
    rf, rb = routes(1, EDGE_C, hw + 1, EDGE_G, dt)
    assert not (rb if backward else rf), "one pixel more must run streaming"
    check_shape(1, EDGE_C, 1, hw + 1, EDGE_G, dt, graph=False)


@pytest.mark.parametrize("resident", [0, 1])
def test_footprint(resident):
    """Outputs, aff and the workspace between guards, inputs inside poison; the resident route leaves the workspace alone."""
    lib = _C.require()
    st = torch.cuda.current_stream().cuda_stream
    for B, Cc, Hh, Ww, G in ((1, 8, 1, 8, 8), (2, 96, 2, 4, 3), (1, 40, 3, 8, 5), (2, 80, 5, 7, 8)):
        HW = Hh * Ww
        for dt in (torch.float32, torch.bfloat16):
            g = torch.Generator().manual_seed(Cc + HW)
            mk = lambda shape, s=1.0: MG.poisoned((torch.randn(*shape, generator=g) * s).to(dt).to(DEV))  # noqa: E731
            xl, gl_ = mk((B, Hh, Ww, Cc), 1.5), mk((B, Hh, Ww, Cc))
            gamma, beta = mk((Cc,), 0.5), mk((Cc,), 0.3)
            add = MG.poisoned(torch.randn(B, Cc, generator=g).to(DEV))
            _C.groupnorm_nhwc_resident(resident)
            rf = _C.groupnorm_nhwc_route(B, Cc, HW, G, dt, False)
            rb = _C.groupnorm_nhwc_route(B, Cc, HW, G, dt, True)
            assert rf == rb == bool(resident), "these geometries fit the resident kernels both ways"
            wsb = int(lib.lora_amd_groupnorm_nhwc_workspace(B, Cc, HW, G))
            assert wsb > 0
            y, aff = MG.Guarded((B, Hh, Ww, Cc), dt, DEV), MG.Guarded((B, 4, Cc), torch.float32, DEV)
            ws, dx = MG.Guarded(wsb // 4, torch.float32, DEV), MG.Guarded((B, Hh, Ww, Cc), dt, DEV)
            what = f"{(B, Cc, Hh, Ww, G)} {dt} resident={resident}"
            _C._check(lib.lora_amd_groupnorm_nhwc_fwd(xl.data_ptr(), gamma.data_ptr(), beta.data_ptr(), add.data_ptr(), y.ptr,
                                                      aff.ptr, ws.ptr, wsb, B, Cc, HW, G, 1e-5, 1, _C.dtype_code(dt), st), what)
            torch.cuda.synchronize()
            if resident:
                MG.assert_untouched(ws.data, what + " workspace after the forward")
            _C._check(lib.lora_amd_groupnorm_nhwc_bwd(xl.data_ptr(), gl_.data_ptr(), None, Cc, gamma.data_ptr(), aff.ptr, dx.ptr,
                                                      ws.ptr, wsb, B, Cc, HW, G, 1, _C.dtype_code(dt), st), what)
            torch.cuda.synchronize()
            for i, gd in enumerate((y, aff, ws, dx)):
                gd.check(f"{what} operand {i}")
            for name, gd in (("y", y), ("aff", aff), ("dx", dx)):
                MG.assert_written(gd.data, f"{what} {name}")
                MG.assert_finite(gd.data, what=f"{what} {name}")
            if resident:
                MG.assert_untouched(ws.data, what + " workspace after the backward")
            y32, dx32 = reference(xl.permute(0, 3, 1, 2), gamma, beta, gl_.permute(0, 3, 1, 2), add, G, True, torch.float32)
            close(y.data.permute(0, 3, 1, 2), y32, dt, msg=what + " forward")
            close(dx.data.permute(0, 3, 1, 2), dx32, dt, scale=float(dx32.abs().max()) + 1e-6, msg=what + " input gradient")
