"""Channels-last 3x3 Conv2d adapters of rank 20, 24, .., 64 on the matrix-core kernels (csrc/conv_nhwc.hip, the wide entries;
``ops.CONV3_WIDE``): ns = ceil(r / 16) rank-16 slices inside ONE launch of the pack and of each of T, dX and dDown.

(1) the pack against the rank <= 16 pack of every zero-padded slice, bit for bit; (2) the three kernels against
oracle/lora_numpy at the bounds of tests/test_gpu_conv_nhwc.py::test_conv3_nhwc_kernels_match_oracle (the per-rank arithmetic
is the same), dX from a non-zero dx0 and the dDown slab NaN-filled; (3) against the per-slice results of the rank-16 entry
points; (4) the module against oracle/torch_ref.conv_adapter_forward; (5) selector and GradSink; (6) dropout under the restated
Philox mask; (7) the switch off; (8) an eager and (9) a captured step of the small stand-in UNet with the extended injection.

(8): the conv adapters run with dropout 0 — with the switch off a site draws its mask in NCHW order, with it on in [B*H*W, C]
order, so ONE oracle step cannot be handed the draws of both settings; the Linear adapters keep dropout 0.1 and the oracle is
handed their draws (tests/test_gpu_factors_wide_masked.py's scheme).  Measured on MI355X, rank 24, flat LoRA gradient against the
f32 oracle step: see CONV3_WIDE_RATIO_BOUND below."""
from __future__ import annotations

import copy
import gc

import numpy as np
import pytest
import torch

import lora_amd as L
from lora_amd import _C, ops
from lora_amd import trainer as T
from lora_amd.standin import DDPMScheduler
from lora_amd.standin.unet import UNet2DConditionModel
from oracle import lora_numpy as O
from oracle import torch_ref as TR
from tests import helpers as H
from tests import memguard as MG
from tests import test_gpu_footprint as FP
from tests.test_gpu_conv_nhwc import _module_case, cl, rounded, rows_to_nchw
from tests.test_gpu_kernels import DT, close, n, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (8): ‖on − f32 oracle‖ / ‖off − f32 oracle‖ of the flat LoRA gradient (Linear and Conv2d adapters, rank 24, 22 3x3 sites), both
# settings on the same dropout draws of the Linear sites; off = the library route = the parent's arithmetic.  Measured on MI355X
# (first GPU visit): on 8.1546e-03, off 8.5088e-03, ratio 0.958 (‖oracle‖ 4.2768e-01).  Bound = measured + 10 % = 0.958 x 1.10
CONV3_WIDE_RATIO_BOUND = 1.054

GEOM = ((1, 1), (1, 1), (1, 1))


def _fold(part, plan, C, r):
    d_down = torch.empty((r, C, 3, 3), device=DEV)
    table, nn_, total = _C.make_reduce_table([(part, d_down, plan.nsplit, plan.rank_pad, C * 9, r, _C.FACTOR_RK, 1.0, 0.0)], DEV)
    _C.reduce_batched(table, nn_, total)
    return d_down


def _slice16(down, s):
    """down[16 s : 16 s + 16] zero-padded to 16 ranks."""
    out = torch.zeros((16,) + tuple(down.shape[1:]), dtype=down.dtype, device=down.device)
    live = min(16, down.shape[0] - 16 * s)
    out[:live] = down[16 * s:16 * s + live]
    return out, live


# ----------------------------------------------------------------------------- (1) pack
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("r", [20, 64])
def test_wide_pack_slices_are_the_rank_16_packs(r, dt):
    C = 64
    plan = _C.conv3_nhwc_wide_plan(1, C, 4, 4, r)
    p16 = _C.conv3_nhwc_plan(1, C, 4, 4, 16)
    ns = -(-r // 16)
    assert plan.native == 1 and plan.rank_pad == 16 * ns and plan.ks == p16.ks == 5
    assert plan.pf_elems == ns * p16.pf_elems and plan.pd_elems == ns * p16.pd_elems
    down = rnd((r, C, 3, 3), "f32", 0.2, seed=3)
    pf, pd = _C.conv3_nhwc_wide_pack(down, DT[dt], plan)
    for s in range(ns):
        d16, _ = _slice16(down, s)
        pf1, pd1 = _C.conv3_nhwc_pack(d16, DT[dt], p16)
        a, b = int(p16.pf_elems), int(p16.pd_elems)
        assert torch.equal(pf[s * a:(s + 1) * a].view(torch.int16), pf1.view(torch.int16)), (s, "pf")
        assert torch.equal(pd[s * b:(s + 1) * b].view(torch.int16), pd1.view(torch.int16)), (s, "pd")


# ----------------------------------------------------------------------------- (2) oracle
CASES = [
    # B, C, H, W, r, dt, pt: the forward tile rows the plan picks (dX runs min(pt, 2) rows up to two slices, one above)
    (1, 64, 1, 1, 20, "bf16", 1),       # one pixel, tail slice of 4
    (3, 64, 5, 7, 28, "bf16", 1),       # masked tile edges, tail of 12
    (1, 128, 8, 32, 32, "bf16", 1),     # two full slices, two column tiles
    (1, 64, 3, 70, 40, "bf16", 1),      # ragged last column tile, tail of 8
    (2, 192, 12, 12, 48, "f16", 1),     # three channel chunks, f16
    (1, 1280, 12, 12, 64, "bf16", 1),   # ksplit > 1 and csplit > 1, four slices
    (4, 320, 32, 32, 64, "bf16", 2),    # several strips per workgroup; 64 four-row tiles: the plan picks two tile rows here
    # every tile height of T with 2, 3 and 4 slices, and the two-row dX (two slices only)
    (4, 64, 32, 32, 24, "bf16", 2),     # pt 2, two slices: dX with two tile rows, tail of 8
    (4, 64, 31, 32, 40, "f16", 2),      # pt 2, three slices, odd H: a half-empty last tile row, f16
    # pt 4 needs 200 four-row tiles: many small images with ragged tiles keep the oracle at a few thousand pixels
    (50, 64, 5, 17, 64, "bf16", 4),     # pt 4, four slices; last tile row and last column tile one pixel deep
    (50, 64, 6, 17, 24, "f16", 4),      # pt 4, two slices (dX two rows), f16
    (34, 64, 5, 33, 36, "bf16", 4),     # pt 4, three slices, tail of 4, three column tiles
]


@pytest.mark.parametrize("B,C,Hh,Ww,r,dt,pt", CASES)
def test_conv3_wide_kernels_match_oracle(B, C, Hh, Ww, r, dt, pt):
    plan = _C.conv3_nhwc_wide_plan(B, C, Hh, Ww, r)
    assert plan.native == 1 and _C.conv3_nhwc_plan(B, C, Hh, Ww, r).native == 0
    assert plan.pt == pt
    if C == 1280:
        assert plan.ksplit > 1 and plan.csplit > 1
    x = cl(rnd((B, C, Hh, Ww), dt, seed=1))
    down = rnd((r, C, 3, 3), "f32", 0.2, seed=3)
    pf, pd = _C.conv3_nhwc_wide_pack(down, DT[dt], plan)
    eye = np.eye(r, dtype=np.float32).reshape(r, r, 1, 1)
    # ---- T = conv3x3(X; down), the factor rounded to the activation dtype
    t = _C.conv3_nhwc_wide_down_fwd(x, pf, r)
    assert t.shape == (B * Hh * Ww, r)
    down_r = rounded(down, dt)
    _, t_o = O.lora_conv2d_forward(n(x), None, None, n(down_r), eye, 1.0, *GEOM)
    absx = np.abs(n(x)).max() * np.abs(n(down)).sum(axis=(1, 2, 3)).max()
    close(rows_to_nchw(t, B, Hh, Ww), t_o, absx, "f32", k=3e-5, msg="T")
    # ---- gradients for a given Gt [B*H*W, r]; dX from a non-zero dx0: one read-modify-write
    gt = rnd((B * Hh * Ww, r), "f32", 1.0, seed=5)
    gt_nchw = rounded(gt, dt).reshape(B, Hh, Ww, r).permute(0, 3, 1, 2).contiguous()
    dx0 = cl(rnd((B, C, Hh, Ww), dt, seed=8))
    dx = dx0.clone(memory_format=torch.preserve_format)
    _C.conv3_nhwc_wide_bwd_dx_(dx, gt, pd)
    dxo, _, _ = O.lora_conv2d_backward(n(gt_nchw), n(x), None, n(down_r), eye, 1.0, *GEOM)
    absg = np.abs(n(gt)).max() * np.abs(n(down)).sum(axis=(0, 2, 3)).max()
    close(n(dx), dxo + n(dx0), absg + np.abs(n(dx0)), dt, k=3e-5, msg="dX")
    # ---- dDown: the slab starts as NaN — every live row is written, rows >= r are never read
    part = torch.full((int(plan.down_part_floats),), float("nan"), device=DEV)
    _C.conv3_nhwc_wide_bwd_down(x, gt, part)
    slab = part.view(plan.nsplit, plan.rank_pad, C * 9)
    assert bool(torch.isfinite(slab[:, :r]).all())
    assert r == plan.rank_pad or bool(torch.isnan(slab[:, r:]).all())
    d_down = _fold(part, plan, C, r)
    _, ddo, _ = O.lora_conv2d_backward(n(gt_nchw), n(x), None, n(down), eye, 1.0, *GEOM)
    kk = 1e-4
    np.testing.assert_allclose(n(d_down), ddo, rtol=kk * 10, atol=kk * np.abs(ddo).max() + 1e-6, err_msg="dDown")


# ----------------------------------------------------------------------------- (3) slices
def test_wide_launches_equal_the_rank_16_entry_points_slice_by_slice():
    """T and dDown of slice s are the rank-16 entry points' on down[16 s : 16 s + 16] / Gt[:, 16 s : 16 s + 16] at the f32
    setting of ``close`` (only the summation order may differ).  dX − dx0 against the sum of the per-slice increments: every
    stored dX carries one rounding to the activation dtype (the wide one once, each narrow one once), which no summation
    order removes, so that comparison adds EPS[bf16] of each stored value to the f32 bound."""
    B, C, Hh, Ww, r, dt = 1, 128, 8, 32, 32, "bf16"
    plan, p16 = _C.conv3_nhwc_wide_plan(B, C, Hh, Ww, r), _C.conv3_nhwc_plan(B, C, Hh, Ww, 16)
    x = cl(rnd((B, C, Hh, Ww), dt, seed=1))
    down = rnd((r, C, 3, 3), "f32", 0.2, seed=3)
    gt = rnd((B * Hh * Ww, r), "f32", 1.0, seed=5)
    dx0 = cl(rnd((B, C, Hh, Ww), dt, 0.125, seed=8))
    pf, pd = _C.conv3_nhwc_wide_pack(down, DT[dt], plan)
    t = _C.conv3_nhwc_wide_down_fwd(x, pf, r)
    dx = dx0.clone(memory_format=torch.preserve_format)
    _C.conv3_nhwc_wide_bwd_dx_(dx, gt, pd)
    part = torch.full((int(plan.down_part_floats),), float("nan"), device=DEV)
    _C.conv3_nhwc_wide_bwd_down(x, gt, part)
    d_down = _fold(part, plan, C, r)
    absx = np.abs(n(x)).max() * np.abs(n(down)).sum(axis=(1, 2, 3)).max()
    absg = np.abs(n(gt)).max() * np.abs(n(down)).sum(axis=(0, 2, 3)).max()
    eye = np.eye(16, dtype=np.float32).reshape(16, 16, 1, 1)
    inc, stored = np.zeros(dx0.shape, np.float64), np.abs(n(dx)).astype(np.float64)
    for s in range(2):
        d16, live = _slice16(down, s)
        assert live == 16
        pf1, pd1 = _C.conv3_nhwc_pack(d16, DT[dt], p16)
        gts = gt[:, 16 * s:16 * s + 16].contiguous()
        t1 = _C.conv3_nhwc_down_fwd(x, pf1, 16)
        close(n(t[:, 16 * s:16 * s + 16]), n(t1), absx, "f32", msg=f"T slice {s}")
        dx1 = dx0.clone(memory_format=torch.preserve_format)
        _C.conv3_nhwc_bwd_dx_(dx1, gts, pd1)
        inc += n(dx1).astype(np.float64) - n(dx0)
        stored += np.abs(n(dx1))
        part1 = torch.full((int(p16.down_part_floats),), float("nan"), device=DEV)
        _C.conv3_nhwc_bwd_down(x, gts, part1)
        dd1 = _fold(part1, p16, C, 16)
        gabs = np.abs(n(rounded(gts, dt))).reshape(B, Hh, Ww, 16).transpose(0, 3, 1, 2)
        _, absd, _ = O.lora_conv2d_backward(gabs, np.abs(n(x)), None, n(d16), eye, 1.0, *GEOM)
        close(n(d_down[16 * s:16 * s + 16]), n(dd1), absd, "f32", msg=f"dDown slice {s}")
    got = n(dx).astype(np.float64) - n(dx0)
    tol = 2e-5 * absg + 2.0 ** -8 * stored
    assert np.all(np.abs(got - inc) <= tol), float((np.abs(got - inc) / tol).max())
    assert float(np.abs(inc).max()) > 4 * float(np.abs(n(dx0)).max()), "the increments dominate dx0 in this case"


# ----------------------------------------------------------------------------- footprint
@FP.case("lora_amd_conv3_nhwc_wide_pack", "lora_amd_conv3_nhwc_wide_down_fwd", "lora_amd_conv3_nhwc_wide_bwd_dx",
         "lora_amd_conv3_nhwc_wide_bwd_down")
def case_conv3_nhwc_wide():
    """tests/test_gpu_footprint.py::case_conv3_nhwc at ranks 20 / 40 / 64: guarded outputs, poisoned inputs, a partial pixel
    tile (W = 20), a ksplit > 1 forward, csplit and nsplit partials; T, dX and dDown against f64; the slab rows >= r keep the
    sentinel."""
    Fn = torch.nn.functional
    for B, Ci, Hh, Ww, r in ((1, 640, 12, 20, 64), (2, 64, 20, 20, 20), (1, 128, 9, 20, 40)):
        plan = _C.conv3_nhwc_wide_plan(B, Ci, Hh, Ww, r)
        assert plan.native == 1
        M = B * Hh * Ww
        x = FP.inp(FP.rnd((B, Hh, Ww, Ci), FP.BF, seed=1))
        down = FP.inp(FP.rnd((r, Ci, 3, 3), FP.F32, 0.1, seed=2))
        gt = FP.inp(FP.rnd((M, r), FP.F32, 0.5, seed=3))
        pf, pd = FP.out(int(plan.pf_elems), FP.BF), FP.out(int(plan.pd_elems), FP.BF)
        lib, stream = FP.lib(), FP.stream()
        FP.ok(lib.lora_amd_conv3_nhwc_wide_pack(down.data_ptr(), r, Ci, _C.BF16, pf.ptr, pd.ptr, stream), "conv3_nhwc_wide_pack")
        t_part, t = FP.out(max(int(plan.t_part_floats), 1)), FP.out((M, r))
        FP.ok(lib.lora_amd_conv3_nhwc_wide_down_fwd(x.data_ptr(), pf.ptr, t_part.ptr if plan.t_part_floats else None, t.ptr, B,
                                                    Ci, Hh, Ww, r, _C.BF16, stream), "conv3_nhwc_wide_down_fwd")
        dx0 = FP.rnd((M, Ci), FP.BF, seed=4)
        dx = MG.guarded_like(dx0)
        FP.ok(lib.lora_amd_conv3_nhwc_wide_bwd_dx(dx.ptr, gt.data_ptr(), pd.ptr, B, Ci, Hh, Ww, r, _C.BF16, stream),
              "conv3_nhwc_wide_bwd_dx")
        dnp = FP.out(int(plan.down_part_floats))
        FP.ok(lib.lora_amd_conv3_nhwc_wide_bwd_down(x.data_ptr(), gt.data_ptr(), dnp.ptr, B, Ci, Hh, Ww, r, _C.BF16, stream),
              "conv3_nhwc_wide_bwd_down")
        FP.check(pf, pd, t_part, t, dx, dnp, what=f"conv3_nhwc_wide B={B} Ci={Ci} r={r}")
        MG.assert_written(pf.data, "conv3 wide pf")
        MG.assert_written(pd.data, "conv3 wide pd")
        MG.assert_written(t.data, "conv3 wide T")
        X = FP.d64(x).permute(0, 3, 1, 2)
        dnb = FP.d64(down.to(FP.BF))
        T_ = Fn.conv2d(X, dnb, padding=1).permute(0, 2, 3, 1).reshape(M, r)
        FP.close(t.data, T_, Fn.conv2d(X.abs(), dnb.abs(), padding=1).permute(0, 2, 3, 1).reshape(M, r), k=3e-5, msg="conv3 wide T")
        Gt = FP.d64(gt.to(FP.BF)).view(B, Hh, Ww, r).permute(0, 3, 1, 2)
        DX = Fn.conv_transpose2d(Gt, dnb, padding=1).permute(0, 2, 3, 1).reshape(M, Ci)
        DXabs = Fn.conv_transpose2d(Gt.abs(), dnb.abs(), padding=1).permute(0, 2, 3, 1).reshape(M, Ci)
        FP.close(dx.data, FP.d64(dx0) + DX, FP.d64(dx0).abs() + DXabs, FP.BF, k=3e-5, msg="conv3 wide dX")
        slab = dnp.data.view(int(plan.nsplit), int(plan.rank_pad), Ci * 9)
        MG.assert_written(slab[:, :r], "conv3 wide dDown: every live row of every split")
        if r < plan.rank_pad:
            MG.assert_untouched(slab[:, r:], "conv3 wide dDown: rows >= r")
        want = torch.nn.grad.conv2d_weight(X, (r, Ci, 3, 3), Gt, padding=1).reshape(r, Ci * 9)
        wabs = torch.nn.grad.conv2d_weight(X.abs(), (r, Ci, 3, 3), Gt.abs(), padding=1).reshape(r, Ci * 9)
        FP.close(FP.d64(slab)[:, :r].sum(0), want, wabs, k=1e-4, msg="conv3 wide dDown")


def test_footprint_case():
    assert "conv3_nhwc_wide" in FP.CASES and "lora_amd_conv3_nhwc_wide_bwd_down" in FP.covered()
    torch.cuda.synchronize()
    case_conv3_nhwc_wide()
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- (4) module
@pytest.fixture
def path_log(monkeypatch):
    log = []
    monkeypatch.setattr(ops, "PATH_LOG", log)
    return log


def _check_module(m, x, gy_c, ref, dt, channels_last=True):
    yr, dxr, ddr, dur = ref
    y = m(x)
    assert y.shape == yr.shape
    if channels_last:
        assert y.is_contiguous(memory_format=torch.channels_last)
    (y.float() * gy_c.to(DEV)).sum().backward()
    e = 2.0 ** -7 if dt == "bf16" else 2.0 ** -9
    assert (n(y) - n(yr)).__abs__().max() <= e * float(yr.abs().max()) + 1e-3
    assert np.abs(n(x.grad) - n(dxr)).max() <= 2 * e * float(dxr.abs().max())
    for name, got, want in (("ddown", m.lora_down.weight.grad, ddr), ("dup", m.lora_up.weight.grad, dur)):
        err = np.abs(n(got) - n(want)).max() / float(want.abs().max())
        assert got.shape == want.shape and err <= 4e-3, (name, err)


@pytest.mark.parametrize("Ci,Co,r,Hh,Ww,B,dt", [
    (320, 320, 32, 32, 32, 2, "bf16"),
    (1280, 1280, 64, 12, 12, 1, "bf16"),
    (640, 320, 20, 16, 16, 2, "f16"),
])
def test_channels_last_wide_module_matches_reference_ops(Ci, Co, r, Hh, Ww, B, dt, path_log):
    m, x, gy_c, ref = _module_case(Ci, Co, 3, r, Hh, Ww, B, dt)
    _check_module(m, x, gy_c, ref, dt)
    M = B * Hh * Ww
    assert [e_ for e_ in path_log if e_[1].startswith("conv3")] == [("fwd", "conv3_nhwc_wide", M, Ci * 9, Co, r),
                                                                   ("bwd", "conv3_nhwc_wide", M, Ci * 9, Co, r)], path_log


# ----------------------------------------------------------------------------- (5) selector and sink
def test_wide_module_with_selector_and_through_a_sink(path_log):
    """Rank 24 with ``set_selector_from_diag`` against the reference op sequence; the same site with its gradients leaving
    through a trainer's GradSink gives the gradients of the plain autograd route (same kernels: the fold differs)."""
    Ci, Co, r, Hh, Ww, B, dt = 128, 64, 24, 16, 16, 2, "bf16"
    m, x, gy_c, _ = _module_case(Ci, Co, 3, r, Hh, Ww, B, dt)
    diag = torch.linspace(0.5, 1.5, r)
    m.set_selector_from_diag(diag)
    xr = x.detach().float().cpu().requires_grad_(True)
    dn = m.lora_down.weight.detach().cpu().clone().requires_grad_(True)
    upw = m.lora_up.weight.detach().cpu().clone().requires_grad_(True)
    yr = TR.conv_adapter_forward(xr, m.conv.weight.detach().float().cpu(), m.conv.bias.detach().float().cpu(), dn, upw, 0.8,
                                 1, 1, 1, 1, selector=torch.diag(diag).reshape(r, r, 1, 1))
    (yr * gy_c).sum().backward()
    _check_module(m, x, gy_c, (yr.detach(), xr.grad, dn.grad, upw.grad), dt)
    assert ("fwd", "conv3_nhwc_wide", B * Hh * Ww, Ci * 9, Co, r) in path_log
    plain = (n(m.lora_up.weight.grad).copy(), n(m.lora_down.weight.grad).copy(), n(x.grad).copy())
    m.lora_up.weight.grad = m.lora_down.weight.grad = None
    st = T.FlatLoraState([{"params": [m.lora_up.weight, m.lora_down.weight], "lr": 1e-3}], device=torch.device(DEV))
    assert st.attach_direct_grads(m) == 1
    x2 = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    y = m(x2)
    (y.float() * gy_c.to(DEV)).sum().backward()
    st.reduce_pending()
    gu, gd = n(st.flat_g[:Co * r]).reshape(Co, r, 1, 1), n(st.flat_g[Co * r:]).reshape(r, Ci, 3, 3)
    assert np.abs(n(x2.grad) - plain[2]).max() <= 2.0 ** -7 * np.abs(plain[2]).max()
    np.testing.assert_allclose(gu, plain[0], rtol=1e-5, atol=1e-6 * np.abs(plain[0]).max())
    np.testing.assert_allclose(gd, plain[1], rtol=1e-5, atol=1e-6 * np.abs(plain[1]).max())
    # a second backward accumulates (beta 1 into the flat buffer)
    y = m(x2)
    (y.float() * gy_c.to(DEV)).sum().backward()
    st.reduce_pending()
    np.testing.assert_allclose(n(st.flat_g[Co * r:]).reshape(r, Ci, 3, 3), 2 * plain[1], rtol=1e-5,
                               atol=2e-6 * np.abs(plain[1]).max())
    m.__dict__.pop("_grad_sink", None)


# ----------------------------------------------------------------------------- (6) dropout
def test_wide_module_with_dropout_under_the_restated_mask(monkeypatch, path_log):
    Ci, Co, r, Hh, Ww, B, dt, p, s_ = 128, 192, 40, 12, 20, 2, "bf16", 0.1, 0.8
    seed, off = 0x5EED0042, 991
    monkeypatch.setattr(ops, "next_dropout_stream", lambda device: (seed, off))
    m, x, gy_c, _ = _module_case(Ci, Co, 3, r, Hh, Ww, B, dt, p=p)
    m.train()
    M = B * Hh * Ww
    up = m.lora_up.weight.data.clone()
    with torch.no_grad():
        m.lora_up.weight.data.zero_()
        y0 = m(x).detach().clone()
        m.lora_up.weight.data.copy_(up)
    y = m(x)
    assert y.is_contiguous(memory_format=torch.channels_last)
    (y.float() * gy_c.to(DEV)).sum().backward()
    assert ("fwd", "conv3_nhwc_wide", M, Ci * 9, Co, r) in path_log and ("bwd", "conv3_nhwc_wide", M, Ci * 9, Co, r) in path_log
    mask = H.philox_dropout_mask(M * Co, p, seed, off).view(M, Co).double()
    assert 0.05 < float((mask == 0).double().mean()) < 0.15
    x64, dn64 = x.detach().double().cpu(), m.lora_down.weight.detach().double().cpu()
    up64 = up.double().cpu().view(Co, r)
    T64 = torch.nn.functional.conv2d(x64, dn64, None, 1, 1).permute(0, 2, 3, 1).reshape(M, r)
    rows = lambda t_: t_.detach().double().cpu().permute(0, 2, 3, 1).reshape(M, -1)  # noqa: E731
    want = rows(y0) + s_ * mask * (T64 @ up64.t())
    e = 2.0 ** -7
    assert float((rows(y) - want).abs().max()) <= e * float(want.abs().max()) + 1e-3
    Gm = rows(gy_c.to(DT[dt])) * mask
    d_up = s_ * (Gm.t() @ T64)
    gt = (s_ * (Gm @ up64)).view(B, Hh, Ww, r).permute(0, 3, 1, 2).contiguous()
    d_down = torch.nn.grad.conv2d_weight(x64, (r, Ci, 3, 3), gt, padding=1)
    for name, got, wanted in (("ddown", m.lora_down.weight.grad, d_down), ("dup", m.lora_up.weight.grad.view(Co, r), d_up)):
        err = float((got.double().cpu() - wanted).abs().max() / wanted.abs().max())
        assert err <= 4e-3, (name, err)


# ----------------------------------------------------------------------------- (7) switch off
def test_switch_off_takes_the_library_route(monkeypatch, path_log):
    """``ops.CONV3_WIDE = False``: the site goes where it went before the wide kernels — the frozen conv + ``lora_conv_branch``
    (library down-projection under autograd, NCHW up-projection kernel), which writes nothing to PATH_LOG for the conv site
    itself; the result leaves NCHW-contiguous and matches the reference at the same bounds."""
    monkeypatch.setattr(ops, "CONV3_WIDE", False)
    Ci, Co, r, Hh, Ww, B, dt = 320, 320, 32, 16, 16, 2, "bf16"
    m, x, gy_c, ref = _module_case(Ci, Co, 3, r, Hh, Ww, B, dt)
    _check_module(m, x, gy_c, ref, dt, channels_last=False)
    print(f"\n[conv3_wide off] PATH_LOG: {sorted(set((ph, path) for ph, path, *_ in path_log))}")
    assert not any(path.startswith("conv3_nhwc") for _, path, *_ in path_log), path_log


# ----------------------------------------------------------------------------- per-sample forward
@pytest.mark.parametrize("r", [24, 64])
def test_per_sample_forward_of_a_wide_3x3_site(r, path_log):
    """tests/test_gpu_per_sample.py::test_conv_sites_per_sample_match_oracle's channels-last 3x3 case at wide ranks: the
    per-sample table (3 rows over 6 samples) multiplies T between the wide down kernel and the rank update."""
    from tests.test_gpu_per_sample import _conv_case, _rows

    nsel = 3
    m, x = _conv_case("nhwc", 3, r, nsel)
    holder = torch.nn.Sequential(m)
    rows = _rows(nsel, r, seed=7)
    L.set_lora_diag_per_sample(holder, rows)
    with torch.no_grad():
        y = m(x)
        y2 = m(x)   # the cached pack
    assert y.shape == (x.shape[0], 96, 16, 16) and torch.equal(y, y2)
    assert [p_ for _, p_, *_ in path_log] == ["ps_conv3_nhwc", "ps_conv3_nhwc"] and path_log[0][5] == r
    X, W, Bv, A, U = n(x), n(m.conv.weight), n(m.conv.bias), n(m.lora_down.weight), n(m.lora_up.weight)
    for b in range(x.shape[0]):
        S = np.diag(n(rows)[b % nsel])
        want, _ = O.lora_conv2d_forward(X[b:b + 1], W, Bv, A, U, 0.6, padding=(1, 1), selector=S)
        absref, _ = O.lora_conv2d_forward(np.abs(X[b:b + 1]), np.abs(W), np.abs(Bv), np.abs(A), np.abs(U), 0.6,
                                          padding=(1, 1), selector=np.abs(S))
        close(n(y[b:b + 1]), want, absref, "bf16", k=4e-3, msg=f"rank {r} sample {b}")


# ----------------------------------------------------------------------------- (8) / (9) the step
P_LIN = 0.1


def _is3(m):
    return isinstance(m, L.LoraInjectedConv2d) and tuple(m.conv.kernel_size) == (3, 3)


def _twins(r):
    """The small stand-in UNet (channels-last, bf16) with the extended injection at rank r and its f32 oracle twin; dropout
    0.1 on the Linear adapters of both, 0 on the Conv2d adapters of both (module docstring)."""
    torch.manual_seed(0)
    base = UNet2DConditionModel(block_out_channels=(64, 128, 128), layers_per_block=1, attention_heads=2,
                                cross_attention_dim=64, norm_num_groups=8)
    base.requires_grad_(False)
    for q in base.parameters():
        q.data = q.data.bfloat16().float()
    ref = copy.deepcopy(base)
    torch.manual_seed(5)
    ref_params = TR.inject(ref, L.UNET_EXTENDED_TARGET_REPLACE, r=r, dropout_p=P_LIN, conv=True)
    for s_ in TR.sites_of(ref):
        s_.up.data.normal_(0, 0.02)
        if isinstance(s_, TR.RefConvSite):
            s_.p = 0.0
    dev = base.to(DEV).to(torch.bfloat16).to(memory_format=torch.channels_last)
    L.inject_trainable_lora_extended(dev, r=r)
    T.promote_lora_to_fp32(dev)
    ours = [m for m in dev.modules() if isinstance(m, (L.LoraInjectedLinear, L.LoraInjectedConv2d))]
    theirs = TR.sites_of(ref)
    assert len(ours) == len(theirs) > 0
    for a, b in zip(ours, theirs):
        assert isinstance(a, L.LoraInjectedConv2d) == isinstance(b, TR.RefConvSite)
        if isinstance(a, L.LoraInjectedConv2d):
            a.dropout.p = 0.0
        assert a.dropout.p == b.p
        a.lora_up.weight.data.copy_(b.up.data.view_as(a.lora_up.weight))
        a.lora_down.weight.data.copy_(b.down.data.view_as(a.lora_down.weight))
    ref.to(DEV)
    ref.train(), dev.train()
    assert sum(_is3(m) for m in ours) >= 8
    return ref, ref_params, dev, ours, theirs


def _batch():
    g = torch.Generator().manual_seed(42)
    B = 2
    lat = (torch.randn(B, 4, 32, 32, generator=g) * 0.18215).to(torch.bfloat16).float().to(DEV)
    ehs = torch.randn(B, 77, 64, generator=g).to(torch.bfloat16).float().to(DEV)
    noise = torch.randn(B, 4, 32, 32, generator=g).to(torch.bfloat16).float().to(DEV)
    return lat, ehs, noise, torch.tensor([100, 700], device=DEV)


def _release(dev):
    for m in dev.modules():
        m.__dict__.pop("_grad_sink", None)
        m.__dict__.pop("_merged", None)
        m.__dict__.pop("_forward_device", None)


def _tap(mod, current, log, routes):
    """Note which site is running (for the dropout draws) and what it wrote to PATH_LOG in its forward."""
    inner = mod._forward_device

    def run(x, *a, **kw):
        current[0] = mod
        at = len(log)
        out = inner(x, *a, **kw)
        routes.setdefault(id(mod), []).extend(path for ph, path, *_ in log[at:] if ph == "fwd")
        return out
    mod.__dict__["_forward_device"] = run


def _cl16(t):
    return t.bfloat16().contiguous(memory_format=torch.channels_last)


def _eager_steps(r):
    ref, ref_params, dev, ours, theirs = _twins(r)
    lat, ehs, noise, ts = _batch()
    sched = DDPMScheduler()
    current, draws = [None], {}
    orig = ops.next_dropout_stream

    def recording(device):
        seed, off = orig(device)
        draws.setdefault(id(current[0]), []).append((seed, off))
        return seed, off

    lin = [m for m in ours if isinstance(m, L.LoraInjectedLinear)]
    res, seen = {}, {}
    saved = ops.CONV3_WIDE
    for mode in (True, False):
        st = T.FlatLoraState([{"params": T.lora_params(dev), "lr": 1e-4, "weight_decay": 1e-2}], max_grad_norm=1.0, device=torch.device(DEV))
        st.attach_direct_grads(dev)
        mw = st.enable_merged_weights(dev)
        ops.PATH_LOG = log = []
        routes = {}
        for m in ours:
            _tap(m, current, log, routes)
        ops.CONV3_WIDE, ops.next_dropout_stream = mode, recording
        try:
            for _ in range(3):   # the host model's layouts settle in the first two; the third is the step
                draws.clear()
                routes.clear()
                del log[:]
                st.zero_grad()
                torch.manual_seed(7)
                T.forward_backward(dev, sched, _cl16(lat), ehs.bfloat16(), T.StepConfig(), noise=_cl16(noise), timesteps=ts, merged=mw)
                st.reduce_pending()
            torch.cuda.synchronize()
            got = st.flat_g.double().clone()
        finally:
            ops.CONV3_WIDE, ops.next_dropout_stream, ops.PATH_LOG = saved, orig, None
            _release(dev)
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
        assert all(len(draws.get(id(m), [])) == 1 for m in lin), "one dropout draw per Linear site and forward"
        assert not any(id(m) in draws for m in ours if isinstance(m, L.LoraInjectedConv2d))
        seen[mode] = [(draws[id(m)][0][0], int(draws[id(m)][0][1].item())) for m in lin]
        res[mode] = (got, [tuple(routes.get(id(m), [])) for m in ours if _is3(m)])
        del st, mw
    assert seen[True] == seen[False], "both settings ran on the same dropout draws"

    def pre_hook(site, draw):
        def hook(mod, args):
            x = args[0]
            N = mod.up.shape[0]
            rows = x.numel() // x.shape[-1]
            mod.mask = H.philox_dropout_mask(rows * N, P_LIN, draw[0], draw[1], DEV).view(*x.shape[:-1], N)
        return site.register_forward_pre_hook(hook)

    hooks = [pre_hook(s_, d) for s_, d in zip([s_ for s_ in theirs if isinstance(s_, TR.RefLinearSite)], seen[True])]
    with H.oracle_on_device():
        _, _, g32 = H.oracle_step_on_device(ref, ref_params, lat, noise, ts, ehs, False)
    for h in hooks:
        h.remove()
    want = torch.cat([g_.reshape(-1) for g_ in g32]).double()
    out = {mode: (float((got - want).norm()), routes) for mode, (got, routes) in res.items()}
    T._CKPT_CAND.pop(id(dev), None)
    del ref, ref_params, dev, ours, theirs, res
    gc.collect()
    torch.cuda.empty_cache()
    return out, float(want.norm())


def test_eager_step_of_the_extended_injection_takes_the_wide_route_and_stays_at_the_oracle():
    """One eager step at rank 24 with ``ops.CONV3_WIDE`` on and off, on the same dropout draws, both against the f32 oracle
    step handed those draws: every 3x3 site logs the wide route when on and none when off; the flat LoRA gradient with the
    switch on is no further from the oracle than CONV3_WIDE_RATIO_BOUND x the same with it off."""
    r = 24
    res, norm = _eager_steps(r)
    (e_on, routes_on), (e_off, routes_off) = res[True], res[False]
    print(f"\n[conv3_wide step] rank {r}: on {e_on:.4e} off {e_off:.4e} (‖oracle‖ {norm:.4e}) ratio {e_on / e_off:.3f}; "
          f"{len(routes_on)} 3x3 sites; routes off: {sorted(set(routes_off))}")
    assert routes_on and all(q == ("conv3_nhwc_wide",) for q in routes_on), sorted(set(routes_on))
    assert not any("conv3_nhwc_wide" in q for q in routes_off), sorted(set(routes_off))
    assert e_off < 0.1 * norm, "the oracle was handed the device's masks"
    assert e_on <= CONV3_WIDE_RATIO_BOUND * e_off, (f"‖on − oracle‖ {e_on:.4e} > {CONV3_WIDE_RATIO_BOUND} x ‖off − oracle‖ {e_off:.4e}")


def test_captured_step_of_the_extended_injection_replays_on_the_wide_route():
    """Rank 24 through trainer.GraphedForwardBackward, replayed twice: finite non-zero gradients, every 3x3 site on the wide
    route (nothing the route needs first appears inside the capture)."""
    r = 24
    ref, ref_params, dev, ours, _ = _twins(r)
    del ref, ref_params
    lat, ehs, noise, ts = _batch()
    sched = DDPMScheduler()
    st = T.FlatLoraState([{"params": T.lora_params(dev), "lr": 1e-4, "weight_decay": 1e-2}], max_grad_norm=1.0, device=torch.device(DEV))
    st.attach_direct_grads(dev)
    mw = st.enable_merged_weights(dev)
    assert ops.CONV3_WIDE
    ops.PATH_LOG = log = []
    n3 = sum(_is3(m) for m in ours)
    try:
        def fwd_bwd(lat_, cond_):
            return T.forward_backward(dev, sched, lat_, cond_, T.StepConfig(), noise=_cl16(noise), timesteps=ts, merged=mw)

        graphed = T.GraphedForwardBackward(fwd_bwd, _cl16(lat), ehs.bfloat16(), st)
        grads = []
        for _ in range(2):
            st.zero_grad()
            graphed(_cl16(lat), ehs.bfloat16())
            torch.cuda.synchronize()
            grads.append(st.flat_g.double().clone())
    finally:
        ops.PATH_LOG = None
        _release(dev)
    for g_ in grads:
        assert bool(torch.isfinite(g_).all()) and float(g_.abs().max()) > 0
    fwd3 = [path for ph, path, _, K, _, rr in log if ph == "fwd" and rr == r and path.startswith("conv3")]
    assert fwd3 and len(fwd3) % n3 == 0 and set(fwd3) == {"conv3_nhwc_wide"}, sorted(set(fwd3))
    bwd3 = [path for ph, path, _, K, _, rr in log if ph == "bwd" and path == "conv3_nhwc_wide"]
    assert len(bwd3) == len(fwd3)
    del graphed, st, mw, fwd_bwd
    T._CKPT_CAND.pop(id(dev), None)
    del dev, ours
    gc.collect()
    torch.cuda.empty_cache()
