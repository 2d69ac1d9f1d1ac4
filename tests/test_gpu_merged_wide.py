"""Maskless Linear adapters of rank 17..64 on the step's merged weights (``ops.MERGED_WIDE``).

The kernel (csrc/merge_step.hip, merge_step_wide_kernel) behind ``lora_amd_merge_step``: (a) against ``oracle.collapse`` in
every layout the narrow kernel writes, (b) tied to the narrow kernel bit for bit through zero-padded ranks (fma(0, x, p) = p:
the chains are the same), (c) the four tile geometries, (d) sites sharing one buffer, (e) its memory footprint — registered
with tests/test_gpu_footprint.py's registry.  The route: (f) ``LoraInjectedLinear`` and a q / k / v group on
``ops.MergedWeights`` against the oracle, with and without a gradient sink, (g) one captured step of a small stand-in UNet
with the switch on and off against the f32 oracle step.

What (g) builds is released when it is done (the trainer's per-model cache entry, the captured graphs and their pools):
the file leaves no device memory behind for the files that run after it."""
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
from tests.test_gpu_kernels import close, n, rnd
from tests.test_gpu_parity_r3 import _heads_pack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAY = (40, 64)

# (g): worst ‖on − f32 oracle‖ / ‖off − f32 oracle‖ of the flat LoRA gradient over ranks 24 and 64, measured on MI355X (first
# GPU visit): rank 24 1.003 (4.1237e-04 / 4.1114e-04), rank 64 1.062 (3.7130e-04 / 3.4973e-04); the same run's rank-16 ratio of
# the merged route over ``--merged 0``: 0.987 (4.6778e-04 / 4.7409e-04).  Bound = worst measured + 10 %
STEP_RATIO_BOUND = 1.17


def _merge(sites, alpha, rounding, tile=None):
    if tile is None:
        plan = _C.MergeStepPlan(sites)
    else:
        _C.merge_step_set_tuning(tile, -1)
        try:
            plan = _C.MergeStepPlan(sites)
        finally:
            _C.merge_step_set_tuning(2, -1)
    plan.launch(alpha, rounding)   # the plan carries its geometry
    return plan


def _bufs(N, K, rh, ch, dt, with_t=True, fill=9.0):
    np_, kp = ((N // rh[0]) * rh[1] if rh else N), ((K // ch[0]) * ch[1] if ch else K)
    out = torch.full((np_, kp), fill, dtype=dt, device=DEV)
    out_t = torch.full((kp, np_), fill, dtype=dt, device=DEV) if with_t else None
    return out, out_t


def _logical(out, N, K, rh, ch, fill=9.0):
    """The written elements of a head-padded scratch weight; the pads must still hold ``fill``."""
    got = out
    if rh:
        v = got.view(N // rh[0], rh[1], got.shape[1])
        assert torch.all(v[:, rh[0]:, :] == fill)
        got = v[:, :rh[0], :].reshape(N, got.shape[1])
    if ch:
        v = got.view(N, K // ch[0], ch[1])
        assert torch.all(v[:, :, ch[0]:] == fill)
        got = v[:, :, :ch[0]].reshape(N, K)
    return got


# ----------------------------------------------------------------------------- (a) oracle
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("N,K,r", [(136, 72, 17), (320, 320, 32), (328, 72, 33), (640, 320, 48), (320, 768, 64)])
def test_wide_merge_step_vs_oracle(N, K, r, dt):
    """lora.py:635-669 through lora_amd_merge_step at ranks 17..64 (ROUND_ONCE): dense, head-padded rows and head-padded
    columns (every layout whose head size 40 divides the shape), with and without the transposed output — W_eff^T is the
    transpose bit for bit, both equal oracle.collapse within one rounding, pads keep their sentinel."""
    w = rnd((N, K), dt, 0.05, seed=1)
    up, down = rnd((N, r), "f32", 0.3, seed=2), rnd((r, K), "f32", 0.3, seed=3)
    want = O.collapse(n(w), n(up), n(down), 0.7)
    bound = 2.0 ** (-8 if dt == "bf16" else -10) * np.abs(want).max()
    layouts = [(None, None)] + ([(LAY, None)] if N % LAY[0] == 0 else []) + ([(None, LAY)] if K % LAY[0] == 0 else [])
    for rh, ch in layouts:
        ref = None
        for with_t in (True, False):
            out, out_t = _bufs(N, K, rh, ch, w.dtype, with_t)
            _merge([dict(w=w, up=up, down=down, out=out, out_t=out_t, row_heads=rh, col_heads=ch, key=7)], 0.7, _C.ROUND_ONCE)
            if with_t:
                assert torch.equal(out_t, out.t()), (rh, ch)
            got = _logical(out, N, K, rh, ch)
            err = np.abs(n(got) - want).max()
            assert err <= bound, (rh, ch, with_t, err, bound)
            assert ref is None or torch.equal(out, ref), (rh, ch)   # the transposed output changes nothing in W_eff
            ref = out


# ----------------------------------------------------------------------------- (b) tie to the narrow kernel
@pytest.mark.parametrize("N,K,rh,ch", [(328, 72, None, None), (640, 320, LAY, None), (320, 320, None, LAY)])
def test_zero_padded_ranks_give_the_bits_of_the_rank_16_kernel(N, K, rh, ch):
    """A rank-16 site whose factors are zero-padded to rank 32 / 64 runs the chunked kernel and must give the rank-16
    kernel's bits, nearest-even and dithered (same key): both form fmaf(up_j, down_j, p) in rank order from p = 0, and the
    padded ranks add fma(0, x, p) = p."""
    for dt in ("bf16", "f16"):
        w = rnd((N, K), dt, 0.05, seed=1)
        up, down = rnd((N, 16), "f32", 0.3, seed=2), rnd((16, K), "f32", 0.3, seed=3)
        for rounding in (_C.ROUND_ONCE, _C.ROUND_DITHER):
            out16, out16_t = _bufs(N, K, rh, ch, w.dtype)
            p16 = _merge([dict(w=w, up=up, down=down, out=out16, out_t=out16_t, row_heads=rh, col_heads=ch, key=11)], 0.7, rounding)
            assert p16.rank_max == 16
            for r in (32, 64):
                up_p = torch.zeros(N, r, device=DEV)
                up_p[:, :16] = up
                down_p = torch.zeros(r, K, device=DEV)
                down_p[:16] = down
                out, out_t = _bufs(N, K, rh, ch, w.dtype)
                pw = _merge([dict(w=w, up=up_p, down=down_p, out=out, out_t=out_t, row_heads=rh, col_heads=ch, key=11)], 0.7, rounding)
                assert pw.rank_max == r
                assert torch.equal(out, out16) and torch.equal(out_t, out16_t), (dt, rounding, r)


# ----------------------------------------------------------------------------- (c) tile geometries
def test_wide_tile_geometries_agree():
    """All four geometries of merge_step_set_tuning write the same bits at rank 33 — nearest-even and dithered — on dense,
    ragged and head-padded sites (the 128 x 128 and 256 x 64 tiles take two passes of the chunked kernel, the others one)."""
    r = 33
    for N, K, rh, ch in [(320, 320, None, None), (328, 72, None, None), (640, 320, LAY, None), (264, 640, None, (80, 128))]:
        w = rnd((N, K), "bf16", 0.05, seed=1)
        up, down = rnd((N, r), "f32", 0.02, seed=2), rnd((r, K), "f32", 0.02, seed=3)
        for rounding in (_C.ROUND_ONCE, _C.ROUND_DITHER):
            res = []
            for tile in range(4):
                out, out_t = _bufs(N, K, rh, ch, w.dtype)
                _merge([dict(w=w, up=up, down=down, out=out, out_t=out_t, row_heads=rh, col_heads=ch, key=5)], 0.7, rounding, tile)
                assert torch.equal(out_t, out.t())
                res.append(out)
            for tile in range(1, 4):
                assert torch.equal(res[0], res[tile]), (N, K, rh, ch, rounding, tile)


# ----------------------------------------------------------------------------- (d) one buffer
def test_wide_sites_share_one_buffer():
    """Three wide sites (ranks 17, 32, 64 in ONE table) as row ranges of one scratch weight and column ranges of one
    transposed buffer: each range equals the site merged alone."""
    K, lay = 320, LAY
    ranks = (17, 32, 64)
    ws = [rnd((320, K), "bf16", 0.05, seed=10 + i) for i in range(3)]
    ups = [rnd((320, r), "f32", 0.3, seed=20 + i) for i, r in enumerate(ranks)]
    downs = [rnd((r, K), "f32", 0.3, seed=30 + i) for i, r in enumerate(ranks)]
    cat = torch.zeros(3 * 512, K, dtype=torch.bfloat16, device=DEV)
    cat_t = torch.zeros(K, 3 * 512, dtype=torch.bfloat16, device=DEV)
    sites = [dict(w=w, up=u, down=d, out=cat[i * 512:(i + 1) * 512], out_t=cat_t[:, i * 512:(i + 1) * 512], row_heads=lay,
                  col_heads=None, key=i) for i, (w, u, d) in enumerate(zip(ws, ups, downs))]
    for rounding in (_C.ROUND_ONCE, _C.ROUND_DITHER):
        cat.zero_(), cat_t.zero_()
        assert _merge(sites, 1.0, rounding).rank_max == 64
        assert torch.equal(cat_t, cat.t())
        for i, (w, u, d) in enumerate(zip(ws, ups, downs)):
            one = torch.zeros(512, K, dtype=torch.bfloat16, device=DEV)
            _merge([dict(w=w, up=u, down=d, out=one, out_t=None, row_heads=lay, col_heads=None, key=i)], 1.0, rounding)
            assert torch.equal(cat[i * 512:(i + 1) * 512], one), (rounding, i)


# ----------------------------------------------------------------------------- (e) footprint
@FP.case("lora_amd_merge_step")
def case_merge_step_wide():
    """Wide sites of one table: N = 136 (one 8-row chunk past a tile), K = 72 (8 x 9: a ragged column tile), ranks 17 / 33 / 64,
    two of them side by side in ONE buffer with gap columns, head-padded rows and head-padded columns; both roundings.
    Guards intact, inputs poisoned, pads and gaps keep the sentinel, values equal the launch on plain allocations."""
    BF, F32 = FP.BF, FP.F32
    d, D = 8, 16
    for rounding in (_C.ROUND_ONCE, _C.ROUND_DITHER):
        pair = FP.out((2 * 136, 72 + 8), BF)              # two sites as row ranges, + 8 gap columns
        pair_t = FP.out((72, 2 * 136 + 16), BF)           # their transposes side by side, + 16 gap columns
        rows_h = FP.out((136 // d * D, 72), BF)           # head-padded rows
        rows_h_t = FP.out((72, 136 // d * D), BF)
        cols_h = FP.out((136, 72 // d * D), BF)           # head-padded columns, no transposed output
        spec = [(17, pair.data[:136, :72], pair_t.data[:, :136], None, None),
                (64, pair.data[136:, :72], pair_t.data[:, 136:272], None, None),
                (33, rows_h.data, rows_h_t.data, (d, D), None),
                (24, cols_h.data, None, None, (d, D))]
        sites, plain = [], []
        for i, (r, o, ot, rh, ch) in enumerate(spec):
            w, up, dn = FP.rnd((136, 72), BF, seed=i), FP.rnd((136, r), F32, 0.05, seed=10 + i), FP.rnd((r, 72), F32, 0.1, seed=20 + i)
            sites.append(dict(w=FP.inp(w), up=FP.inp(up), down=FP.inp(dn), out=o, out_t=ot, row_heads=rh, col_heads=ch, key=i + 1))
            po, pot = torch.full(o.shape, 9.0, dtype=BF, device=DEV), (torch.full(ot.shape, 9.0, dtype=BF, device=DEV) if ot is not None else None)
            plain.append(dict(w=w, up=up, down=dn, out=po, out_t=pot, row_heads=rh, col_heads=ch, key=i + 1))
        _C.MergeStepPlan(sites).launch(0.9, rounding)
        FP.check(pair, pair_t, rows_h, rows_h_t, cols_h, what="merge_step wide")
        _C.MergeStepPlan(plain).launch(0.9, rounding)
        torch.cuda.synchronize()
        MG.assert_untouched(pair.data[:, 72:], "wide pair gap columns")
        MG.assert_untouched(pair_t.data[:, 272:], "wide pair_t gap columns")
        for g_, p_ in zip(sites, plain):
            rh, ch = g_["row_heads"], g_["col_heads"]
            rows = FP.heads_cols(136, *rh) if rh else torch.arange(136, device=DEV)
            cols = FP.heads_cols(72, *ch) if ch else torch.arange(72, device=DEV)
            o, po = g_["out"], p_["out"]
            MG.assert_written(o[rows][:, cols], "merge_step wide W_eff")
            assert torch.equal(o[rows][:, cols], po[rows][:, cols]), "wide W_eff differs from the unguarded launch"
            want = FP.d64(p_["w"]) + 0.9 * FP.d64(p_["up"]) @ FP.d64(p_["down"])
            ref = FP.d64(p_["w"]).abs() + 0.9 * FP.d64(p_["up"]).abs() @ FP.d64(p_["down"]).abs()
            FP.close(o[rows][:, cols], want, ref, BF, k=2e-5, eps=2.0 ** -8 if rounding == _C.ROUND_ONCE else 2.0 ** -7,
                     msg=f"merge_step wide rounding {rounding}")
            keep = torch.ones(o.shape, dtype=torch.bool, device=DEV)
            keep[rows[:, None], cols[None, :]] = False
            MG.assert_untouched(o[keep], "merge_step wide pads")
            if g_["out_t"] is not None:
                ot = g_["out_t"]
                assert torch.equal(ot[cols][:, rows], o[rows][:, cols].t()), "wide W_eff^T differs from W_eff"
                keep_t = torch.ones(ot.shape, dtype=torch.bool, device=DEV)
                keep_t[cols[:, None], rows[None, :]] = False
                MG.assert_untouched(ot[keep_t], "merge_step wide transposed pads")


def test_footprint_case():
    assert "lora_amd_merge_step" in FP.covered() and "merge_step_wide" in FP.CASES
    torch.cuda.synchronize()
    case_merge_step_wide()
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- (f) the adapter on MergedWeights
@pytest.fixture
def path_log():
    ops.PATH_LOG = log = []
    yield log
    ops.PATH_LOG = None


def _adapter(K, N, r, s, seed):
    torch.manual_seed(seed)
    m = L.LoraInjectedLinear(K, N, False, r=r, dropout_p=0.0, scale=s).to(DEV).to(torch.bfloat16)
    m.linear.requires_grad_(False)
    T.promote_lora_to_fp32(m)
    m.lora_up.weight.data.normal_(0, 0.05)
    return m


@pytest.mark.parametrize("in_heads,out_heads", [(None, None), (None, (8, 40, 64)), ((8, 40, 64), None)])
@pytest.mark.parametrize("r", [17, 32, 64])
def test_wide_adapter_on_merged_weights_vs_oracle(r, in_heads, out_heads, path_log):
    """lora.py:53-58 + autograd at ranks 17..64 with the adapter on ops.MergedWeights: the route is the merged one (forward
    and input gradient = dense GEMMs on the scratch weights, factor gradients on the primitives), y and dX within the bounds
    of the rank <= 16 test (test_gpu_parity_r3), pad columns exactly zero, dUp / dDown within the colreduce tests' bound of
    oracle.lora_linear_backward — returned to autograd, and accumulated (beta = 1) into a gradient sink."""
    M, K, N, s = 300, 320, 320, 0.8
    m = _adapter(K, N, r, s, 0)
    m.__dict__["_merged"] = mw = ops.MergedWeights()
    x, gy = rnd((M, K), "bf16", seed=5), rnd((M, N), "bf16", seed=6)
    X, G = n(x), n(gy)
    W, A, U = n(m.linear.weight), n(m.lora_down.weight), n(m.lora_up.weight)
    xd = (torch.from_numpy(_heads_pack(X, in_heads)).to(DEV).bfloat16() if in_heads else x).requires_grad_(True)
    gd = torch.from_numpy(_heads_pack(G, out_heads)).to(DEV).bfloat16() if out_heads else gy
    yo, _ = O.lora_linear_forward(X, W, None, A, U, s)
    dxo, ddo, duo, _, _ = O.lora_linear_backward(G, X, W, A, U, s)
    absu, absd = s * (np.abs(G).T @ (np.abs(X) @ np.abs(A).T)), (s * np.abs(G) @ np.abs(U)).T @ np.abs(X)
    for rep in range(3):  # 1: through refresh()'s batched plan; 2: into a gradient sink that already holds ones
        mw.refresh()
        xd.grad = None
        m.lora_up.weight.grad = m.lora_down.weight.grad = None
        sink = None
        if rep == 2:
            sink = ops.GradSink(torch.ones(r, K, device=DEV), torch.ones(N, r, device=DEV))
            m.__dict__["_grad_sink"] = sink
        del path_log[:]
        y = m.forward_heads(xd, in_heads, out_heads)
        y.backward(gd)
        fwd = [p for ph, p, *_ in path_log if ph == "fwd"]
        bwd = [p for ph, p, *_ in path_log if ph == "bwd"]
        assert fwd == ["merged_heads" if (in_heads or out_heads) else "merged"] and bwd == ["merged_dx+factors_primitives"], path_log
        assert path_log[0][2:] == (M, K, N, r)
        yv, dxv = n(y), n(xd.grad)
        if out_heads:
            h, d, D = out_heads
            assert np.all(yv.reshape(M, h, D)[:, :, d:] == 0)
            yv = yv.reshape(M, h, D)[:, :, :d].reshape(M, N)
        if in_heads:
            h, d, D = in_heads
            assert np.all(dxv.reshape(M, h, D)[:, :, d:] == 0)
            dxv = dxv.reshape(M, h, D)[:, :, :d].reshape(M, K)
        absy = np.abs(X) @ (np.abs(W) + s * np.abs(U) @ np.abs(A)).T
        assert np.all(np.abs(yv - yo) <= 2.0 ** -8 * absy + 2.0 ** -8 * np.abs(yo) + 1e-3), rep
        absdx = np.abs(G) @ (np.abs(W) + s * np.abs(U) @ np.abs(A))
        assert np.all(np.abs(dxv - dxo) <= 2.0 ** -8 * absdx + 2.0 ** -8 * np.abs(dxo) + 1e-3), rep
        if sink is None:
            d_up, d_down, base = n(m.lora_up.weight.grad), n(m.lora_down.weight.grad), 0.0
        else:
            assert m.lora_up.weight.grad is None and m.lora_down.weight.grad is None and sink.pending is None
            d_up, d_down, base = n(sink.up_grad), n(sink.down_grad), 1.0
        close(d_up, duo + base, absu + base, "f32", msg=f"dUp rep {rep}")
        close(d_down, ddo + base, absd + base, "f32", msg=f"dDown rep {rep}")
    assert mw.refreshes == 2 and len(mw.entries) == 1 and mw._plans[0][0].rank_max == r


@pytest.mark.parametrize("out_heads", [None, (8, 40, 64)])
def test_wide_group_of_sites_on_one_input_vs_oracle(out_heads, path_log):
    """to_q / to_k / to_v at rank 32 through lora.lora_linear_group with the adapters on ops.MergedWeights (one concatenated
    scratch weight, one forward GEMM): outputs, the summed input gradient and every factor gradient vs the oracle."""
    M, K, N, r, s = 300, 320, 320, 32, 1.0
    mw = ops.MergedWeights()
    mods = [_adapter(K, N, r, s, 1 + i) for i in range(3)]
    for m in mods:
        m.__dict__["_merged"] = mw
    x = rnd((M, K), "bf16", seed=7).requires_grad_(True)
    gs = [rnd((M, N), "bf16", seed=8 + i) for i in range(3)]
    outs = L.lora_linear_group(mods, x, out_heads=out_heads)
    assert outs is not None and len(outs) == 3 and len(mw.groups) == 1
    gd = [torch.from_numpy(_heads_pack(n(g), out_heads)).to(DEV).bfloat16() if out_heads else g for g in gs]
    torch.autograd.backward(outs, gd)
    tag = "merged_group_cat" + ("_heads" if out_heads else "")
    assert [p for ph, p, *_ in path_log if ph == "fwd"] == [tag] * 3, path_log
    assert [p for ph, p, *_ in path_log if ph == "bwd"] == ["merged_group_dx+factors_primitives"] * 3, path_log
    X = n(x)
    dx_sum, absdx = 0.0, 0.0
    for m, y, g in zip(mods, outs, gs):
        W, A, U, G = n(m.linear.weight), n(m.lora_down.weight), n(m.lora_up.weight), n(g)
        yo, _ = O.lora_linear_forward(X, W, None, A, U, s)
        dxo, ddo, duo, _, _ = O.lora_linear_backward(G, X, W, A, U, s)
        yv = n(y)
        if out_heads:
            h, d, D = out_heads
            assert np.all(yv.reshape(M, h, D)[:, :, d:] == 0)
            yv = yv.reshape(M, h, D)[:, :, :d].reshape(M, N)
        absy = np.abs(X) @ (np.abs(W) + s * np.abs(U) @ np.abs(A)).T
        assert np.all(np.abs(yv - yo) <= 2.0 ** -8 * absy + 2.0 ** -8 * np.abs(yo) + 1e-3)
        dx_sum = dx_sum + dxo
        absdx = absdx + np.abs(G) @ (np.abs(W) + s * np.abs(U) @ np.abs(A))
        close(n(m.lora_up.weight.grad), duo, s * (np.abs(G).T @ (np.abs(X) @ np.abs(A).T)), "f32", msg="dUp")
        close(n(m.lora_down.weight.grad), ddo, (s * np.abs(G) @ np.abs(U)).T @ np.abs(X), "f32", msg="dDown")
    # three bf16 roundings of the running sum (addmm_ accumulates in the output dtype)
    assert np.all(np.abs(n(x.grad) - dx_sum) <= 2.0 ** -8 * absdx + 3 * 2.0 ** -8 * np.abs(dx_sum) + 2e-3)


def test_what_the_wide_route_does_not_take(monkeypatch):
    """``merged_ok`` at rank 32: 16-bit weights in the compute dtype only — an f32 master (the chunked kernel has no f64
    re-formation of cancelling elements), f32 compute, a shape off the 16-byte chunks and the switch turned off keep today's
    route; rank 16 on a master is still taken."""
    def ok(r, wdt, xdt, N=320, K=320):
        m = L.LoraInjectedLinear(K, N, False, r=r).to(DEV).to(wdt)
        m.linear.requires_grad_(False)
        T.promote_lora_to_fp32(m)
        return ops.merged_ok(torch.zeros(4, K, dtype=xdt, device=DEV), m.linear.weight, m.lora_down.weight, m.lora_up.weight,
                             None, 0.0, None, None)

    bf, f32 = torch.bfloat16, torch.float32
    assert ok(32, bf, bf) and ok(64, torch.float16, torch.float16) and ok(17, bf, bf)
    assert ok(16, f32, bf) and not ok(32, f32, bf)
    assert not ok(32, f32, f32)
    assert not ok(32, bf, bf, N=324) and not ok(32, bf, bf, K=324)
    monkeypatch.setattr(ops, "MERGED_WIDE", False)
    assert not ok(32, bf, bf) and ok(16, bf, bf)


# ----------------------------------------------------------------------------- (g) one captured step
def _twins(r):
    """A small stand-in UNet twice (every Linear at least 64 wide, so that rank 64 is a legal rank): bf16 on the device with
    our adapters, f32 oracle twin with the reference-algorithm adapters; same (bf16-representable) frozen values, same factors."""
    torch.manual_seed(0)
    base = UNet2DConditionModel(block_out_channels=(64, 128, 128), layers_per_block=1, attention_heads=2,
                                cross_attention_dim=64, norm_num_groups=8)
    base.requires_grad_(False)
    for p in base.parameters():
        p.data = p.data.bfloat16().float()
    ref = copy.deepcopy(base)
    torch.manual_seed(5)
    ref_params = TR.inject(ref, L.UNET_DEFAULT_TARGET_REPLACE, r=r)
    for s_ in TR.sites_of(ref):
        s_.up.data.normal_(0, 0.02)
    dev = base.to(DEV).to(torch.bfloat16)
    L.inject_trainable_lora(dev, r=r)
    T.promote_lora_to_fp32(dev)
    ours, theirs = [m for m in dev.modules() if isinstance(m, L.LoraInjectedLinear)], TR.sites_of(ref)
    assert len(ours) == len(theirs) > 0
    for a, b in zip(ours, theirs):
        assert a.lora_up.weight.dtype == torch.float32 and a.lora_up.weight.shape == b.up.shape
        a.lora_up.weight.data.copy_(b.up.data)
        a.lora_down.weight.data.copy_(b.down.data)
    ref.to(DEV)
    ref.train(), dev.train()
    return ref, ref_params, dev


def _step_errors(r, modes):
    """One replayed step of the captured forward+backward per mode on ONE batch -> {mode: (‖flat gradient − f32 oracle‖, the
    (M, K, N) of the sites whose forward took the merged route)} and ‖oracle‖.  ``modes``: "merged" (MergedWeights, the
    switches as they stand), "wide_off" (MergedWeights with ops.MERGED_WIDE = False), "unmerged" (no MergedWeights)."""
    ref, ref_params, dev = _twins(r)
    g = torch.Generator().manual_seed(42)
    B = 2
    lat = (torch.randn(B, 4, 32, 32, generator=g) * 0.18215).to(torch.bfloat16).float().to(DEV)
    ehs = torch.randn(B, 77, 64, generator=g).to(torch.bfloat16).float().to(DEV)
    noise = torch.randn(B, 4, 32, 32, generator=g).to(torch.bfloat16).float().to(DEV)
    ts = torch.tensor([100, 700], device=DEV)
    with H.oracle_on_device():
        _, _, g32 = H.oracle_step_on_device(ref, ref_params, lat, noise, ts, ehs, False)
    want = torch.cat(g32).double()
    sched = DDPMScheduler()
    res = {}
    saved = ops.MERGED_WIDE
    for mode in modes:
        st = T.FlatLoraState([{"params": T.lora_params(dev), "lr": 1e-4, "weight_decay": 1e-2}], max_grad_norm=1.0, device=torch.device(DEV))
        st.attach_direct_grads(dev)
        assert [tuple(p.shape) for p in st.params] == [tuple(p.shape) for p in ref_params]
        mw = st.enable_merged_weights(dev) if mode != "unmerged" else None
        ops.MERGED_WIDE = saved and mode != "wide_off"
        ops.PATH_LOG = log = []
        try:
            def fwd_bwd(lat_, cond_):
                return T.forward_backward(dev, sched, lat_, cond_, T.StepConfig(), noise=noise.bfloat16(), timesteps=ts, merged=mw)

            graphed = T.GraphedForwardBackward(fwd_bwd, lat.bfloat16(), ehs.bfloat16(), st)
            st.zero_grad()
            graphed(lat.bfloat16(), ehs.bfloat16())
            torch.cuda.synchronize()
            got = st.flat_g.double().clone()
        finally:
            ops.MERGED_WIDE, ops.PATH_LOG = saved, None
            for m in dev.modules():
                m.__dict__.pop("_grad_sink", None)
                m.__dict__.pop("_merged", None)
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
        sites = {(M, K, N) for ph, path, M, K, N, _ in log if ph == "fwd" and path.startswith("merged")}
        other = {path for ph, path, *_ in log if ph == "fwd" and not path.startswith("merged")}
        res[mode] = (float((got - want).norm()), sites, other)
        del graphed, st, mw, fwd_bwd
    # nothing of this stays on the device: the trainer's per-model cache would keep the model alive, the captured graphs their pools
    T._CKPT_CAND.pop(id(dev), None)
    del ref, ref_params, dev
    gc.collect()
    torch.cuda.empty_cache()
    return res, float(want.norm())


@pytest.fixture(scope="module")
def rank16_step():
    """The reference point of (g): at rank 16, the merged route's gradient error over the per-site route's (``--merged 0``)."""
    res, norm = _step_errors(16, ("merged", "unmerged"))
    ratio = res["merged"][0] / res["unmerged"][0]
    print(f"\n[merged_wide step] rank 16: merged {res['merged'][0]:.4e} unmerged {res['unmerged'][0]:.4e} (‖oracle‖ {norm:.4e}) "
          f"ratio {ratio:.3f}; {len(res['merged'][1])} site shapes on the merged route")
    assert res["merged"][1] and not res["unmerged"][1]
    return ratio, res["merged"][1]


@pytest.mark.parametrize("r", [24, 64])
def test_captured_step_gradients_with_the_switch_on_and_off(r, rank16_step):
    """One step of a small stand-in UNet (bf16, trainer state, merged weights, hipGraph replay) at ranks 24 and 64 with
    ops.MERGED_WIDE on and off, from one seed: every site shape that takes the merged route at rank 16 takes it here (and none
    with the switch off), and the flat LoRA gradient is no further from the f32 oracle step (``helpers.oracle_on_device``) than
    STEP_RATIO_BOUND x the off route's (the measured ratios stand at STEP_RATIO_BOUND)."""
    ratio16, sites16 = rank16_step
    res, norm = _step_errors(r, ("merged", "wide_off"))
    (e_on, sites_on, other_on), (e_off, sites_off, other_off) = res["merged"], res["wide_off"]
    print(f"\n[merged_wide step] rank {r}: on {e_on:.4e} off {e_off:.4e} (‖oracle‖ {norm:.4e}) ratio {e_on / e_off:.3f}; "
          f"rank-16 ratio {ratio16:.3f}; off-route forward paths {sorted(other_off)}")
    assert sites16 <= sites_on, sorted(sites16 - sites_on)
    assert not sites_off and "lib+primitives" in other_off, (sites_off, other_off)
    assert e_on <= STEP_RATIO_BOUND * e_off, f"rank {r}: ‖on − oracle‖ {e_on:.4e} > {STEP_RATIO_BOUND} x ‖off − oracle‖ {e_off:.4e}"
