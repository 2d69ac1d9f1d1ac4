"""The masked matrix-core factor pass at LoRA ranks 17..64 (csrc/factor_mfma.hip, DROP and WIDE together; ``ops.WIDE_DROPOUT``).

nn.Dropout on the branch keeps a Linear site off the merged weights; its factor gradients still go to the step's deferred pass,
where every (row block, 16-rank slice) workgroup regenerates the forward's mask on G — indexed by G's own row and 8-column
chunk, so the slices of a row block see the same mask: (a) every slice's slab rows are bit for bit the masked rank-16 pass on
that slice; (b) the fold against ``oracle.lora_numpy.lora_linear_backward`` under the restated Philox mask; (c) the offset
held on the device; (d) masked and maskless sites of four slice counts in one launch; (e) the memory footprint (the case of
``lora_amd_linear_bwd_factors_mfma_ragged`` with both flag bits in tests/test_gpu_footprint.py's registry: it registers when this
module is imported, which a run of the whole suite does at collection); (f) the route of one adapter on a trainer's sink; (g) an eager step
and (h) a captured step of a small stand-in UNet with dropout on every site.

Shapes, geometry and helpers are tests/test_gpu_factors_wide.py's.  What (g) and (h) build is released when they are done."""
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
from tests import test_gpu_factors_wide as W
from tests import test_gpu_footprint as FP
from tests.test_gpu_kernels import close, n, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS, SHAPES, GEOMETRY, HEADS = W.DTS, W.SHAPES, W.GEOMETRY, W.HEADS
P, SEED, OFF = 0.1, 0x1234567, 40

# (g): worst ‖on − f32 oracle‖ / ‖off − f32 oracle‖ of the flat LoRA gradient over ranks 24 and 64, both settings on the SAME
# dropout draws, which the oracle twin is handed (``ops.WIDE_DROPOUT`` on: the deferred matrix-core pass; off: the primitives
# in every site's backward), measured on MI355X (first GPU visit, against the off setting = the parent's arithmetic): rank 24
# 0.987 (4.1047e-04 / 4.1585e-04), rank 64 1.027 (3.9375e-04 / 3.8351e-04), ‖oracle‖ 2.5e-02 / 2.3e-02.
# Bound = worst measured + 10 % = 1.027 x 1.10
WIDE_DROPOUT_RATIO_BOUND = 1.13


def _mask(M, N, p=P, seed=SEED, off=OFF):
    """The multiplier (0 or 1 / (1 - p)) of every element of the logical [M, N] G, restated (tests/helpers.py)."""
    return H.philox_dropout_mask(M * N, p, seed, off).view(M, N).numpy()


def _launch(sites, dt, s_, wide=True, off_dev=None):
    """W._launch with every site's dropout triple (``drop`` of the site: (p, seed, offset) or None) in the table; a group with a
    masked site is launched masked.  ``off_dev``: the offset rides in that device tensor instead of the table."""
    arr, total = _C.factor_pack_table([(s["down"], s["up"], s["pk_down"], s["pk_up"]) for s in sites])
    _C.factor_pack(_C.table_to_device(arr, DEV), len(sites), total, dt)
    by_cls = {}
    for s in sites:
        by_cls.setdefault((int(s["plan"].lds_class), int(s["plan"].rows_per_block)), []).append(s)
    for (cls, rpb), group in by_cls.items():
        rows = []
        for s in group:
            drop = s.get("drop")
            if drop is not None and off_dev is not None:
                drop = (drop[0], drop[1], off_dev)
            rows.append((s["g"], s["x"], s["pk_down"], s["pk_up"], s["up_part"], s["down_part"], s_, s["gh"], s["xh"], s["r"],
                         s["plan"], drop))
        arr, grid = _C.factors_mfma_table(rows, dt, cls)
        if wide:
            assert grid == sum(int(s["plan"].nparts) * W._ns(s["r"]) for s in group)
        masked = any(s.get("drop") is not None and s["drop"][0] > 0 for s in group)
        _C.linear_bwd_factors_mfma_ragged(_C.table_to_device(arr, DEV), len(group), grid, cls, dt, masked, rpb, wide=wide)
    return len(by_cls)


def _masked_site(*a, drop=(P, SEED, OFF), **kw):
    s = W._site(*a, **kw)
    s["drop"] = drop
    return s


_IDS = [f"{s[0]}x{s[1]}x{s[2]}{'g' if s[3] else ''}{'x' if s[4] else ''}" for s in SHAPES]


# ----------------------------------------------------------------------------- (a) bit tie
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("shape,geom", list(zip(SHAPES, GEOMETRY)), ids=_IDS)
def test_masked_wide_slab_rows_are_the_masked_rank_16_pass_on_each_slice(shape, geom, dt):
    """Rank 33, p = 0.1: rows [16 s, 16 s + min(16, r - 16 s)) of every row block's [16 ns][C] slab equal, bit for bit, the
    masked rank <= 16 pass on slice s as a zero-padded rank-16 site with the same (p, seed, offset) at the same block height:
    the mask does not depend on the slice.  Dead rows are exact zeros; the slabs start as NaN."""
    (M, K, N, gh, xh), (cls, rpb), r, dtype = shape, geom, 33, DTS[dt]
    w = _masked_site(M, K, N, r, gh, xh, dtype, seed=1, up_scale=1e-3)
    assert (int(w["plan"].lds_class), int(w["plan"].rows_per_block)) == (cls, rpb)
    assert bool(torch.isnan(w["up_part"]).all()) and bool(torch.isnan(w["down_part"]).all())
    _launch([w], dtype, 0.7)
    nparts, ns = int(w["plan"].nparts), W._ns(r)
    assert nparts == -(-M // rpb) and M % rpb
    up_w, down_w = w["up_part"].view(nparts, 16 * ns, N), w["down_part"].view(nparts, 16 * ns, K)
    for s in range(ns):
        d16, u16, rs = W._slice16(w["down"], w["up"], s)
        nw = _masked_site(M, K, N, 16, gh, xh, dtype, seed=1, wide=False, rows=rpb, factors=(d16, u16))
        assert (int(nw["plan"].lds_class), int(nw["plan"].rows_per_block), int(nw["plan"].nparts)) == (cls, rpb, nparts)
        _launch([nw], dtype, 0.7, wide=False)
        torch.cuda.synchronize()
        up_n, down_n = nw["up_part"].view(nparts, 16, N), nw["down_part"].view(nparts, 16, K)
        assert bool(torch.isfinite(up_n[:, :rs]).all()) and bool(torch.isfinite(down_n[:, :rs]).all())
        assert torch.equal(up_w[:, 16 * s:16 * s + rs].view(torch.int32), up_n[:, :rs].view(torch.int32)), (s, "up")
        assert torch.equal(down_w[:, 16 * s:16 * s + rs].view(torch.int32), down_n[:, :rs].view(torch.int32)), (s, "down")
    assert not bool(up_w[:, r:].any()) and not bool(down_w[:, r:].any())
    # and the mask is in effect: the maskless pass on the same site gives other bits
    plain = W._site(M, K, N, r, gh, xh, dtype, seed=1, up_scale=1e-3)
    W._launch([plain], dtype, 0.7)
    torch.cuda.synchronize()
    assert not torch.equal(plain["up_part"].view(torch.int32), w["up_part"].view(torch.int32))


# ----------------------------------------------------------------------------- (b) oracle
def _reference(s, s_):
    """The masked reference of a site, once: W._fold_and_check finds it in place and compares at k = 1e-4 of the absolute
    bound, which carries 1 / (1 - p) (tests/test_gpu_ws_heads.py::test_factor_pass_with_dropout_on_head_padded_rows)."""
    M, K, N = s["M"], s["K"], s["N"]
    drop = s.get("drop")
    p = drop[0] if drop else 0.0
    mask = _mask(M, N, *drop) if p > 0 else None
    if mask is not None and M * N >= 4096:
        assert abs(float((mask == 0).mean()) - p) < 0.05, float((mask == 0).mean())   # p = 0.1: 5 - 15 % of the mask is zero
    A, U = n(s["down"]), n(s["up"])
    _, s["ddo"], s["duo"], _, _ = O.lora_linear_backward(s["G"], s["X"], np.zeros((N, K), np.float32), A, U, s_, mask=mask)
    k = s_ / (1 - p)
    s["absu"] = k * (np.abs(s["G"]).T @ (np.abs(s["X"]) @ np.abs(A).T))
    s["absd"] = (k * np.abs(s["G"]) @ np.abs(U)).T @ np.abs(s["X"])
    return mask


@pytest.mark.parametrize("dt,up_scale", [("bf16", 0.3), ("f16", 0.3), ("f16", 1e-4)], ids=["bf16", "f16", "f16_up1e-4"])
@pytest.mark.parametrize("r", [17, 32, 33, 48, 64])
def test_masked_wide_pass_vs_oracle(r, dt, up_scale):
    """dB = s (mask .* G)^T (X A^T), dA = (s (mask .* G) B)^T X through the pack, the masked wide pass and the fold: every
    shape of (a) and M = 1, one launch per (class, height), folded with beta = 0 and beta = 1."""
    dtype, s_ = DTS[dt], 0.7
    sites = [_masked_site(M, K, N, r, gh, xh, dtype, seed=i, up_scale=up_scale)
             for i, (M, K, N, gh, xh) in enumerate(SHAPES + [(1, 320, 320, None, None)])]
    zeros = total = 0
    for s in sites:
        mask = _reference(s, s_)
        zeros, total = zeros + int((mask == 0).sum()), total + mask.size
    assert 0.05 < zeros / total < 0.15
    assert _launch(sites, dtype, s_) == 3
    for beta in (0.0, 1.0):
        W._fold_and_check(sites, s_, beta, f"masked {dt} up~{up_scale}")


# ----------------------------------------------------------------------------- (c) device-held offset
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_offset_on_the_device_gives_the_bits_of_the_host_offset(dt):
    dtype = DTS[dt]
    shapes = [SHAPES[0], SHAPES[1], SHAPES[3]]
    host = [_masked_site(M, K, N, 33, gh, xh, dtype, seed=i) for i, (M, K, N, gh, xh) in enumerate(shapes)]
    dev = [_masked_site(M, K, N, 33, gh, xh, dtype, seed=i) for i, (M, K, N, gh, xh) in enumerate(shapes)]
    _launch(host, dtype, 0.7)
    off_dev = torch.tensor([OFF], dtype=torch.int64, device=DEV)
    _launch(dev, dtype, 0.7, off_dev=off_dev)
    torch.cuda.synchronize()
    for a, b in zip(host, dev):
        for k in ("up_part", "down_part"):
            assert bool(torch.isfinite(a[k]).all()) and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


# ----------------------------------------------------------------------------- (d) mixed table
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_masked_and_maskless_sites_of_four_slice_counts_share_one_launch(dt):
    """Ranks 17, 64 and 33 masked (each with its own seed and offset) and a maskless rank 48 site in ONE table, one launch."""
    dtype, s_ = DTS[dt], 0.9
    sites = [_masked_site(300, 320, 320, 17, None, None, dtype, seed=1, drop=(P, SEED, OFF)),
             _masked_site(70, 64, 96, 64, None, None, dtype, seed=2, drop=(0.2, SEED + 1, OFF + 8)),
             _masked_site(129, 320, 320, 33, HEADS, None, dtype, seed=3, drop=(P, SEED + 2, 0)),
             _masked_site(65, 320, 320, 48, None, HEADS, dtype, seed=4, drop=None)]
    for s in sites:
        _reference(s, s_)
    assert _launch(sites, dtype, s_) == 1
    W._fold_and_check(sites, s_, 0.0, f"{dt} masked + maskless")


# ----------------------------------------------------------------------------- (e) footprint
@FP.case("lora_amd_linear_bwd_factors_mfma_ragged")
def case_factors_wide_masked():
    """W.WIDE_TABLE (ranks 17 / 33 / 64 / 33: M = 1, one row past a block, head-padded G and X, a 64 x 96 site) with dropout on
    every site but the last, bf16 and f16, with the block map: the pass writes exactly the 16 ns rows of every block's slab;
    guards intact, inputs poisoned (NaN head pads), values equal the launch on plain allocations and the dense formula under
    the restated mask."""
    for dt in (FP.BF, torch.float16):
        sites = [W._guarded_site(M, K, N, r, 10 * j + 1, dt, gh, xh) for j, (M, K, N, r, gh, xh) in enumerate(W.WIDE_TABLE)]
        drops = [(P, SEED + j, OFF + 8 * j) for j in range(len(sites) - 1)] + [None]
        plain = [dict(up_part=torch.zeros_like(s["up_part"].data), down_part=torch.zeros_like(s["down_part"].data)) for s in sites]
        arr, total = _C.factor_pack_table([(s["down"], s["up"], s["pk_down"].data, s["pk_up"].data) for s in sites])
        _C.factor_pack(FP.table(arr), len(sites), total, dt)
        assert {(int(s["plan"].lds_class), int(s["plan"].rows_per_block)) for s in sites} == {(1, 64)}
        for guarded in (True, False):
            bufs = [dict(up_part=s["up_part"].data, down_part=s["down_part"].data) for s in sites] if guarded else plain
            arr, grid = _C.factors_mfma_table(
                [(s["g"], s["x"], s["pk_down"].data, s["pk_up"].data, b["up_part"], b["down_part"], s["scale"], s["g_heads"],
                  s["x_heads"], s["r"], s["plan"], d) for s, b, d in zip(sites, bufs, drops)], dt, 1)
            raw, moff = _C.factors_mfma_table_bytes(arr, grid)
            tab = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
            _C.linear_bwd_factors_mfma_ragged(tab, len(sites), grid, 1, dt, True, 64, map_offset=moff, wide=True)
        FP.check(*[s[k] for s in sites for k in ("pk_down", "pk_up", "up_part", "down_part")], what="factors wide masked")
        for s, p_, d in zip(sites, plain, drops):
            nparts, RT = int(s["plan"].nparts), int(s["plan"].rank_tile)
            for k in ("up_part", "down_part"):
                MG.assert_written(s[k].data, f"masked wide {k}: all 16 ns rows of every block")
                assert torch.equal(s[k].data.view(torch.int32), p_[k].view(torch.int32)), f"{k} differs from the unguarded launch"
            ref = dict(s)
            if d is not None:   # the dense formula on mask .* G (the multiplier carries 1 / (1 - p))
                ref["g_log"] = FP.d64(s["g_log"]) * torch.from_numpy(_mask(s["M"], s["N"], *d)).to(DEV).double()
            FP._check_factor_grads(ref, s["up_part"], s["down_part"], nparts, RT, f"factors wide masked M={s['M']} r={s['r']}")


def test_footprint_case():
    assert "factors_wide_masked" in FP.CASES and "lora_amd_linear_bwd_factors_mfma_ragged" in FP.covered()
    torch.cuda.synchronize()
    case_factors_wide_masked()
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- (f) the route
@pytest.fixture
def recorded(monkeypatch):
    """PATH_LOG and every dropout draw (seed, offset tensor) of the test, in call order."""
    log, draws = [], []
    orig = ops.next_dropout_stream

    def recording(device):
        seed, off = orig(device)
        draws.append((seed, off))
        return seed, off

    monkeypatch.setattr(ops, "PATH_LOG", log)
    monkeypatch.setattr(ops, "next_dropout_stream", recording)
    return log, draws


def test_dropout_site_of_rank_32_on_a_trainers_sink(recorded, monkeypatch):
    """LoraInjectedLinear(320, 640, r = 32, dropout 0.1), bf16, on a trainer's sink (tests/test_gpu_ws_heads.py's set-up): with
    ``ops.WIDE_DROPOUT`` the backward is Gt and the rank update around the frozen GEMM and both factor gradients are the
    deferred pass's — nothing at all is launched when x takes no gradient; without it the primitives.  y and dX are the same
    bits in both; the flat gradient of each against a float64 evaluation under the same mask at the bounds of
    tests/test_gpu_r16_wide.py::test_wide_dropout_module_forward_backward_on_both_kernels."""
    log, draws = recorded
    r, p, B, S, K, N = 32, 0.1, 2, 77, 320, 640
    M = B * S
    x0, gy = rnd((B, S, K), "bf16", seed=5), rnd((B, S, N), "bf16", seed=6)

    def run(flag, need_x=True):
        monkeypatch.setattr(ops, "WIDE_DROPOUT", flag)
        torch.manual_seed(0)
        m = L.LoraInjectedLinear(K, N, True, r=r, dropout_p=p).to(DEV).to(torch.bfloat16)
        m.linear.requires_grad_(False)
        T.promote_lora_to_fp32(m)
        m.lora_up.weight.data.normal_(0, 0.05)
        m.train()
        holder = torch.nn.ModuleList([m])
        st = T.FlatLoraState([{"params": T.lora_params(holder), "lr": 1e-3, "weight_decay": 0.0}], max_grad_norm=0.0, device=DEV)
        st.attach_direct_grads(holder)
        mw = st.enable_merged_weights(holder)
        assert mw.defer_factors
        x = x0.clone().requires_grad_(need_x)
        del log[:], draws[:]
        with ops.dropout_pool(DEV):
            torch.manual_seed(99)   # the dropout stream of every run
            mw.refresh()
            y = m(x)
            y.backward(gy)
            mw.flush_factors()
        st.all_reduce()
        torch.cuda.synchronize()
        (seed, off), = draws
        return dict(m=m, y=y.detach().clone(), dx=x.grad.clone() if need_x else None, draw=(seed, int(off.item())),
                    d_up=st.grad_view(m.lora_up.weight).clone(), d_down=st.grad_view(m.lora_down.weight).clone(),
                    paths=[(ph, path) for ph, path, *_ in log], shape=log[0][2:])

    on, off_, nox = run(True), run(False), run(True, need_x=False)
    assert on["paths"] == [("fwd", "lib+primitives"), ("bwd", "rowdot+lib+rank_update+factors_deferred_mfma")], on["paths"]
    assert nox["paths"] == [("fwd", "lib+primitives"), ("bwd", "factors_deferred_mfma")], nox["paths"]
    assert off_["paths"] == [("fwd", "lib+primitives"), ("bwd", "primitives")], off_["paths"]
    assert on["shape"] == (M, K, N, r)
    assert on["draw"] == off_["draw"] == nox["draw"]
    assert torch.equal(on["y"], off_["y"]) and torch.equal(on["dx"], off_["dx"]) and torch.equal(on["y"], nox["y"])
    m = on["m"]
    s = float(m.scale)
    mask = H.philox_dropout_mask(M * N, p, *on["draw"]).view(M, N).double().numpy()
    assert 0.05 < float((mask == 0).mean()) < 0.15
    X, G = n(x0).astype(np.float64).reshape(M, K), n(gy).astype(np.float64).reshape(M, N)
    W_, b = n(m.linear.weight).astype(np.float64), n(m.linear.bias).astype(np.float64)
    A, U = n(m.lora_down.weight).astype(np.float64), n(m.lora_up.weight).astype(np.float64)
    Tn = X @ A.T
    yo = X @ W_.T + b + s * mask * (Tn @ U.T)
    Gm = G * mask
    Gt = s * (Gm @ U)
    dxo, duo, ddo = G @ W_ + Gt @ A, s * (Gm.T @ Tn), Gt.T @ X
    aT = np.abs(X) @ np.abs(A).T
    absy = np.abs(X) @ np.abs(W_).T + np.abs(b) + s / (1 - p) * (aT @ np.abs(U).T)
    aGt = s * (np.abs(Gm) @ np.abs(U))
    absdx = np.abs(G) @ np.abs(W_) + aGt @ np.abs(A)
    absu, absd = s * (np.abs(Gm).T @ aT), aGt.T @ np.abs(X)
    yv, dxv = n(on["y"]).reshape(M, N), n(on["dx"]).reshape(M, K)
    assert np.all(np.abs(yv - yo) <= 2.0 ** -8 * absy + 2.0 ** -8 * np.abs(yo) + 1e-3)
    assert np.all(np.abs(dxv - dxo) <= 2.0 ** -8 * absdx + 2.0 ** -8 * np.abs(dxo) + 1e-3)
    for name, res in (("on", on), ("off", off_), ("on, no dX", nox)):
        for what, got, want, absref in (("dUp", res["d_up"], duo, absu), ("dDown", res["d_down"], ddo, absd)):
            worst = float((np.abs(n(got).astype(np.float64) - want) / (2e-5 * absref + 1e-30)).max())
            print(f"[wide_dropout route] {name} {what}: worst |err| / tol = {worst:.3g}")
            close(n(got), want, absref, "f32", msg=f"{what} {name}")


# ----------------------------------------------------------------------------- (g) / (h) the step
def _twins(r, p=P):
    """W._twins with nn.Dropout(p) on every adapter of both twins."""
    torch.manual_seed(0)
    base = UNet2DConditionModel(block_out_channels=(64, 128, 128), layers_per_block=1, attention_heads=2,
                                cross_attention_dim=64, norm_num_groups=8)
    base.requires_grad_(False)
    for q in base.parameters():
        q.data = q.data.bfloat16().float()
    ref = copy.deepcopy(base)
    torch.manual_seed(5)
    ref_params = TR.inject(ref, L.UNET_DEFAULT_TARGET_REPLACE, r=r, dropout_p=p)
    for s_ in TR.sites_of(ref):
        s_.up.data.normal_(0, 0.02)
    dev = base.to(DEV).to(torch.bfloat16)
    L.inject_trainable_lora(dev, r=r, dropout_p=p)
    T.promote_lora_to_fp32(dev)
    ours, theirs = [m for m in dev.modules() if isinstance(m, L.LoraInjectedLinear)], TR.sites_of(ref)
    assert len(ours) == len(theirs) > 0
    for a, b in zip(ours, theirs):
        assert a.dropout.p == p and b.p == p
        a.lora_up.weight.data.copy_(b.up.data)
        a.lora_down.weight.data.copy_(b.down.data)
    ref.to(DEV)
    ref.train(), dev.train()
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


def _eager_steps(r):
    """One eager step with ops.WIDE_DROPOUT on and off, on ONE batch and the same dropout draws, and one f32 oracle step that is
    handed those draws -> {on / off: (‖flat gradient − oracle‖, backward paths of the rank-r sites)}, ‖oracle‖, sites."""
    ref, ref_params, dev, ours, theirs = _twins(r)
    lat, ehs, noise, ts = _batch()
    sched = DDPMScheduler()
    current, draws = [None], {}
    orig = ops.next_dropout_stream

    def recording(device):
        seed, off = orig(device)
        draws.setdefault(id(current[0]), []).append((seed, off))
        return seed, off

    def tap(mod):   # the adapter's single device entry: note which site is running (tests/test_gpu_parity_r4.py)
        inner = mod._forward_device

        def run(x, *a, **kw):
            current[0] = mod
            return inner(x, *a, **kw)
        mod.__dict__["_forward_device"] = run

    res, seen = {}, {}
    saved = ops.WIDE_DROPOUT
    for mode in (True, False):
        st = T.FlatLoraState([{"params": T.lora_params(dev), "lr": 1e-4, "weight_decay": 1e-2}], max_grad_norm=1.0, device=torch.device(DEV))
        st.attach_direct_grads(dev)
        mw = st.enable_merged_weights(dev)
        for m in ours:
            tap(m)
        ops.WIDE_DROPOUT, ops.next_dropout_stream = mode, recording
        ops.PATH_LOG = log = []
        try:
            for _ in range(3):   # the host model's layouts settle in the first two; the third is the step
                draws.clear()
                del log[:]
                st.zero_grad()
                torch.manual_seed(7)   # the dropout stream of every step of both settings
                T.forward_backward(dev, sched, lat.bfloat16(), ehs.bfloat16(), T.StepConfig(), noise=noise.bfloat16(), timesteps=ts, merged=mw)
                st.reduce_pending()
            torch.cuda.synchronize()
            got = st.flat_g.double().clone()
        finally:
            ops.WIDE_DROPOUT, ops.next_dropout_stream, ops.PATH_LOG = saved, orig, None
            _release(dev)
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
        assert all(len(draws.get(id(m), [])) == 1 for m in ours), "one dropout draw per site and forward"
        seen[mode] = [(draws[id(m)][0][0], int(draws[id(m)][0][1].item())) for m in ours]
        bwd = [path for ph, path, _, _, _, rr in log if ph == "bwd" and rr == r]
        res[mode] = (got, bwd)
        del st, mw
    assert seen[True] == seen[False], "both settings ran on the same dropout draws"
    assert len(set(seen[True])) == len(ours), "every site has its own offset"

    def pre_hook(site, draw):
        def hook(mod, args):
            x = args[0]
            N = mod.up.shape[0]
            rows = x.numel() // x.shape[-1]
            mod.mask = H.philox_dropout_mask(rows * N, P, draw[0], draw[1], DEV).view(*x.shape[:-1], N)
        return site.register_forward_pre_hook(hook)

    hooks = [pre_hook(s_, d) for s_, d in zip(theirs, seen[True])]
    with H.oracle_on_device():
        _, _, g32 = H.oracle_step_on_device(ref, ref_params, lat, noise, ts, ehs, False)
    for h in hooks:
        h.remove()
    want = torch.cat(g32).double()
    out = {mode: (float((got - want).norm()), bwd) for mode, (got, bwd) in res.items()}
    n_sites = len(ours)
    T._CKPT_CAND.pop(id(dev), None)
    del ref, ref_params, dev, ours, theirs, res
    gc.collect()
    torch.cuda.empty_cache()
    return out, float(want.norm()), n_sites


@pytest.mark.parametrize("r", [24, 64])
def test_eager_step_with_dropout_takes_the_deferred_pass_and_stays_at_the_oracle(r):
    """One eager step of the small stand-in UNet (bf16, trainer state, dropout 0.1 on every Linear adapter) at ranks 24 and 64:
    with ops.WIDE_DROPOUT every site leaves its factor gradients to the deferred pass, without it every site runs the
    primitives; on the same draws, the flat LoRA gradient with the switch on is no further from the f32 oracle step (handed
    those draws) than WIDE_DROPOUT_RATIO_BOUND x the same with it off."""
    res, norm, n_sites = _eager_steps(r)
    (e_on, bwd_on), (e_off, bwd_off) = res[True], res[False]
    print(f"\n[wide_dropout step] rank {r}: on {e_on:.4e} off {e_off:.4e} (‖oracle‖ {norm:.4e}) ratio {e_on / e_off:.3f}; "
          f"{len(bwd_on)} backward sites of {n_sites} adapters")
    assert len(bwd_on) == len(bwd_off) == n_sites
    assert all(p_.endswith("factors_deferred_mfma") for p_ in bwd_on), sorted(set(bwd_on))
    assert all(p_ == "primitives" for p_ in bwd_off), sorted(set(bwd_off))
    assert e_off < 0.1 * norm, "the oracle was handed the device's masks"
    assert e_on <= WIDE_DROPOUT_RATIO_BOUND * e_off, (f"rank {r}: ‖on − oracle‖ {e_on:.4e} > {WIDE_DROPOUT_RATIO_BOUND} x "
                                                      f"‖off − oracle‖ {e_off:.4e}")


def test_captured_step_with_dropout_replays_fresh_masks():
    """Rank 24 through trainer.GraphedForwardBackward, replayed twice: finite non-zero gradients that differ between the
    replays (the offsets are drawn inside the graph), every site on the deferred pass."""
    r = 24
    ref, ref_params, dev, ours, _ = _twins(r)
    del ref, ref_params
    lat, ehs, noise, ts = _batch()
    sched = DDPMScheduler()
    st = T.FlatLoraState([{"params": T.lora_params(dev), "lr": 1e-4, "weight_decay": 1e-2}], max_grad_norm=1.0, device=torch.device(DEV))
    st.attach_direct_grads(dev)
    mw = st.enable_merged_weights(dev)
    assert ops.WIDE_DROPOUT
    ops.PATH_LOG = log = []
    try:
        def fwd_bwd(lat_, cond_):
            return T.forward_backward(dev, sched, lat_, cond_, T.StepConfig(), noise=noise.bfloat16(), timesteps=ts, merged=mw)

        graphed = T.GraphedForwardBackward(fwd_bwd, lat.bfloat16(), ehs.bfloat16(), st)
        grads = []
        for _ in range(2):
            st.zero_grad()
            graphed(lat.bfloat16(), ehs.bfloat16())
            torch.cuda.synchronize()
            grads.append(st.flat_g.double().clone())
    finally:
        ops.PATH_LOG = None
        _release(dev)
    for g_ in grads:
        assert bool(torch.isfinite(g_).all()) and float(g_.abs().max()) > 0
    assert not torch.equal(grads[0], grads[1]), "every replay draws fresh masks"
    bwd = [path for ph, path, _, _, _, rr in log if ph == "bwd" and rr == r]
    assert bwd and len(bwd) % len(ours) == 0 and all(p_.endswith("factors_deferred_mfma") for p_ in bwd), sorted(set(bwd))
    del graphed, st, mw, fwd_bwd
    T._CKPT_CAND.pop(id(dev), None)
    del dev, ours
    gc.collect()
    torch.cuda.empty_cache()
