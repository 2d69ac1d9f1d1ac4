"""The matrix-core factor pass at LoRA ranks 17..64 (csrc/factor_mfma.hip, the WIDE form; ``ops.WIDE_FACTORS``).

A rank-r site runs as ns = ceil(r / 16) independent rank-16 slices on the same G and X, one workgroup per (row block, slice):
(a) every slice of a wide pack is bit for bit the rank <= 16 pack of the zero-padded factor slice, tail included; (b) every
slice's slab rows are bit for bit the rank-16 pass on that slice at the same block height and register class; (c) the fold
against ``oracle.lora_numpy.lora_linear_backward``, beta 0 and 1, two slice counts in one launch, f16 with ``up`` at 1e-4
(the per-slice power of two); (d) the memory footprint, registered with tests/test_gpu_footprint.py's registry; (e) the route:
one captured step of a small stand-in UNet with the switch on and off against the f32 oracle step, and an adapter without a
trainer state.

What (e) builds is released when it is done, as tests/test_gpu_merged_wide.py does."""
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
DTS = {"bf16": torch.bfloat16, "f16": torch.float16}
HEADS = (8, 40, 64)

# (b) / (c): class 1 at 64 rows; class 2 at 64 rows; a 32-row site; head-padded G; head-padded X.  Every M leaves a ragged
# last row block
SHAPES = [(70, 64, 96, None, None), (300, 640, 640, None, None), (40, 1280, 1280, None, None),
          (300, 320, 320, HEADS, None), (300, 320, 320, None, HEADS)]
GEOMETRY = [(1, 64), (2, 64), (2, 32), (1, 64), (1, 64)]   # (register class, rows per block) the planner gives SHAPES

# (e): worst ‖on − f32 oracle‖ / ‖off − f32 oracle‖ of the flat LoRA gradient over ranks 24 and 64 (``ops.WIDE_FACTORS`` on:
# the deferred matrix-core pass; off: the primitives), measured on MI355X (first GPU visit): rank 24 0.998 (4.1268e-04 /
# 4.1339e-04), rank 64 0.986 (3.7149e-04 / 3.7672e-04).  Bound = worst measured + 10 %
WIDE_FACTORS_RATIO_BOUND = 1.10


def _ns(r):
    return -(-r // 16)


def _slice16(down, up, s):
    """Slice s of the factors as a zero-padded rank-16 pair."""
    r = down.shape[0]
    rs = min(16, r - 16 * s)
    d16, u16 = torch.zeros(16, down.shape[1], device=DEV), torch.zeros(up.shape[0], 16, device=DEV)
    d16[:rs] = down[16 * s:16 * s + rs]
    u16[:, :rs] = up[:, 16 * s:16 * s + rs]
    return d16, u16, rs


def _pack(down, up, plan, dt):
    """One site through lora_amd_factor_pack into NaN-filled packs of the plan's size."""
    pk_down = torch.full((int(plan.pack_down_elems),), float("nan"), dtype=dt, device=DEV)
    pk_up = torch.full((int(plan.pack_up_elems),), float("nan"), dtype=dt, device=DEV)
    arr, total = _C.factor_pack_table([(down, up, pk_down, pk_up)])
    _C.factor_pack(_C.table_to_device(arr, DEV), 1, total, dt)
    return pk_down, pk_up


def _bits(t):
    return t.view(torch.int16)


# ----------------------------------------------------------------------------- (a) pack ties
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("r", [17, 33, 64])
def test_wide_pack_slices_are_the_rank_16_packs_of_the_padded_slices(r, dt):
    N, K, dtype = 96, 64, DTS[dt]
    down, up = rnd((r, K), "f32", 0.2, seed=r), rnd((N, r), "f32", 3e-4, seed=r + 1)
    for s in range(_ns(r)):   # slices of very different magnitude: each takes its own power of two (f16)
        up[:, 16 * s:16 * s + 16] *= 8.0 ** s
    plan, p16 = _C.factors_mfma_plan(300, K, N, r, dtype, wide=True), _C.factors_mfma_plan(300, K, N, 16, dtype)
    pk_down, pk_up = _pack(down, up, plan, dtype)
    torch.cuda.synchronize()
    for s in range(_ns(r)):
        d16, u16, _ = _slice16(down, up, s)
        nd, nu = _pack(d16, u16, p16, dtype)
        for wide, narrow, C_ in ((pk_down, nd, K), (pk_up, nu, N)):
            per = 2 * C_ * 16 + 8
            assert narrow.numel() == per and wide.numel() == _ns(r) * per
            body = per - 8   # the tail: f16 only (bf16 leaves it unwritten in both)
            got, want = wide[s * per:(s + 1) * per], narrow
            assert torch.equal(_bits(got[:body]), _bits(want[:body])), (r, dt, s)
            if dt == "f16":   # the tail: this slice's power of two and its inverse
                assert torch.equal(_bits(got[body:]), _bits(want[body:])), (r, dt, s)
                sc = got[body:].view(torch.float32)
                assert float(sc[0]) * float(sc[1]) == 1.0 and float(sc[0]) > 0
            else:
                assert bool(torch.isnan(got[body:]).all()) and bool(torch.isnan(want[body:]).all())
    if dt == "f16":   # the scales differ from slice to slice by the 8 x steps above
        sc = [float(pk_up[s * (2 * N * 16 + 8) + 2 * N * 16:].view(torch.float32)[0]) for s in range(_ns(r))]
        assert len(set(sc)) == len(sc), sc


# ----------------------------------------------------------------------------- the pass on raw tables
def _site(M, K, N, r, gh, xh, dt, seed, up_scale=0.3, wide=True, rows=0, factors=None):
    """G / X (head-padded with poisoned pad columns where asked), factors, packs and NaN slabs of one site."""
    name = {torch.bfloat16: "bf16", torch.float16: "f16"}[dt]
    x, g = rnd((M, K), name, seed=10 + seed), rnd((M, N), name, seed=30 + seed)
    down, up = factors if factors else (rnd((r, K), "f32", 0.2, seed=50 + seed), rnd((N, r), "f32", up_scale, seed=70 + seed))
    X, G = n(x), n(g)
    gd = torch.from_numpy(_heads_pack(G, gh)).to(DEV).to(dt) if gh else g
    xd = torch.from_numpy(_heads_pack(X, xh)).to(DEV).to(dt) if xh else x
    if gh:  # pad columns of a real G need not be zero: the kernel must not read them
        gd.view(M, gh[0], gh[2])[:, :, gh[1]:] = 7.0
    if xh:
        xd.view(M, xh[0], xh[2])[:, :, xh[1]:] = -3.0
    plan = _C.factors_mfma_plan(M, K, N, r, dt, rows, wide=wide)
    assert plan.supported, (M, K, N, r)
    return dict(M=M, K=K, N=N, r=r, X=X, G=G, g=gd, x=xd, gh=gh, xh=xh, down=down, up=up, plan=plan,
                up_part=torch.full((int(plan.up_part_floats),), float("nan"), device=DEV),
                down_part=torch.full((int(plan.down_part_floats),), float("nan"), device=DEV),
                pk_down=torch.full((int(plan.pack_down_elems),), float("nan"), dtype=dt, device=DEV),
                pk_up=torch.full((int(plan.pack_up_elems),), float("nan"), dtype=dt, device=DEV))


def _launch(sites, dt, s_, wide=True):
    """One pack launch, one pass launch per (register class, block height)."""
    arr, total = _C.factor_pack_table([(s["down"], s["up"], s["pk_down"], s["pk_up"]) for s in sites])
    _C.factor_pack(_C.table_to_device(arr, DEV), len(sites), total, dt)
    by_cls = {}
    for s in sites:
        by_cls.setdefault((int(s["plan"].lds_class), int(s["plan"].rows_per_block)), []).append(s)
    for (cls, rpb), group in by_cls.items():
        arr, grid = _C.factors_mfma_table([(s["g"], s["x"], s["pk_down"], s["pk_up"], s["up_part"], s["down_part"], s_, s["gh"],
                                            s["xh"], s["r"], s["plan"]) for s in group], dt, cls)
        if wide:
            assert grid == sum(int(s["plan"].nparts) * _ns(s["r"]) for s in group)
        _C.linear_bwd_factors_mfma_ragged(_C.table_to_device(arr, DEV), len(group), grid, cls, dt, False, rpb, wide=wide)
    return len(by_cls)


# ----------------------------------------------------------------------------- (b) pass ties
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("shape,geom", list(zip(SHAPES, GEOMETRY)), ids=[f"{s[0]}x{s[1]}x{s[2]}{'g' if s[3] else ''}{'x' if s[4] else ''}"
                                                                            for s in SHAPES])
def test_wide_slab_rows_are_the_rank_16_pass_on_each_slice(shape, geom, dt):
    """Rank 33 (two full slices and one of a single rank): rows [16 s, 16 s + min(16, r - 16 s)) of every row block's
    [16 ns][C] slab equal, bit for bit, the rank <= 16 pass on slice s as a zero-padded rank-16 site planned at the same block
    height (the same register class follows).  The dead rows of the last slice are exact zeros."""
    (M, K, N, gh, xh), (cls, rpb), r, dtype = shape, geom, 33, DTS[dt]
    w = _site(M, K, N, r, gh, xh, dtype, seed=1, up_scale=1e-3)
    assert (int(w["plan"].lds_class), int(w["plan"].rows_per_block)) == (cls, rpb)
    _launch([w], dtype, 0.7)
    nparts, ns = int(w["plan"].nparts), _ns(r)
    assert nparts == -(-M // rpb) and M % rpb
    up_w, down_w = w["up_part"].view(nparts, 16 * ns, N), w["down_part"].view(nparts, 16 * ns, K)
    for s in range(ns):
        d16, u16, rs = _slice16(w["down"], w["up"], s)
        nw = _site(M, K, N, 16, gh, xh, dtype, seed=1, wide=False, rows=rpb, factors=(d16, u16))
        assert (int(nw["plan"].lds_class), int(nw["plan"].rows_per_block), int(nw["plan"].nparts)) == (cls, rpb, nparts)
        _launch([nw], dtype, 0.7, wide=False)
        torch.cuda.synchronize()
        up_n, down_n = nw["up_part"].view(nparts, 16, N), nw["down_part"].view(nparts, 16, K)
        assert bool(torch.isfinite(up_n[:, :rs]).all()) and bool(torch.isfinite(down_n[:, :rs]).all())
        assert torch.equal(up_w[:, 16 * s:16 * s + rs].view(torch.int32), up_n[:, :rs].view(torch.int32)), (s, "up")
        assert torch.equal(down_w[:, 16 * s:16 * s + rs].view(torch.int32), down_n[:, :rs].view(torch.int32)), (s, "down")
    assert not bool(up_w[:, r:].any()) and not bool(down_w[:, r:].any())


# ----------------------------------------------------------------------------- (c) oracle
def _fold_and_check(sites, s_, beta, what):
    for s in sites:
        N, K, r, plan = s["N"], s["K"], s["r"], s["plan"]
        d_up, d_down = torch.full((N, r), beta, device=DEV), torch.full((r, K), beta, device=DEV)
        if beta == 0.0:   # beta = 0 ignores what the outputs held
            d_up.fill_(float("nan")), d_down.fill_(float("nan"))
        table, cnt, total = _C.make_reduce_table(
            [(s["up_part"], d_up, plan.nparts, plan.rank_tile, N, r, _C.FACTOR_KR, 1.0, beta),
             (s["down_part"], d_down, plan.nparts, plan.rank_tile, K, r, _C.FACTOR_RK, 1.0, beta)], DEV)
        _C.reduce_batched(table, cnt, total)
        if "ddo" not in s:   # the reference, once per site
            A, U = n(s["down"]), n(s["up"])
            _, s["ddo"], s["duo"], _, _ = O.lora_linear_backward(s["G"], s["X"], np.zeros((N, K), np.float32), A, U, s_)
            s["absu"] = s_ * (np.abs(s["G"]).T @ (np.abs(s["X"]) @ np.abs(A).T))
            s["absd"] = (s_ * np.abs(s["G"]) @ np.abs(U)).T @ np.abs(s["X"])
        close(n(d_up), s["duo"] + beta, s["absu"] + beta, "f32", k=1e-4, msg=f"{what} dUp {s['M']}x{K}x{N} r{r} beta {beta}")
        close(n(d_down), s["ddo"] + beta, s["absd"] + beta, "f32", k=1e-4, msg=f"{what} dDown {s['M']}x{K}x{N} r{r} beta {beta}")


@pytest.mark.parametrize("dt,up_scale", [("bf16", 0.3), ("f16", 0.3), ("f16", 1e-4)], ids=["bf16", "f16", "f16_up1e-4"])
@pytest.mark.parametrize("r", [17, 32, 33, 48, 64])
def test_wide_pass_vs_oracle(r, dt, up_scale):
    """dB = s G^T (X A^T), dA = (s G B)^T X (lora.py:53-58's autograd) through the pack, the wide pass and the fold, at the
    tolerance of the rank <= 16 pass (tests/test_gpu_parity_r4.py): every shape of (b) and M = 1, one pass launch per (class,
    height), folded with beta = 0 and with beta = 1 into preloaded outputs.  f16 with ``up`` at 1e-4 (where it sits for
    hundreds of steps after its zero start) holds the same bound through the per-slice power of two."""
    dtype, s_ = DTS[dt], 0.7
    sites = [_site(M, K, N, r, gh, xh, dtype, seed=i, up_scale=up_scale)
             for i, (M, K, N, gh, xh) in enumerate(SHAPES + [(1, 320, 320, None, None)])]
    assert _launch(sites, dtype, s_) == 3
    for beta in (0.0, 1.0):
        _fold_and_check(sites, s_, beta, f"{dt} up~{up_scale}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_sites_of_different_slice_counts_share_one_launch(dt):
    """Ranks 17, 64, 33 and 48 (2, 4, 3, 3 slices) in ONE table, one launch: the grid is the sum of nrb x ns."""
    dtype, s_ = DTS[dt], 0.9
    sites = [_site(300, 320, 320, 17, None, None, dtype, seed=1), _site(70, 64, 96, 64, None, None, dtype, seed=2),
             _site(129, 320, 320, 33, HEADS, None, dtype, seed=3), _site(1, 320, 320, 48, None, HEADS, dtype, seed=4)]
    assert _launch(sites, dtype, s_) == 1
    _fold_and_check(sites, s_, 0.0, f"{dt} mixed slice counts")


# ----------------------------------------------------------------------------- (d) footprint
def _guarded_site(M, K, N, r, seed, dt, g_heads=None, x_heads=None):
    """tests/test_gpu_footprint.py's _fm_site at a rank above 16: poisoned G / X (NaN head pads) and factors, guarded packs
    and slabs exactly as the wide plan sizes them."""
    g_log, x_log = FP.rnd((M, N), dt, seed=seed), FP.rnd((M, K), dt, seed=seed + 1)
    g = FP.padded(g_log, *g_heads) if g_heads else FP.inp(g_log)
    x = FP.padded(x_log, *x_heads) if x_heads else FP.inp(x_log)
    down, up = FP.inp(FP.rnd((r, K), FP.F32, 0.1, seed=seed + 2)), FP.inp(FP.rnd((N, r), FP.F32, 0.05, seed=seed + 3))
    plan = _C.factors_mfma_plan(M, K, N, r, dt, wide=True)
    assert plan.supported and plan.rank_tile == 16 * _ns(r)
    return dict(M=M, K=K, N=N, r=r, g=g, x=x, g_log=g_log, x_log=x_log, down=down, up=up, plan=plan, scale=0.6,
                g_heads=(N // g_heads[0], *g_heads) if g_heads else None,
                x_heads=(K // x_heads[0], *x_heads) if x_heads else None,
                pk_down=FP.out(int(plan.pack_down_elems), dt), pk_up=FP.out(int(plan.pack_up_elems), dt),
                up_part=FP.out(int(plan.up_part_floats)), down_part=FP.out(int(plan.down_part_floats)))


WIDE_TABLE = [(129, 320, 320, 17, (40, 64), None), (65, 320, 320, 33, None, (40, 64)), (1, 320, 320, 64, None, None),
              (70, 64, 96, 33, None, None)]


@FP.case("lora_amd_factor_pack", "lora_amd_linear_bwd_factors_mfma_ragged")
def case_factors_wide():
    """Ranks 17 / 33 / 64 in one wide table (M = 1, one row past a block, head-padded G and X, a 64 x 96 site), bf16 and f16:
    the pack writes exactly the ns slice bodies (f16: and their tails), the pass exactly the 16 ns rows of every block's slab;
    guards intact, inputs poisoned, values equal the launch on plain allocations and the dense formula."""
    for dt in (FP.BF, torch.float16):
        sites = [_guarded_site(M, K, N, r, 10 * j + 1, dt, gh, xh) for j, (M, K, N, r, gh, xh) in enumerate(WIDE_TABLE)]
        plain = [dict(pk_down=torch.zeros_like(s["pk_down"].data), pk_up=torch.zeros_like(s["pk_up"].data),
                      up_part=torch.zeros_like(s["up_part"].data), down_part=torch.zeros_like(s["down_part"].data)) for s in sites]
        for guarded in (True, False):
            bufs = [{k: s[k].data for k in p} for s, p in zip(sites, plain)] if guarded else plain
            for s, b in zip(sites, bufs):
                s["_b"] = b
            get = lambda s, k: s["_b"][k]  # noqa: E731
            arr, total = _C.factor_pack_table([(s["down"], s["up"], get(s, "pk_down"), get(s, "pk_up")) for s in sites])
            _C.factor_pack(FP.table(arr), len(sites), total, dt)
            cls = max(int(s["plan"].lds_class) for s in sites)
            heights = {int(s["plan"].rows_per_block) for s in sites}
            assert cls == 1 and heights == {64}
            arr, grid = _C.factors_mfma_table(
                [(s["g"], s["x"], get(s, "pk_down"), get(s, "pk_up"), get(s, "up_part"), get(s, "down_part"), s["scale"],
                  s["g_heads"], s["x_heads"], s["r"], s["plan"]) for s in sites], dt, cls)
            raw, moff = _C.factors_mfma_table_bytes(arr, grid)
            tab = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
            _C.linear_bwd_factors_mfma_ragged(tab, len(sites), grid, cls, dt, False, 64, map_offset=moff, wide=True)
        FP.check(*[s[k] for s in sites for k in ("pk_down", "pk_up", "up_part", "down_part")], what="factors wide")
        for s, p in zip(sites, plain):
            ns = _ns(s["r"])
            for k, C_ in (("pk_down", s["K"]), ("pk_up", s["N"])):
                per, body = 2 * C_ * 16 + 8, 2 * C_ * 16
                v = s[k].data.view(ns, per)
                MG.assert_written(v[:, :body], f"wide {k} slice bodies")
                if dt == torch.float16:
                    MG.assert_written(v[:, body:], f"wide {k} tails")
                else:
                    MG.assert_untouched(v[:, body:], f"wide {k} tails (bf16 has no scale)")
                assert torch.equal(v[:, :body].view(torch.int16), p[k].view(ns, per)[:, :body].view(torch.int16)), k
            nparts, RT = int(s["plan"].nparts), int(s["plan"].rank_tile)
            for k in ("up_part", "down_part"):
                MG.assert_written(s[k].data, f"wide {k}: all 16 ns rows of every block")
                assert torch.equal(s[k].data.view(torch.int32), p[k].view(torch.int32)), f"{k} differs from the unguarded launch"
            FP._check_factor_grads(s, s["up_part"], s["down_part"], nparts, RT, f"factors wide M={s['M']} r={s['r']}")


def test_footprint_case():
    assert "factors_wide" in FP.CASES and {"lora_amd_factor_pack", "lora_amd_linear_bwd_factors_mfma_ragged"} <= FP.covered()
    torch.cuda.synchronize()
    case_factors_wide()
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- (e) the route
@pytest.fixture
def path_log():
    ops.PATH_LOG = log = []
    yield log
    ops.PATH_LOG = None


def test_adapter_without_a_trainer_state_keeps_the_primitives(path_log):
    """No trainer state, no deferred pass: the four primitive launches in the site's backward, as before."""
    M, K, N, r = 300, 320, 320, 32
    torch.manual_seed(0)
    m = L.LoraInjectedLinear(K, N, False, r=r, dropout_p=0.0, scale=0.8).to(DEV).to(torch.bfloat16)
    m.linear.requires_grad_(False)
    T.promote_lora_to_fp32(m)
    m.lora_up.weight.data.normal_(0, 0.05)
    m.__dict__["_merged"] = mw = ops.MergedWeights()
    assert ops.WIDE_FACTORS and not mw.defer_factors
    x, gy = rnd((M, K), "bf16", seed=5).requires_grad_(True), rnd((M, N), "bf16", seed=6)
    mw.refresh()
    m.forward_heads(x, None, None).backward(gy)
    assert [p for ph, p, *_ in path_log if ph == "bwd"] == ["merged_dx+factors_primitives"], path_log
    _, ddo, duo, _, _ = O.lora_linear_backward(n(gy), n(x), n(m.linear.weight), n(m.lora_down.weight), n(m.lora_up.weight), 0.8)
    X, G, A, U = np.abs(n(x)), np.abs(n(gy)), np.abs(n(m.lora_down.weight)), np.abs(n(m.lora_up.weight))
    close(n(m.lora_up.weight.grad), duo, 0.8 * (G.T @ (X @ A.T)), "f32", msg="dUp")
    close(n(m.lora_down.weight.grad), ddo, (0.8 * G @ U).T @ X, "f32", msg="dDown")


def _twins(r):
    """The small stand-in UNet of tests/test_gpu_merged_wide.py's (g) (same constructor arguments: every Linear at least 64
    wide), twice: bf16 on the device with our adapters, f32 oracle twin with the reference-algorithm adapters."""
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
        a.lora_up.weight.data.copy_(b.up.data)
        a.lora_down.weight.data.copy_(b.down.data)
    ref.to(DEV)
    ref.train(), dev.train()
    return ref, ref_params, dev


def _step(r):
    """One replayed step of the captured forward + backward with ops.WIDE_FACTORS on and off, on ONE batch and one oracle step
    -> {on / off: (‖flat gradient − f32 oracle‖, backward paths of the merged sites of rank r)}."""
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
    saved = ops.WIDE_FACTORS
    for mode in (True, False):
        st = T.FlatLoraState([{"params": T.lora_params(dev), "lr": 1e-4, "weight_decay": 1e-2}], max_grad_norm=1.0, device=torch.device(DEV))
        st.attach_direct_grads(dev)
        mw = st.enable_merged_weights(dev)
        ops.WIDE_FACTORS = mode
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
            ops.WIDE_FACTORS, ops.PATH_LOG = saved, None
            for m in dev.modules():
                m.__dict__.pop("_grad_sink", None)
                m.__dict__.pop("_merged", None)
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
        bwd = [path for ph, path, _, _, _, rr in log if ph == "bwd" and path.startswith("merged") and rr == r]
        res[mode] = (float((got - want).norm()), bwd)
        del graphed, st, mw, fwd_bwd
    # nothing of this stays on the device: the trainer's per-model cache would keep the model alive, the captured graphs their pools
    T._CKPT_CAND.pop(id(dev), None)
    del ref, ref_params, dev
    gc.collect()
    torch.cuda.empty_cache()
    return res, float(want.norm())


@pytest.mark.parametrize("r", [24, 64])
def test_captured_step_takes_the_deferred_pass_and_stays_at_the_oracle(r):
    """One step of the small stand-in UNet (bf16, trainer state, merged weights, hipGraph replay) at ranks 24 and 64: with
    ops.WIDE_FACTORS every wide merged site leaves its factor gradients to the deferred matrix-core pass (none runs the
    primitives), without it the log is the primitives'; the flat LoRA gradient with the switch on is no further from the f32
    oracle step than WIDE_FACTORS_RATIO_BOUND x the same with it off."""
    res, norm = _step(r)
    (e_on, bwd_on), (e_off, bwd_off) = res[True], res[False]
    print(f"\n[factors_wide step] rank {r}: on {e_on:.4e} off {e_off:.4e} (‖oracle‖ {norm:.4e}) ratio {e_on / e_off:.3f}; "
          f"{len(bwd_on)} wide merged backward sites")
    assert bwd_on and all(p.endswith("factors_deferred_mfma") for p in bwd_on), sorted(set(bwd_on))
    assert not any("primitives" in p for p in bwd_on)
    assert len(bwd_off) == len(bwd_on) and all(p.endswith("factors_primitives") for p in bwd_off), sorted(set(bwd_off))
    assert e_on <= WIDE_FACTORS_RATIO_BOUND * e_off, (f"rank {r}: ‖on − oracle‖ {e_on:.4e} > {WIDE_FACTORS_RATIO_BOUND} x "
                                                       f"‖off − oracle‖ {e_off:.4e}")
