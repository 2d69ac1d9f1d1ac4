"""Footprint of every launcher of include/lora_amd.h: what it writes, what it reads, and nothing else.

Every launcher has a case (``CASES``; one case may launch several entries of a family, and
tests/test_capi_cpu.py::test_every_launcher_has_a_footprint_case fails for a launcher of the header without one).  A case
  * places each output in a :class:`tests.memguard.Guarded` allocation ``[guard | data | guard]`` pre-filled with a
    sentinel NaN (accumulating and in-place outputs start from known values instead) and checks the guards bit for bit;
  * places each input in the middle of a NaN-filled allocation (:func:`tests.memguard.poisoned`), with NaN in the row
    gaps of strided operands and in the pads of head-padded rows: an over-read reaches the output as NaN;
  * checks the written set (no sentinel left where the contract says the launch writes, the sentinel intact where it says
    the launch does not) and the values against an f64 reference at the tolerances of DESIGN §5 (f32 results:
    2e-5 of the absolute bound, the factor pass 1e-4; 16-bit results: one rounding on top).
Shapes sit at the edges of what each plan accepts (M = 1, one row past a tile, rank tiles not full, partial pixel tiles,
several sites in ONE buffer); counters of the launchers that fold across workgroups are checked back at zero after every
launch and a second launch on the same counters must give the same bits.

Cases whose value reference is long (the SVD distillation's fused small steps) compare the guarded launch with the same
launch on plain allocations, bit for bit: tests/test_gpu_svd_small.py checks the plain launch against f64.
"""
from __future__ import annotations

import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from lora_amd import _C
from tests import helpers as H
from tests import memguard as MG

DEV = "cuda:0"
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
EPS = {F32: 0.0, BF: 2.0 ** -8, HF: 2.0 ** -11}
CASES = {}


def case(*launchers):
    """Register a footprint case for ``launchers`` (the entry points of include/lora_amd.h it launches and checks)."""
    def deco(fn):
        name = fn.__name__[len("case_"):]
        assert name not in CASES
        CASES[name] = (tuple(launchers), fn)
        return fn
    return deco


def covered():
    return {name for launchers, _ in CASES.values() for name in launchers}


# ----------------------------------------------------------------------------- helpers
def lib():
    return _C.require()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(rc, what):
    _C._check(rc, what)


def rnd(shape, dt=F32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dt).to(DEV)


def out(shape, dt=F32, **kw):
    return MG.Guarded(shape, dt, DEV, **kw)


def inp(t, ld=None, align=256):
    return MG.poisoned(t, ld=ld, align=align)


def check(*gs, what=""):
    torch.cuda.synchronize()
    for i, g in enumerate(gs):
        g.check(f"{what} operand {i}")


def d64(t):
    return t.detach().double()


def close(got, want, absref, dt=F32, k=2e-5, msg="", eps=None):
    """|got - want| <= k * absref + eps(dt) * |want| elementwise (absref = the sum of |terms|)."""
    got, want, absref = d64(got), d64(want), d64(absref)
    assert bool(torch.isfinite(got).all()), f"{msg}: non-finite values in the output"
    tol = k * absref + (EPS[dt] if eps is None else eps) * want.abs() + 1e-30
    bad = (got - want).abs() > tol
    assert not bool(bad.any()), (f"{msg}: {int(bad.sum())} of {bad.numel()} outside tolerance; worst "
                                 f"{float((got - want).abs().max()):.3e}")


def heads_cols(n_logical, d, D):
    """Physical column of each logical column of a head-padded row (heads of d in slots of D)."""
    i = torch.arange(n_logical, device=DEV)
    return (i // d) * D + i % d


def padded(t, d, D):
    """Logical [M, heads*d] -> a poisoned physical [M, heads*D] (NaN pads) as the head-padded kernels read it."""
    M, n = t.shape
    g = MG.Guarded((M, n // d * D), t.dtype, DEV, poison=True)
    g.data[:, heads_cols(n, d, D)] = t
    v = g.data
    v._memguard = g
    return v


def table(arr):
    return _C.table_to_device(arr, DEV)


# ----------------------------------------------------------------------------- fold of partials into the flat buffer
REDUCE_ROWS = [  # (nparts, RT, C, r, layout): ranks 1..16, rank tiles not full, odd C, 17 parts (one past 16)
    (3, 4, 320, 1, 0), (5, 4, 33, 3, 1), (1, 8, 40, 5, 0), (17, 16, 24, 9, 1), (2, 16, 8, 13, 0), (4, 16, 64, 16, 1)]
REDUCE_GAP = 2   # a slice no row lists sits behind this row: it must keep the sentinel


@case("lora_amd_reduce_batched")
def case_reduce_batched(bad_row=None):
    """Sites adjacent in ONE flat f32 buffer, as the trainer's flat gradient, at beta 0 and 1.  ``bad_row``:
    describe that row with one column too many (the check must then fail)."""
    sizes = [r * Cc for _, _, Cc, r, _ in REDUCE_ROWS]
    gap = 7
    starts, pos = [], 0
    for i, s in enumerate(sizes):
        starts.append(pos)
        pos += s + (gap if i == REDUCE_GAP else 0)
    for beta in (0.0, 1.0):
        flat = out(pos)
        prev = []
        for i, s in enumerate(sizes):
            v = rnd((s,), seed=50 + i) if beta else None
            if v is not None:
                flat.data[starts[i]:starts[i] + s] = v
            prev.append(v)
        parts, rows = [], []
        for i, (nparts, RT, Cc, r, layout) in enumerate(REDUCE_ROWS):
            p = MG.Guarded((nparts, RT, Cc), F32, DEV, poison=True)   # rows r .. RT-1 hold the poison: never read
            p.data[:, :r, :] = rnd((nparts, r, Cc), seed=10 + i)
            parts.append(p)
            Cd = Cc + 1 if i == bad_row else Cc
            rows.append((p.data, flat.data[starts[i]:], nparts, RT, Cd, r, layout, 0.75, beta))
        tab, n, total = _C.make_reduce_table(rows, DEV)
        _C.reduce_batched(tab, n, total)
        check(flat, *parts, what="reduce_batched")
        MG.assert_untouched(flat.data[starts[REDUCE_GAP] + sizes[REDUCE_GAP]:starts[REDUCE_GAP + 1]], "gap slice")
        for i, (nparts, RT, Cc, r, layout) in enumerate(REDUCE_ROWS):
            src = d64(parts[i].data[:, :r, :])
            want = 0.75 * src.sum(0)
            ref = 0.75 * src.abs().sum(0)
            if layout == 1:
                want, ref = want.t(), ref.t()
            want, ref = want.reshape(-1), ref.reshape(-1)
            if beta:
                want, ref = want + d64(prev[i]), ref + d64(prev[i]).abs()
            close(flat.data[starts[i]:starts[i] + sizes[i]], want, ref, msg=f"reduce row {i} beta {beta}")


@case("lora_amd_sum_parts")
def case_sum_parts():
    for nparts, n in ((1, 4), (5, 76), (17, 4100)):   # n and the stride: multiples of 4
        part = inp(rnd((nparts * n,), seed=n), align=16)
        o = out(n, align=16)                                        # the launcher needs 16-byte-aligned buffers only
        ok(lib().lora_amd_sum_parts(part.data_ptr(), nparts, n, o.ptr, n, stream()), "sum_parts")
        check(o, what="sum_parts")
        p = d64(part).view(nparts, n)
        close(o.data, p.sum(0), p.abs().sum(0), msg="sum_parts")


# ----------------------------------------------------------------------------- launchers with arrival counters
CONV3_FUSED = [  # B, Ci, Co, H, W, r: a plan with ksplit > 1, a partial last pixel tile (W = 16 + 4), B = 1
    (1, 640, 96, 12, 20, 16), (1, 256, 64, 8, 24, 8)]


@case("lora_amd_conv3_nhwc_fwd_fused", "lora_amd_conv3_nhwc_pack_batched")
def case_conv3_nhwc_fwd_fused(stale_counters=False):
    """t_part + counters of a ksplit > 1 plan; every counter back at zero after each launch; a second launch on the same
    counters gives the same bits.  ``stale_counters``: start from the counters a launch that forgot its reset leaves
    behind (ksplit per tile; the check must then fail)."""
    s_ = 0.8
    for B, Ci, Co, Hh, Ww, r in CONV3_FUSED:
        plan = _C.conv3_nhwc_plan(B, Ci, Hh, Ww, r)
        assert plan.native == 1 and plan.ksplit > 1 and Ww % 16
        M = B * Hh * Ww
        x_nhwc = inp(rnd((B, Hh, Ww, Ci), BF, seed=1))
        y0 = rnd((M, Co), BF, seed=2)
        down, up = inp(rnd((r, Ci, 3, 3), F32, 0.1, seed=3)), inp(rnd((Co, r), F32, 0.05, seed=4))
        pf, pd, pu = out(int(plan.pf_elems), BF), out(int(plan.pd_elems), BF), out(Co * 32, BF)
        arr, total = _C.conv3_nhwc_pack_table([(down, up, pf.data, pd.data, pu.data)])
        _C.conv3_nhwc_pack_batched(table(arr), 1, total, BF)
        check(pf, pd, pu, what="conv3 pack_batched")
        for g_, nm in ((pf, "pf"), (pd, "pd"), (pu, "pu")):
            MG.assert_written(g_.data, f"conv3 pack {nm}")
        t_part = out(int(plan.t_part_floats))
        counters = out(int(plan.fwd_tiles), torch.int32, fill="zero")
        if stale_counters:
            counters.data.fill_(int(plan.ksplit))
        results = []
        for _ in range(2):
            y = MG.guarded_like(y0)
            t = out((M, r))
            ok(lib().lora_amd_conv3_nhwc_fwd_fused(x_nhwc.data_ptr(), pf.ptr, pu.ptr, y.ptr, t.ptr, t_part.ptr, counters.ptr,
                                                   B, Ci, Co, Hh, Ww, r, _C.BF16, s_, 0.0, 0, 0, None, stream()),
               "conv3_nhwc_fwd_fused")
            check(y, t, t_part, counters, what="conv3_nhwc_fwd_fused")
            assert int(counters.data.abs().max()) == 0, "arrival counters not back at zero after the launch"
            results.append((y.data.clone(), t.data.clone()))
        assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
        y_, t_ = results[0]
        xd = d64(x_nhwc).permute(0, 3, 1, 2)
        dn = d64(down) if r <= 8 else d64(down.to(BF))
        T = F.conv2d(xd, dn, padding=1).permute(0, 2, 3, 1).reshape(M, r)
        Tabs = F.conv2d(xd.abs(), dn.abs(), padding=1).permute(0, 2, 3, 1).reshape(M, r)
        close(t_, T, Tabs, k=3e-5, msg="conv3 fused T")
        T32 = d64(t_)
        close(y_, d64(y0) + s_ * T32 @ d64(up).t(), d64(y0).abs() + s_ * T32.abs() @ d64(up).abs().t(), BF, k=3e-5,
              msg="conv3 fused Y")


@case("lora_amd_linear_bwd_g_folded")
def case_linear_bwd_g_folded():
    """Gt folded by the last-arriving column workgroup of a row block: M one past a row block and M = 1, the widest N."""
    s_ = 0.7
    for M, N, r in ((129, 1280, 9), (1, 320, 16), (145, 10240, 13)):
        lp = _C.linear_plan(M, 320, N, r)
        assert lp.fused
        g, t, up = inp(rnd((M, N), BF, seed=1)), inp(rnd((M, r), F32, 0.5, seed=2)), inp(rnd((N, r), F32, 0.05, seed=3))
        counters = out(_C.linear_bwd_g_blocks(M, N, r), torch.int32, fill="zero")
        res = []
        for _ in range(2):
            gp, upp, gt = out(int(lp.gt_part_floats)), out(int(lp.up_part_floats)), out((M, r))
            ok(lib().lora_amd_linear_bwd_g_folded(g.data_ptr(), N, t.data_ptr(), up.data_ptr(), gp.ptr, gt.ptr, counters.ptr,
                                                  upp.ptr, M, N, r, _C.BF16, _C.F32, s_, 0.0, 0, 0, None, stream()),
               "linear_bwd_g_folded")
            check(gp, upp, gt, counters, what="linear_bwd_g_folded")
            assert int(counters.data.abs().max()) == 0, "row-block counters not back at zero"
            res.append((gt.data.clone(), upp.data.clone()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        G64 = d64(g)
        close(res[0][0], s_ * G64 @ d64(up), s_ * G64.abs() @ d64(up).abs(), msg="folded Gt")
        RT = int(lp.up_part_floats) // (int(lp.nparts_up) * N)
        dup = d64(res[0][1]).view(int(lp.nparts_up), RT, N)[:, :r, :].sum(0)
        close(dup, s_ * d64(t).t() @ G64, s_ * d64(t).abs().t() @ G64.abs(), msg="folded dUp partials")


# ----------------------------------------------------------------------------- the factor pass of the merged route
def _fm_site(M, K, N, r, seed, g_heads=None, x_heads=None, mfma=True):
    """One site of the matrix-core pass: poisoned G / X (NaN head pads), guarded packs and slabs sized by the plan."""
    g_log, x_log = rnd((M, N), BF, seed=seed), rnd((M, K), BF, seed=seed + 1)
    g = padded(g_log, *g_heads) if g_heads else inp(g_log)
    x = padded(x_log, *x_heads) if x_heads else inp(x_log)
    down, up = inp(rnd((r, K), F32, 0.1, seed=seed + 2)), inp(rnd((N, r), F32, 0.05, seed=seed + 3))
    plan = _C.factors_mfma_plan(M, K, N, r, BF) if mfma else None
    assert plan is None or plan.supported
    s = dict(M=M, K=K, N=N, r=r, g=g, x=x, g_log=g_log, x_log=x_log, down=down, up=up, plan=plan, scale=0.6,
             g_heads=(N // g_heads[0], *g_heads) if g_heads else None,
             x_heads=(K // x_heads[0], *x_heads) if x_heads else None,
             )
    if plan is not None:
        s.update(pk_down=out(int(plan.pack_down_elems), BF), pk_up=out(int(plan.pack_up_elems), BF),
                 up_part=out(int(plan.up_part_floats)), down_part=out(int(plan.down_part_floats)))
    return s


def _check_factor_grads(s, up_part, down_part, nparts, RT, what):
    M, K, N, r, sc = s["M"], s["K"], s["N"], s["r"], s["scale"]
    for slab, C_ in ((up_part, N), (down_part, K)):
        MG.assert_written(slab.data.view(nparts, RT, C_)[:, :r, :], f"{what} slab rows < r")
    G, X = d64(s["g_log"]), d64(s["x_log"])
    dn, u = d64(s["down"]), d64(s["up"])
    dup = d64(up_part.data).view(nparts, RT, N)[:, :r, :].sum(0).t()
    ddn = d64(down_part.data).view(nparts, RT, K)[:, :r, :].sum(0)
    close(dup, sc * G.t() @ (X @ dn.t()), sc * G.abs().t() @ (X.abs() @ dn.abs().t()), k=1e-4, msg=f"{what} d_up")
    close(ddn, sc * (G @ u).t() @ X, sc * (G.abs() @ u.abs()).t() @ X.abs(), k=1e-4, msg=f"{what} d_down")


FM_TABLES = [  # one table per (rank tile, LDS class): M = 1, M = k * rows_per_block + 1, head-padded G (q/k/v) or X (to_out)
    [(1, 320, 320, 1, None, None), (129, 320, 320, 3, (40, 64), None), (65, 320, 320, 3, None, (40, 64))],
    [(257, 640, 320, 5, None, None), (1, 320, 640, 5, None, None)],
    [(65, 320, 1280, 9, None, None), (129, 320, 320, 13, (40, 64), (40, 64)), (1, 320, 320, 16, None, None)],
    [(33, 1280, 640, 13, None, None), (97, 640, 640, 16, (80, 128), None)],
]


@case("lora_amd_factor_pack", "lora_amd_linear_bwd_factors_mfma_ragged")
def case_factors_mfma_ragged():
    """Every site of a table in one launch, slabs exactly as the plan sizes them with guards behind them, both LDS classes,
    ranks 1, 3, 5, 9, 13 and 16, with and without the block map."""
    for ti, rows in enumerate(FM_TABLES):
        sites = [_fm_site(M, K, N, r, 100 * ti + 10 * j, gh, xh) for j, (M, K, N, r, gh, xh) in enumerate(rows)]
        arr, total = _C.factor_pack_table([(s["down"], s["up"], s["pk_down"].data, s["pk_up"].data) for s in sites])
        _C.factor_pack(table(arr), len(sites), total, BF)
        check(*[s[k] for s in sites for k in ("pk_down", "pk_up")], what="factor_pack")
        for s in sites:
            RT = int(s["plan"].rank_tile)
            MG.assert_written(s["pk_down"].data[:2 * s["K"] * RT], "pk_down")
            MG.assert_written(s["pk_up"].data[:2 * s["N"] * RT], "pk_up")
        cls = max(int(s["plan"].lds_class) for s in sites)
        heights = {int(s["plan"].rows_per_block) for s in sites}
        rows_arg = heights.pop() if len(heights) == 1 else 0   # 0: a class-2 table of both block heights
        for mapped in (False, True):
            for s in sites:
                for k in ("up_part", "down_part"):
                    MG.fill_sentinel(s[k].data)
            arr, grid = _C.factors_mfma_table(
                [(s["g"], s["x"], s["pk_down"].data, s["pk_up"].data, s["up_part"].data, s["down_part"].data, s["scale"],
                  s["g_heads"], s["x_heads"], s["r"], s["plan"]) for s in sites], BF, cls)
            if mapped:
                raw, moff = _C.factors_mfma_table_bytes(arr, grid)
                tab = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
            else:
                tab, moff = table(arr), 0
            _C.linear_bwd_factors_mfma_ragged(tab, len(sites), grid, cls, BF, False, rows_arg, map_offset=moff)
            check(*[s[k] for s in sites for k in ("up_part", "down_part")], what="factors_mfma_ragged")
            for s in sites:
                _check_factor_grads(s, s["up_part"], s["down_part"], int(s["plan"].nparts), int(s["plan"].rank_tile),
                                    f"factors_mfma table {ti} mapped={mapped} M={s['M']} r={s['r']}")


@case("lora_amd_linear_bwd_factors_self", "lora_amd_linear_bwd_factors_self_ragged")
def case_factors_self():
    """The VALU factor pass: per site and as a one-launch table, M = 1 and one row past a block, head-padded G and X."""
    for M, K, N, r, gh, xh in ((1, 320, 320, 5, None, None), (129, 320, 320, 3, (40, 64), None),
                               (65, 328, 64, 16, None, None), (200, 320, 320, 9, None, (40, 64))):
        s = _fm_site(M, K, N, r, 7 * M + r, gh, xh, mfma=False)
        plan = _C.factors_self_plan(M, K, N, r)
        assert plan.supported
        upp, dnp = out(int(plan.up_part_floats)), out(int(plan.down_part_floats))
        _C.linear_bwd_factors_self(s["g"], s["x"], s["down"], s["up"], upp.data, dnp.data, s["scale"], s["g_heads"],
                                   s["x_heads"])
        check(upp, dnp, what="factors_self")
        _check_factor_grads(s, upp, dnp, int(plan.nparts), int(plan.rank_tile), f"factors_self M={M} r={r}")
    for rows in ([(1, 320, 320, 3, None, None), (129, 320, 320, 4, (40, 64), (40, 64))],
                 [(257, 640, 320, 16, None, None), (3, 320, 1280, 9, None, None)]):
        sites, slabs = [], []
        for M, K, N, r, gh, xh in rows:
            s = _fm_site(M, K, N, r, 3 * M + r, gh, xh, mfma=False)
            plan = _C.factors_self_plan(M, K, N, r, _C.SELF_ROWS_DEFERRED)
            upp, dnp = out(int(plan.up_part_floats)), out(int(plan.down_part_floats))
            sites.append(s)
            slabs.append((upp, dnp, plan))
        arr, grid = _C.factors_self_ragged_table(
            [(s["g"], s["x"], s["down"], s["up"], u.data, d.data, s["scale"], s["g_heads"], s["x_heads"])
             for s, (u, d, _) in zip(sites, slabs)], BF)
        _C.linear_bwd_factors_self_ragged(table(arr), len(sites), grid, sites[0]["r"], BF)
        check(*[g_ for u, d, _ in slabs for g_ in (u, d)], what="factors_self_ragged")
        for s, (u, d, plan) in zip(sites, slabs):
            _check_factor_grads(s, u, d, int(plan.nparts), int(plan.rank_tile), f"factors_self_ragged M={s['M']}")


# ----------------------------------------------------------------------------- merges
@case("lora_amd_merge_step")
def case_merge_step():
    """q / k / v as row ranges of ONE buffer (ld_out wider than a row, head-padded rows: pad rows never written) with
    their transposes side by side in a second buffer; an output projection with head-padded columns; a dense site with
    N one past a tile edge; both rounding modes.  Pads and gaps keep the sentinel."""
    N, K, r, d, D = 320, 320, 4, 40, 64
    Np = N // d * D
    for rounding in (_C.ROUND_ONCE, _C.ROUND_DITHER):
        qkv = out((3 * Np, K + 8), BF)                # + 8 gap columns no site writes
        qkv_t = out((K, 3 * Np + 16), BF)             # transposes side by side, + 16 gap columns
        w_o = out((N, K // d * D), BF)                # to_out: input head-padded
        dense = out((136, 72), BF)                     # N = 136 = 128 + 8, K = 72 = 8 x 9
        sites, refs = [], []
        for i in range(3):
            w = inp(rnd((N, K), BF, seed=i))
            up, dn = inp(rnd((N, r), F32, 0.05, seed=10 + i)), inp(rnd((r, K), F32, 0.1, seed=20 + i))
            o = qkv.data[i * Np:(i + 1) * Np, :K]
            ot = qkv_t.data[:, i * Np:(i + 1) * Np]
            sites.append(dict(w=w, up=up, down=dn, out=o, out_t=ot, row_heads=(d, D), key=i + 1))
            refs.append((w, up, dn, o, ot, (d, D), None))
        w = inp(rnd((N, K), BF, seed=5))
        up, dn = inp(rnd((N, r), F32, 0.05, seed=15)), inp(rnd((r, K), F32, 0.1, seed=25))
        sites.append(dict(w=w, up=up, down=dn, out=w_o.data, col_heads=(d, D), key=7))
        refs.append((w, up, dn, w_o.data, None, None, (d, D)))
        w = inp(rnd((136, 72), BF, seed=6))
        up, dn = inp(rnd((136, 16), F32, 0.05, seed=16)), inp(rnd((16, 72), F32, 0.1, seed=26))
        sites.append(dict(w=w, up=up, down=dn, out=dense.data, key=9))
        refs.append((w, up, dn, dense.data, None, None, None))
        plan = _C.MergeStepPlan(sites)
        plan.launch(0.9, rounding)
        check(qkv, qkv_t, w_o, dense, what="merge_step")
        MG.assert_untouched(qkv.data[:, K:], "qkv gap columns")
        MG.assert_untouched(qkv_t.data[:, 3 * Np:], "qkv_t gap columns")
        for w, up, dn, o, ot, rh, ch in refs:
            Nn, Kk = w.shape
            rows = heads_cols(Nn, *rh) if rh else torch.arange(Nn, device=DEV)
            cols = heads_cols(Kk, *ch) if ch else torch.arange(Kk, device=DEV)
            want = d64(w) + 0.9 * d64(up) @ d64(dn)
            ref = d64(w).abs() + 0.9 * d64(up).abs() @ d64(dn).abs()
            got = o[rows][:, cols]
            # nearest: half an ulp of the f32-accumulated value; dither: within one ulp
            close(got, want, ref, BF, k=2e-5, eps=2.0 ** -8 if rounding == _C.ROUND_ONCE else 2.0 ** -7,
                  msg=f"merge_step W_eff rounding {rounding}")
            keep = torch.ones(o.shape, dtype=torch.bool, device=DEV)
            keep[rows[:, None], cols[None, :]] = False
            MG.assert_untouched(o[keep], "merge_step pads")
            if ot is not None:
                assert torch.equal(ot[cols][:, rows], got.t()), "W_eff^T differs from W_eff"
                keep_t = torch.ones(ot.shape, dtype=torch.bool, device=DEV)
                keep_t[cols[:, None], rows[None, :]] = False
                MG.assert_untouched(ot[keep_t], "merge_step transposed pads")


@case("lora_amd_merge_batched")
def case_merge_batched():
    """Sites of one plan: N one past a tile, K % 8 != 0 and K = 8 x odd (slab kernel), K = 32 x odd (column-owner tile
    ct8 = 4), a transposed site, a head-padded output with d < D; f32 in reference rounding, bf16 rounded once."""
    for wdt, rounding in ((F32, _C.ROUND_REFERENCE), (BF, _C.ROUND_ONCE)):
        spec = [(129, 321, 4, False, None), (17, 328, 3, False, None), (65, 96, 16, False, None), (1, 8, 1, False, None),
                (320, 160, 4, True, None), (64, 320, 8, False, (40, 64))]
        sites, checks = [], []
        for i, (N, K, r, tr, hd) in enumerate(spec):
            w = inp(rnd((N, K), wdt, seed=i))
            if tr:  # the transposed product: w [N = original K, K = original N]; up = original down [r, N], down = original up [K, r]
                up, dn = inp(rnd((r, N), wdt, 0.1, seed=10 + i)), inp(rnd((K, r), wdt, 0.05, seed=20 + i))
                prod = d64(dn).mm(d64(up)).t()
                prod_abs = d64(dn).abs().mm(d64(up).abs()).t()
            else:
                up, dn = inp(rnd((N, r), wdt, 0.05, seed=10 + i)), inp(rnd((r, K), wdt, 0.1, seed=20 + i))
                prod, prod_abs = d64(up) @ d64(dn), d64(up).abs() @ d64(dn).abs()
            o = out((N, K // hd[0] * hd[1]) if hd else (N, K), wdt)
            sites.append((w, o.data, up, dn, hd, tr))
            checks.append((w, o, prod, prod_abs, hd))
        plan = _C.MergePlan(sites)
        plan.launch(0.7, rounding)
        check(*[c[1] for c in checks], what="merge_batched")
        for w, o, prod, prod_abs, hd in checks:
            N, K = w.shape
            cols = heads_cols(K, *hd) if hd else torch.arange(K, device=DEV)
            got = o.data[:, cols]
            close(got, d64(w) + 0.7 * prod, d64(w).abs() + 0.7 * prod_abs, wdt, k=2e-5, msg=f"merge_batched N={N} K={K}")
            if hd:
                keep = torch.ones(o.data.shape, dtype=torch.bool, device=DEV)
                keep[:, cols] = False
                MG.assert_untouched(o.data[keep], "merge_batched pad columns")


# ----------------------------------------------------------------------------- optimiser
@case("lora_amd_sumsq")
def case_sumsq():
    for n in (1, 4097, 3 * 65536 + 5):
        g = inp(rnd((n,), seed=n))
        ws_bytes = int(lib().lora_amd_sumsq_workspace(n))
        ws, o = out(max(ws_bytes // 4, 1)), out(1)
        ok(lib().lora_amd_sumsq(g.data_ptr(), n, o.ptr, ws.ptr, ws_bytes, stream()), "sumsq")
        check(ws, o, what="sumsq")
        close(o.data, (d64(g) ** 2).sum().view(1), (d64(g) ** 2).sum().view(1), k=2e-5, msg="sumsq")


ADAMW_GROUPS = [(0, 13, 1e-3, 0.01), (20, 517, 2e-3, 0.0), (600, 1001, 5e-4, 0.1)]   # gaps 13..20, 517..600, 1001..1003


def _adamw_ref(p, g, m, v, coef, step, b1=0.9, b2=0.999, eps=1e-8):
    p, g, m, v = d64(p), d64(g) * coef, d64(m), d64(v)
    P, Mm, V = p.clone(), m.clone(), v.clone()
    for b, e, lr, wd in ADAMW_GROUPS:
        sl = slice(b, e)
        Mm[sl] = b1 * m[sl] + (1 - b1) * g[sl]
        V[sl] = b2 * v[sl] + (1 - b2) * g[sl] ** 2
        denom = V[sl].sqrt() / math.sqrt(1 - b2 ** step) + eps
        P[sl] = p[sl] * (1 - lr * wd) - lr / (1 - b1 ** step) * Mm[sl] / denom
    return P, Mm, V


def _owned(n):
    own = torch.zeros(n, dtype=torch.bool, device=DEV)
    for b, e, _, _ in ADAMW_GROUPS:
        own[b:e] = True
    return own


@case("lora_amd_clip_adamw", "lora_amd_step_advance", "lora_amd_loss_scale_update")
def case_clip_adamw():
    """Groups with gaps: p, g, m, v outside every group stay bit-unchanged; the device-step form with the loss-scaling
    flag set and not set; step_advance and loss_scale_update on guarded words."""
    n = 1003
    own = _owned(n)
    groups = _C.make_adamw_groups(ADAMW_GROUPS, DEV)
    p0, g0, m0, v0 = rnd((n,), seed=1), rnd((n,), seed=2, scale=0.1), rnd((n,), seed=3, scale=0.01), rnd((n,), seed=4).abs() * 1e-3
    sumsq = inp((g0.double() ** 2).sum().float().view(1))
    max_norm = 0.5
    coef = min(1.0, max_norm / (math.sqrt(float(sumsq)) + 1e-6))
    for form in ("host", "dev", "dev_skip"):
        P, G, Mm, V = (MG.guarded_like(t) for t in (p0, g0, m0, v0))
        if form == "host":
            ok(lib().lora_amd_clip_adamw(P.ptr, G.ptr, Mm.ptr, V.ptr, n, groups.data_ptr(), len(ADAMW_GROUPS),
                                         sumsq.data_ptr(), 1.0, max_norm, 0.9, 0.999, 1e-8, 3, None, None, 1, stream()),
               "clip_adamw")
            c = coef
        else:
            step = out(1, torch.int64, fill=torch.tensor([3], device=DEV))
            scaler = inp(torch.tensor([1024.0, 0.0, 0.5, 0.0 if form == "dev_skip" else 1.0], device=DEV))
            ok(lib().lora_amd_clip_adamw(P.ptr, G.ptr, Mm.ptr, V.ptr, n, groups.data_ptr(), len(ADAMW_GROUPS),
                                         sumsq.data_ptr(), 1.0, max_norm, 0.9, 0.999, 1e-8, 0, step.ptr, scaler.data_ptr(),
                                         1, stream()), "clip_adamw device step")
            check(step, what="clip_adamw device step")
            c = 0.5 * min(1.0, max_norm / (math.sqrt(float(sumsq)) * 0.5 + 1e-6))
        check(P, G, Mm, V, what=f"clip_adamw {form}")
        for got, base in ((P, p0), (G, g0), (Mm, m0), (V, v0)):
            assert torch.equal(MG._bits(got.data)[~own], MG._bits(base)[~own]), f"{form}: element outside every group changed"
        assert bool((G.data[own] == 0).all()), f"{form}: gradient not zeroed in the groups"
        if form == "dev_skip":
            for got, base in ((P, p0), (Mm, m0), (V, v0)):
                assert torch.equal(got.data, base), "skipped update changed the state"
            continue
        Pw, Mw, Vw = _adamw_ref(p0, g0, m0, v0, c, 3)
        refs = {"p": d64(p0).abs() + 0.05, "m": 0.9 * d64(m0).abs() + 0.1 * c * d64(g0).abs(), "v": Vw.abs()}
        for got, want, nm in ((P, Pw, "p"), (Mm, Mw, "m"), (V, Vw, "v")):
            close(got.data[own], want[own], refs[nm][own], k=2e-5, msg=f"adamw {form} {nm}")
    # n = 1: one element, one group, the tail loop only
    P1, G1, M1, V1 = (MG.guarded_like(t[:1].clone()) for t in (p0, g0, m0, v0))
    g1 = _C.make_adamw_groups([(0, 1, 1e-3, 0.01)], DEV)
    ss1 = inp((g0[:1].double() ** 2).float())
    ok(lib().lora_amd_clip_adamw(P1.ptr, G1.ptr, M1.ptr, V1.ptr, 1, g1.data_ptr(), 1, ss1.data_ptr(), 1.0, 0.0, 0.9, 0.999,
                                 1e-8, 1, None, None, 1, stream()), "clip_adamw n=1")
    check(P1, G1, M1, V1, what="clip_adamw n=1")
    gg, bc2 = float(g0[0]), math.sqrt(1 - 0.999)
    mw, vw = 0.9 * float(m0[0]) + 0.1 * gg, 0.999 * float(v0[0]) + 0.001 * gg * gg
    pw = float(p0[0]) * (1 - 1e-5) - 1e-3 / 0.1 * mw / (math.sqrt(vw) / bc2 + 1e-8)
    for got, want in ((P1, pw), (M1, mw), (V1, vw)):
        assert abs(float(got.data) - want) <= 2e-5 * (abs(want) + 1e-3), (float(got.data), want)
    assert float(G1.data) == 0.0
    step = out(1, torch.int64, fill=torch.tensor([41], device=DEV))
    ok(lib().lora_amd_step_advance(step.ptr, stream()), "step_advance")
    check(step, what="step_advance")
    assert int(step.data) == 42
    for finite in (True, False):
        state = out(4, fill=torch.tensor([1024.0, 5.0, 0.0, 0.0], device=DEV))
        ss = inp(torch.tensor([3.0 if finite else float("inf")], device=DEV))
        step = out(1, torch.int64, fill=torch.tensor([7], device=DEV))
        ok(lib().lora_amd_loss_scale_update(state.ptr, ss.data_ptr(), step.ptr, 2.0, 0.5, 6, stream()), "loss_scale_update")
        check(state, step, what="loss_scale_update")
        want = [2048.0, 0.0, 1 / 1024.0, 1.0] if finite else [512.0, 0.0, 1 / 1024.0, 0.0]
        assert state.data.tolist() == want and int(step.data) == (8 if finite else 7)


@case("lora_amd_ti_rows_step")
def case_ti_rows_step():
    """Placeholder rows of an embedding table: rows not listed stay bit-unchanged; the listed rows equal the launch on
    plain allocations bit for bit (tests/test_gpu_kernels.py checks that one against a full-table AdamW)."""
    vocab, hidden = 37, 72
    ids = torch.tensor([3, 36, 0], dtype=torch.int64, device=DEV)
    for dt in (F32, BF):
        tab0, grad = rnd((vocab, hidden), dt, seed=1), inp(rnd((vocab, hidden), dt, 0.1, seed=2))
        rows0 = tab0[ids].float()
        res = []
        for guarded in (False, True):
            bufs = [MG.guarded_like(t) if guarded else t.clone()
                    for t in (tab0, rows0, torch.zeros_like(rows0), torch.zeros_like(rows0))]
            tab, rows, m, v = (b.data if guarded else b for b in bufs)
            ok(lib().lora_amd_ti_rows_step(tab.data_ptr(), grad.data_ptr(), ids.data_ptr(), 3, hidden, _C.dtype_code(dt),
                                           rows.data_ptr(), m.data_ptr(), v.data_ptr(), 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1,
                                           0.1, 0.4, stream()), "ti_rows_step")
            if guarded:
                check(*bufs, what="ti_rows_step")
            res.append((tab, rows, m, v))
        keep = torch.ones(vocab, dtype=torch.bool, device=DEV)
        keep[ids] = False
        assert torch.equal(MG._bits(res[1][0][keep]), MG._bits(tab0[keep])), "unlisted rows changed"
        assert not torch.equal(res[1][0][ids], tab0[ids])
        for a, b in zip(*res):
            assert torch.equal(MG._bits(a), MG._bits(b))


# ----------------------------------------------------------------------------- host passes
@case("lora_amd_layernorm_fwd", "lora_amd_layernorm_bwd")
def case_layernorm():
    """The smallest and odd supported widths (K = 8, 72, 2560), M = 1 and odd; stats guarded."""
    for M, K in ((1, 8), (5, 72), (3, 2560)):
        for dt in (F32, BF):
            x, res = inp(rnd((M, K), dt, 1.5, seed=1)), inp(rnd((M, K), dt, 1.0, seed=2))
            gamma, beta = inp(rnd((K,), dt, 0.5, seed=3) + 1), inp(rnd((K,), dt, 0.3, seed=4))
            gout, gsum = inp(rnd((M, K), dt, seed=5)), inp(rnd((M, K), dt, seed=6))
            y, st = out((M, K), dt), out((M, 2))
            ok(lib().lora_amd_layernorm_fwd(x.data_ptr(), None, gamma.data_ptr(), beta.data_ptr(), None, y.ptr, st.ptr, M, K,
                                            1e-5, _C.dtype_code(dt), stream()), "layernorm_fwd")
            dx = out((M, K), dt)
            ok(lib().lora_amd_layernorm_bwd(x.data_ptr(), gout.data_ptr(), None, gamma.data_ptr(), st.ptr, dx.ptr, M, K,
                                            _C.dtype_code(dt), stream()), "layernorm_bwd")
            s2, y2, st2, dx2 = out((M, K), dt), out((M, K), dt), out((M, 2)), out((M, K), dt)
            ok(lib().lora_amd_layernorm_fwd(x.data_ptr(), res.data_ptr(), gamma.data_ptr(), beta.data_ptr(), s2.ptr,
                                            y2.ptr, st2.ptr, M, K, 1e-5, _C.dtype_code(dt), stream()), "layernorm_fwd with res")
            ok(lib().lora_amd_layernorm_bwd(s2.ptr, gout.data_ptr(), gsum.data_ptr(), gamma.data_ptr(), st2.ptr, dx2.ptr,
                                            M, K, _C.dtype_code(dt), stream()), "layernorm_bwd with gsum")
            check(y, st, dx, s2, y2, st2, dx2, what=f"layernorm M={M} K={K}")
            y3, st3 = out((M, K), dt), out((M, 2))  # the wrapper into a caller's buffers
            _C.layernorm_fwd(x, gamma, beta, 1e-5, out=y3.data, stats=st3.data)
            check(y3, st3, what="layernorm_fwd(out=)")
            assert torch.equal(y3.data, y.data) and torch.equal(st3.data, st.data)
            tol = dict(rtol=1e-4 if dt == F32 else 2.0 ** -7, atol=2e-5 if dt == F32 else 2e-2)
            for xin, yo, dxo, gs in ((x, y, dx, None), (None, y2, dx2, gsum)):
                xr = (x.float() if xin is not None else (x.float() + res.float()).to(dt).float()).detach().clone()
                xr.requires_grad_(True)
                if xin is None:
                    assert torch.equal(s2.data, (x + res)), "add_layernorm sum"
                yr = F.layer_norm(xr, (K,), gamma.float(), beta.float(), 1e-5)
                yr.backward(gout.float())
                torch.testing.assert_close(yo.data.float(), yr.detach(), **tol)
                want = xr.grad + (gs.float() if gs is not None else 0)
                torch.testing.assert_close(dxo.data.float(), want, rtol=tol["rtol"],
                                           atol=tol["atol"] * (float(want.abs().max()) + 1e-6))


@case("lora_amd_geglu_fwd", "lora_amd_geglu_bwd")
def case_geglu():
    """M = 1 and odd inner widths, strided y / gout / output rows (ld > width, NaN gaps, gaps of the outputs untouched)."""
    for M, inner in ((1, 8), (7, 40), (3, 1288)):
        for dt in (F32, BF):
            y = inp(rnd((M, 2 * inner), dt, 2.0, seed=inner), ld=2 * inner + 8)
            gout = inp(rnd((M, inner), dt, seed=inner + 1), ld=inner + 16)
            o = out((M, inner + 8), dt)
            gy = out((M, 2 * inner + 24), dt)
            ok(lib().lora_amd_geglu_fwd(y.data_ptr(), y.stride(0), o.ptr, inner + 8, M, inner, _C.dtype_code(dt), stream()),
               "geglu_fwd")
            ok(lib().lora_amd_geglu_bwd(y.data_ptr(), y.stride(0), gout.data_ptr(), gout.stride(0), gy.ptr, 2 * inner + 24,
                                        M, inner, _C.dtype_code(dt), stream()), "geglu_bwd")
            check(o, gy, what="geglu")
            o2 = out((M, inner), dt)        # the wrapper into a caller's buffer (row-contiguous y)
            _C.geglu_fwd(y.contiguous(), out=o2.data)
            check(o2, what="geglu_fwd(out=)")
            assert torch.equal(o2.data, o.data[:, :inner])
            MG.assert_untouched(o.data[:, inner:], "geglu out row gap")
            MG.assert_untouched(gy.data[:, 2 * inner:], "geglu gy row gap")
            yr = y.float().requires_grad_(True)
            h, gate = yr.chunk(2, dim=-1)
            outr = h * F.gelu(gate)
            outr.backward(gout.float())
            tol = dict(rtol=1e-4 if dt == F32 else 2.0 ** -7, atol=2e-5 if dt == F32 else 2e-2)
            torch.testing.assert_close(o.data[:, :inner].float(), outr.detach(), **tol)
            torch.testing.assert_close(gy.data[:, :2 * inner].float(), yr.grad, rtol=tol["rtol"],
                                       atol=tol["atol"] * (float(yr.grad.abs().max()) + 1e-6))


@case("lora_amd_groupnorm_fwd", "lora_amd_groupnorm_bwd", "lora_amd_groupnorm_nhwc_fwd", "lora_amd_groupnorm_nhwc_bwd")
def case_groupnorm():
    """The smallest and odd supported geometries, B = 1; stats, per-channel terms and workspaces guarded."""
    for B, Cc, Hh, Ww, G in ((1, 8, 1, 8, 8), (2, 96, 2, 4, 3), (1, 40, 3, 8, 5)):
        HW = Hh * Ww
        for dt in (F32, BF):
            x = inp(rnd((B, Cc, Hh, Ww), dt, 1.5, seed=1) + 0.5)
            gamma, beta = inp(rnd((Cc,), dt, 0.5, seed=2) + 1), inp(rnd((Cc,), dt, 0.3, seed=3))
            gout = inp(rnd((B, Cc, Hh, Ww), dt, seed=4))
            xr = x.float().requires_grad_(True)
            yr = F.silu(F.group_norm(xr, G, gamma.float(), beta.float(), 1e-5))
            yr.backward(gout.float())
            tol = dict(rtol=1e-4 if dt == F32 else 2.0 ** -7, atol=2e-5 if dt == F32 else 2e-2)
            gscale = float(xr.grad.abs().max()) + 1e-6
            # NCHW
            wsb = int(lib().lora_amd_groupnorm_workspace(B, Cc, HW, G))
            assert wsb > 0 and lib().lora_amd_groupnorm_supported(B, Cc, HW, G) == 1
            y, st, ws, dx = out((B, Cc, Hh, Ww), dt), out((B * G, 2)), out(wsb // 4), out((B, Cc, Hh, Ww), dt)
            ok(lib().lora_amd_groupnorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.ptr, st.ptr, ws.ptr, wsb, B, Cc,
                                            HW, G, 1e-5, 1, _C.dtype_code(dt), stream()), "groupnorm_fwd")
            ok(lib().lora_amd_groupnorm_bwd(x.data_ptr(), gout.data_ptr(), gamma.data_ptr(), beta.data_ptr(), st.ptr, dx.ptr,
                                            ws.ptr, wsb, B, Cc, HW, G, 1, _C.dtype_code(dt), stream()), "groupnorm_bwd")
            check(y, st, ws, dx, what="groupnorm")
            torch.testing.assert_close(y.data.float(), yr.detach(), **tol)
            torch.testing.assert_close(dx.data.float(), xr.grad, rtol=tol["rtol"], atol=tol["atol"] * gscale)
            # channels-last (memory [B][HW][C]; needs C % 8 == 0)
            if Cc % 8:
                continue
            xl = inp(x.permute(0, 2, 3, 1).contiguous())
            gl_ = inp(gout.permute(0, 2, 3, 1).contiguous())
            wsb = int(lib().lora_amd_groupnorm_nhwc_workspace(B, Cc, HW, G))
            assert wsb > 0
            y, aff, ws, dx = out((B, Hh, Ww, Cc), dt), out((B, 4, Cc)), out(wsb // 4), out((B, Hh, Ww, Cc), dt)
            ok(lib().lora_amd_groupnorm_nhwc_fwd(xl.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, y.ptr, aff.ptr,
                                                 ws.ptr, wsb, B, Cc, HW, G, 1e-5, 1, _C.dtype_code(dt), stream()),
               "groupnorm_nhwc_fwd")
            ok(lib().lora_amd_groupnorm_nhwc_bwd(xl.data_ptr(), gl_.data_ptr(), None, Cc, gamma.data_ptr(), aff.ptr, dx.ptr,
                                                 ws.ptr, wsb, B, Cc, HW, G, 1, _C.dtype_code(dt), stream()),
               "groupnorm_nhwc_bwd")
            check(y, aff, ws, dx, what="groupnorm_nhwc")
            torch.testing.assert_close(y.data.permute(0, 3, 1, 2).float(), yr.detach(), **tol)
            torch.testing.assert_close(dx.data.permute(0, 3, 1, 2).float(), xr.grad, rtol=tol["rtol"], atol=tol["atol"] * gscale)


# ----------------------------------------------------------------------------- streaming K1 / K2 primitives
def _mask(M, N, p, seed, off):
    """The dropout multiplier of element (m, n) of a dense [M, N] operand (tests/helpers restates the kernels' Philox)."""
    if p == 0:
        return torch.ones(M, N, dtype=torch.float64, device=DEV)
    n8 = -(-(M * N) // 8) * 8
    return H.philox_dropout_mask(n8, p, seed, off)[:M * N].view(M, N).double().to(DEV)


STREAM_SHAPES = [  # M, K, N, r, x dtype: M = 1, K / N not multiples of a wave's chunk, ranks 9..16 (matrix-core forms)
    (1, 8, 8, 1, BF), (33, 77, 41, 5, F32), (130, 1288, 320, 16, BF), (257, 328, 2568, 13, BF), (64, 320, 648, 9, BF)]


@case("lora_amd_rowdot", "lora_amd_rank_update", "lora_amd_rank_update_rowscale", "lora_amd_colreduce")
def case_streaming():
    """Strided X / Y rows with NaN in the row gaps (Y's gaps must stay untouched), dropout, a row table that wraps."""
    s_, p, seed, off = 0.7, 0.25, 0x5EED, 11
    for M, K, N, r, dt in STREAM_SHAPES:
        dc = _C.dtype_code(dt)
        x = inp(rnd((M, K), dt, seed=1), ld=K + 8)
        f = inp(rnd((r, K), F32, 0.3, seed=2))
        X, Fd = d64(x), d64(f)
        for masked in (False, True):
            t = out((M, r))
            if masked:
                ok(lib().lora_amd_rowdot(x.data_ptr(), K + 8, f.data_ptr(), t.ptr, M, K, r, dc, _C.F32, _C.FACTOR_RK, s_,
                                         None, 0, p, seed, off, None, stream()), "rowdot masked")
                Xm = X * _mask(M, K, p, seed, off)
            else:
                ok(lib().lora_amd_rowdot(x.data_ptr(), K + 8, f.data_ptr(), t.ptr, M, K, r, dc, _C.F32, _C.FACTOR_RK, s_,
                                         None, 0, 0.0, 0, 0, None, stream()), "rowdot")
                Xm = X
            check(t, what="rowdot")
            close(t.data, s_ * Xm @ Fd.t(), s_ * Xm.abs() @ Fd.abs().t(), msg=f"rowdot masked={masked} M={M} K={K} r={r}")
            t2 = out((M, r))    # the same through the wrapper, into a caller's buffer
            assert _C.rowdot(x, f, _C.FACTOR_RK, s_, dropout_p=p if masked else 0.0, seed=seed, offset=off,
                             out=t2.data) is t2.data
            check(t2, what="rowdot(out=)")
            close(t2.data, s_ * Xm @ Fd.t(), s_ * Xm.abs() @ Fd.abs().t(), msg="rowdot(out=)")
        T = inp(rnd((M, r), F32, 0.5, seed=3))
        up = inp(rnd((N, r), F32, 0.2, seed=4))
        y0 = rnd((M, N), dt, seed=5)
        nsel, rps = 3, 1 if M % 2 else 2                              # rows-per-sample 1 and a table that wraps
        rs = inp(rnd((nsel, r), F32, 1.0, seed=6))
        for form in ("plain", "rowscale"):
            y = out((M, N + 8), dt)
            y.data[:, :N] = y0
            if form == "plain":
                ok(lib().lora_amd_rank_update(y.ptr, N + 8, T.data_ptr(), up.data_ptr(), M, N, r, dc, _C.F32, _C.FACTOR_KR,
                                              s_, p, seed, off, None, stream()), "rank_update")
                Tm = d64(T)
            else:
                ok(lib().lora_amd_rank_update_rowscale(y.ptr, N + 8, T.data_ptr(), up.data_ptr(), M, N, r, dc, _C.F32,
                                                       _C.FACTOR_KR, s_, rs.data_ptr(), nsel, rps, p, seed, off, stream()),
                   "rank_update_rowscale")
                Tm = d64(T) * d64(rs)[(torch.arange(M, device=DEV) // rps) % nsel]
            check(y, what=f"rank_update {form}")
            MG.assert_untouched(y.data[:, N:], f"rank_update {form} row gaps")
            mk = _mask(M, N, p, seed, off)
            close(y.data[:, :N], d64(y0) + s_ * mk * (Tm @ d64(up).t()), d64(y0).abs() + s_ * mk * (Tm.abs() @ d64(up).abs().t()),
                  dt, msg=f"rank_update {form} M={M} N={N} r={r}")
        wsb = int(lib().lora_amd_colreduce_workspace(M, K, r))
        ws = out(max(wsb // 4, 1))
        d0 = rnd((r, K), F32, seed=7)
        D = MG.guarded_like(d0)
        ok(lib().lora_amd_colreduce(x.data_ptr(), K + 8, T.data_ptr(), D.ptr, M, K, r, dc, _C.FACTOR_RK, s_, 1.0, p, seed, off,
                                    None, ws.ptr, wsb, stream()), "colreduce")
        check(ws, D, what="colreduce")
        Xm = X * _mask(M, K, p, seed, off)
        close(D.data, d64(d0) + s_ * d64(T).t() @ Xm, d64(d0).abs() + s_ * d64(T).abs().t() @ Xm.abs(),
              msg=f"colreduce M={M} K={K} r={r}")


# ----------------------------------------------------------------------------- per-site fused kernels
LINEAR_SHAPES = [(1, 320, 320, 4), (129, 640, 10240, 16), (97, 320, 1280, 9), (65, 320, 640, 3)]


@case("lora_amd_linear_fwd", "lora_amd_linear_bwd_g", "lora_amd_linear_bwd_x")
def case_linear_fused():
    """The fused forward and the two backward passes on strided X, Y, G, dX (NaN row gaps; Y / dX gaps untouched),
    partial slabs exactly as lora_amd_linear_plan sizes them, M = 1 and one row past a block, the widest N."""
    s_ = 0.7
    for M, K, N, r in LINEAR_SHAPES:
        lp = _C.linear_plan(M, K, N, r)
        assert lp.fused == 1
        x, g = inp(rnd((M, K), BF, seed=1), ld=K + 8), inp(rnd((M, N), BF, seed=2), ld=N + 8)
        down, up = inp(rnd((r, K), F32, 0.3, seed=3)), inp(rnd((N, r), F32, 0.2, seed=4))
        y0, dx0 = rnd((M, N), BF, seed=5), rnd((M, K), BF, seed=6)
        y, t = out((M, N + 8), BF), out((M, r))
        y.data[:, :N] = y0
        ok(lib().lora_amd_linear_fwd(x.data_ptr(), K + 8, y.ptr, N + 8, down.data_ptr(), up.data_ptr(), t.ptr, M, K, N, r,
                                     _C.BF16, _C.F32, s_, None, 0.0, 0, 0, None, stream()), "linear_fwd")
        gp, upp, dnp = out(int(lp.gt_part_floats)), out(int(lp.up_part_floats)), out(int(lp.down_part_floats))
        ok(lib().lora_amd_linear_bwd_g(g.data_ptr(), N + 8, t.ptr, up.data_ptr(), gp.ptr, upp.ptr, M, N, r, _C.BF16, _C.F32,
                                       s_, 0.0, 0, 0, None, stream()), "linear_bwd_g")
        dx = out((M, K + 8), BF)
        dx.data[:, :K] = dx0
        ok(lib().lora_amd_linear_bwd_x(x.data_ptr(), K + 8, dx.ptr, K + 8, gp.ptr, int(lp.nct_g), down.data_ptr(), None,
                                       dnp.ptr, M, K, r, _C.BF16, _C.F32, stream()), "linear_bwd_x")
        check(y, t, gp, upp, dnp, dx, what=f"linear fused M={M} N={N}")
        MG.assert_untouched(y.data[:, N:], "linear_fwd y row gaps")
        MG.assert_untouched(dx.data[:, K:], "linear_bwd_x dx row gaps")
        X, G, A, U = d64(x), d64(g), d64(down), d64(up)
        T = X @ A.t()
        close(t.data, T, X.abs() @ A.abs().t(), msg="linear_fwd T")
        close(y.data[:, :N], d64(y0) + s_ * d64(t.data) @ U.t(), d64(y0).abs() + s_ * d64(t.data).abs() @ U.abs().t(), BF,
              msg="linear_fwd Y")
        Gt = s_ * G @ U
        close(d64(gp.data).view(int(lp.nct_g), M, r).sum(0), Gt, s_ * G.abs() @ U.abs(), msg="linear_bwd_g Gt")
        RT = int(lp.rank_tile)
        dup = d64(upp.data).view(int(lp.nparts_up), RT, N)[:, :r].sum(0)
        close(dup, s_ * d64(t.data).t() @ G, s_ * d64(t.data).abs().t() @ G.abs(), msg="linear_bwd_g dUp")
        ddn = d64(dnp.data).view(int(lp.nparts_down), RT, K)[:, :r].sum(0)
        close(ddn, Gt.t() @ X, Gt.abs().t() @ X.abs(), msg="linear_bwd_x dDown")
        close(dx.data[:, :K], d64(dx0) + Gt @ A, d64(dx0).abs() + Gt.abs() @ A.abs(), BF, msg="linear_bwd_x dX")


@case("lora_amd_linear_bwd_factors")
def case_linear_bwd_factors():
    """Both partial slabs in one launch for sites whose Gt came out of the GEMM: dense and strided, dropout on G, head-padded
    G and X with NaN pads."""
    s_, p, seed, off = 0.6, 0.2, 77, 3
    for M, K, N, r, form in ((1, 320, 320, 4, "plain"), (129, 640, 1280, 16, "drop"), (65, 320, 320, 9, "heads"),
                             (200, 320, 320, 3, "plain")):
        lp = _C.linear_plan(M, K, N, r)
        g_log, x_log = rnd((M, N), BF, seed=1), rnd((M, K), BF, seed=2)
        if form == "heads":
            g, x, gw, xw = padded(g_log, 40, 64), padded(x_log, 40, 64), N // 40 * 64, K // 40 * 64
        else:
            g, x, gw, xw = inp(g_log, ld=N + 8), inp(x_log, ld=K + 8), N + 8, K + 8
        t, gt = inp(rnd((M, r), F32, 0.5, seed=3)), inp(rnd((M, r), F32, 0.5, seed=4))
        upp, dnp = out(int(lp.up_part_floats)), out(int(lp.down_part_floats))
        if form == "drop":
            ok(lib().lora_amd_linear_bwd_factors(g.data_ptr(), gw, t.data_ptr(), upp.ptr, x.data_ptr(), xw, gt.data_ptr(),
                                                 None, dnp.ptr, M, K, N, r, _C.BF16, s_, 0, 0, 0, 0, p, seed, off, None,
                                                 stream()), "linear_bwd_factors with dropout")
        elif form == "heads":
            ok(lib().lora_amd_linear_bwd_factors(g.data_ptr(), gw, t.data_ptr(), upp.ptr, x.data_ptr(), xw, gt.data_ptr(),
                                                 None, dnp.ptr, M, K, N, r, _C.BF16, s_, 40, 64, 40, 64, 0.0, 0, 0, None,
                                                 stream()), "linear_bwd_factors with heads")
        else:
            ok(lib().lora_amd_linear_bwd_factors(g.data_ptr(), gw, t.data_ptr(), upp.ptr, x.data_ptr(), xw, gt.data_ptr(),
                                                 None, dnp.ptr, M, K, N, r, _C.BF16, s_, 0, 0, 0, 0, 0.0, 0, 0, None,
                                                 stream()), "linear_bwd_factors")
        check(upp, dnp, what=f"linear_bwd_factors {form}")
        G = d64(g_log) * (_mask(M, N, p, seed, off) if form == "drop" else 1.0)
        X, T, Gt = d64(x_log), d64(t), d64(gt)
        RT = int(lp.rank_tile)
        dup = d64(upp.data).view(int(lp.nparts_up), RT, N)[:, :r].sum(0)
        ddn = d64(dnp.data).view(int(lp.nparts_down), RT, K)[:, :r].sum(0)
        close(dup, s_ * T.t() @ G, s_ * T.abs().t() @ G.abs(), msg=f"bwd_factors {form} dUp")
        close(ddn, Gt.t() @ X, Gt.abs().t() @ X.abs(), msg=f"bwd_factors {form} dDown")


# ----------------------------------------------------------------------------- the MFMA GEMM + LoRA forms
GEMM_M = 129   # one row past 128 / 64 / 32: every tile shape (64x320, 64x160, 32x160, 128x160) has a partial last row tile


def _gemm_ref(X, W, b, A, U, s_, rs=None, mask=None):
    """T, Y and the bound of Y: T rounded to the activation dtype before the up-projection (the reference's autocast),
    s * up rounded as the kernels' operand, ``mask`` = the dropout multiplier of the low-rank term."""
    T = X @ A.t()
    T16 = d64(T.to(BF)) if rs is None else d64((T * rs).to(BF))
    U16 = d64((s_ * U).to(BF))
    mk = 1.0 if mask is None else mask
    return T, X @ W.t() + b + mk * (T16 @ U16.t()), X.abs() @ W.abs().t() + b.abs() + mk * (T.abs() @ U16.abs().t())


@case("lora_amd_linear_gemm_fwd", "lora_amd_linear_gemm_fwd_rowscale")
def case_linear_gemm():
    """M not a multiple of any tile for every tile choice the tests pin (21-24, 31-34), N = 328 (a partial column tile),
    strided X / Y, head-padded X and Y (Y's pads written as zeros), per-sample multipliers with a row table that wraps."""
    s_, ts, M, K, N, r = 0.7, 0.5, GEMM_M, 320, 328, 4
    x, w = inp(rnd((M, K), BF, seed=1), ld=K + 64), inp(rnd((N, K), BF, 0.05, seed=2))
    b = inp(rnd((N,), BF, 0.5, seed=3))
    down, up = inp(rnd((r, K), F32, 0.2, seed=4)), inp(rnd((N, r), F32, 0.3, seed=5))
    X, W, B_, A, U = d64(x), d64(w), d64(b), d64(down), d64(up)
    T, Y, Yabs = _gemm_ref(X, W, B_, A, U, s_)
    assert lib().lora_amd_linear_gemm_supported(M, K, N, r, _C.BF16) == 1
    for tile in (0, 21, 22, 23, 24, 31, 32, 33, 34):
        y, t = out((M, N + 8), BF), out((M, r))
        ok(lib().lora_amd_linear_gemm_fwd(x.data_ptr(), K + 64, w.data_ptr(), K, b.data_ptr(), y.ptr, N + 8, down.data_ptr(),
                                          up.data_ptr(), t.ptr, M, K, N, r, _C.BF16, s_, ts, 0, tile, 0, 0, 0, 0, stream()),
           "linear_gemm_fwd")
        check(y, t, what=f"linear_gemm_fwd tile {tile}")
        MG.assert_untouched(y.data[:, N:], "gemm y row gaps")
        close(t.data, ts * T, ts * X.abs() @ A.abs().t(), k=3e-5, msg=f"gemm T tile {tile}")
        close(y.data[:, :N], Y, Yabs, BF, k=2e-3, msg=f"gemm Y tile {tile}")
    nsel = 3
    rs = inp(rnd((nsel, r), F32, 1.0, seed=6))
    for tile, rps in ((0, 5), (22, 1), (33, 5)):
        RS = d64(rs)[(torch.arange(M, device=DEV) // rps) % nsel]
        _, Yr, Yrabs = _gemm_ref(X, W, B_, A, U, s_, RS)
        y, t = out((M, N), BF), out((M, r))
        ok(lib().lora_amd_linear_gemm_fwd_rowscale(x.data_ptr(), K + 64, w.data_ptr(), K, b.data_ptr(), y.ptr, N,
                                                   down.data_ptr(), up.data_ptr(), t.ptr, M, K, N, r, _C.BF16, s_, rs.data_ptr(),
                                                   nsel, rps, tile, stream()), "linear_gemm_fwd_rowscale")
        check(y, t, what=f"gemm rowscale tile {tile}")
        close(t.data, T, X.abs() @ A.abs().t(), k=3e-5, msg="gemm rowscale T")
        close(y.data, Yr, Yrabs * RS.abs().max(), BF, k=2e-3, msg=f"gemm rowscale Y tile {tile}")
    # head-padded X and Y (q / k / v write the padded layout, the output projection reads it)
    Kh, Nh, d, D = 320, 320, 40, 64
    xh_log = rnd((M, Kh), BF, seed=7)
    xh = padded(xh_log, d, D)
    wh, bh = inp(rnd((Nh, Kh), BF, 0.05, seed=8)), inp(rnd((Nh,), BF, 0.5, seed=9))
    dh, uh = inp(rnd((r, Kh), F32, 0.2, seed=10)), inp(rnd((Nh, r), F32, 0.3, seed=11))
    Th, Yh, Yhabs = _gemm_ref(d64(xh_log), d64(wh), d64(bh), d64(dh), d64(uh), s_)
    cols = heads_cols(Nh, d, D)
    for tile in (22, 24, 21, 33):
        y, t = out((M, Nh // d * D), BF), out((M, r))
        ok(lib().lora_amd_linear_gemm_fwd(xh.data_ptr(), xh.stride(0), wh.data_ptr(), Kh, bh.data_ptr(), y.ptr,
                                          Nh // d * D, dh.data_ptr(), uh.data_ptr(), t.ptr, M, Kh, Nh, r, _C.BF16, s_,
                                          1.0, 0, tile, d, D, d, D, stream()), "linear_gemm_fwd with heads")
        check(y, t, what=f"gemm heads tile {tile}")
        pads = torch.ones(y.data.shape[1], dtype=torch.bool, device=DEV)
        pads[cols] = False
        assert bool((y.data[:, pads] == 0).all()), "head pads of Y must be written as zeros"
        close(t.data, Th, d64(xh_log).abs() @ d64(dh).abs().t(), k=3e-5, msg="gemm heads T")
        close(y.data[:, cols], Yh, Yhabs, BF, k=2e-3, msg=f"gemm heads Y tile {tile}")


@case("lora_amd_ws_pack", "lora_amd_linear_ws")
def case_linear_ws():
    """q / k / v sharing one X, their outputs as column ranges of ONE buffer (gaps between them untouched), M one past a
    row tile; the head-padded forms (built for the dropout sites): padded outputs (q / k / v; pads written as zeros) and a
    padded input (to_out)."""
    s_, M, K, N, r = 0.7, 129, 320, 320, 4
    pcols, trows = C.c_int32(0), C.c_int32(0)
    assert lib().lora_amd_ws_config(K, C.byref(pcols), C.byref(trows)) != 0 and N % pcols.value == 0
    x_log = rnd((M, K), BF, seed=1)
    d, D = 40, 64
    for x_heads, heads in ((False, False), (False, True), (True, False)):
        x = padded(x_log, d, D) if x_heads else inp(x_log, ld=K + 8)
        ow = N // d * D if heads else N
        ybuf = out((M, 3 * (ow + 8)), BF)                    # three outputs side by side, 8 gap columns behind each
        sites = (_C.WsSite * 3)()
        refs, keep = [], []
        for i in range(3):
            w = inp(rnd((N, K), BF, 0.05, seed=10 + i))
            wp = out(int(lib().lora_amd_ws_packed_elems(N, K)), BF)
            ok(lib().lora_amd_ws_pack(w.data_ptr(), K, 1, N, K, _C.BF16, wp.ptr, stream()), "ws_pack")
            b = inp(rnd((N,), BF, 0.5, seed=20 + i))
            dn, up = inp(rnd((r, K), F32, 0.2, seed=30 + i)), inp(rnd((N, r), F32, 0.3, seed=40 + i))
            t = out((M, r))
            q = sites[i]
            q.wp, q.bias, q.y, q.down, q.up, q.t_out = wp.ptr, b.data_ptr(), ybuf.ptr + 2 * i * (ow + 8), dn.data_ptr(), \
                up.data_ptr(), t.ptr
            q.ldy, q.N, q.r, q.flayout, q.scale, q.t_scale = 3 * (ow + 8), N, r, 0, s_, 1.0
            q.y_heads = d | (D << 16) if heads else 0
            p = 0.1 if heads or x_heads else 0.0
            q.dropout_p, q.seed, q.offset = p, 99 + i, 5
            refs.append((w, b, dn, up, t, wp, _mask(M, N, p, 99 + i, 5)))
        if heads or x_heads:
            ok(lib().lora_amd_linear_ws(x.data_ptr(), x.stride(0), M, K, d if x_heads else 0, D if x_heads else 0,
                                        _C.BF16, sites, 3, 0, stream()), "linear_ws with heads")
        else:
            ok(lib().lora_amd_linear_ws(x.data_ptr(), K + 8, M, K, 0, 0, _C.BF16, sites, 3, 0, stream()), "linear_ws")
        check(ybuf, *[g_ for ref in refs for g_ in (ref[4], ref[5])], what=f"linear_ws x_heads={x_heads} y_heads={heads}")
        cols = heads_cols(N, d, D) if heads else torch.arange(N, device=DEV)
        for i, (w, b, dn, up, t, _, mk) in enumerate(refs):
            yv = ybuf.data[:, i * (ow + 8):(i + 1) * (ow + 8)]
            MG.assert_untouched(yv[:, ow:], f"ws site {i} gap columns")
            if heads:
                pads = torch.ones(ow, dtype=torch.bool, device=DEV)
                pads[cols] = False
                assert bool((yv[:, :ow][:, pads] == 0).all()), "ws head pads must be written as zeros"
            T, Y, Yabs = _gemm_ref(d64(x_log), d64(w), d64(b), d64(dn), d64(up), s_, mask=mk)
            close(t.data, T, d64(x_log).abs() @ d64(dn).abs().t(), k=3e-5, msg=f"ws T site {i}")
            close(yv[:, cols], Y, Yabs, BF, k=2e-3, msg=f"ws Y site {i} heads={heads}")


# ----------------------------------------------------------------------------- twins: guarded launch == plain launch
class _Alloc:
    """Allocations of one run of a twin case: plain tensors, or guarded / poisoned ones (``guarded``)."""

    def __init__(self, guarded):
        self.guarded, self.gs = guarded, []

    def out(self, shape, dt=F32, fill=None):
        if self.guarded:
            g = MG.Guarded(shape, dt, DEV, fill="sentinel" if fill is None else fill)
            self.gs.append(g)
            return g.data
        return torch.zeros(shape, dtype=dt, device=DEV) if fill is None else fill.clone()

    def counters(self, n):
        return self.out(n, torch.int32, fill=torch.zeros(n, dtype=torch.int32, device=DEV))

    def inp(self, t):
        return MG.poisoned(t) if self.guarded else t.clone()

    def check(self, what):
        torch.cuda.synchronize()
        for i, g in enumerate(self.gs):
            g.check(f"{what} allocation {i}")


def _twin(fn, what):
    """Run ``fn(alloc)`` on plain and on guarded / poisoned allocations: the guards intact and the returned results equal
    bit for bit (an over-read of the slack around a plain allocation would meet NaN in the guarded run)."""
    plain = fn(_Alloc(False))
    a = _Alloc(True)
    guarded = fn(a)
    a.check(what)
    assert len(plain) == len(guarded)
    for i, (u, v) in enumerate(zip(plain, guarded)):
        assert torch.equal(MG._bits(u.contiguous()), MG._bits(v.contiguous())), f"{what}: result {i} differs from the plain launch"
        if u.is_floating_point():
            assert not bool(MG.is_sentinel(v).any()), f"{what}: result {i} holds the sentinel"


CONV_CASES = [(1, 8, 8, 8, 8, 3, 5, F32, 0.0), (2, 40, 24, 8, 32, 3, 16, BF, 0.25), (3, 16, 64, 8, 8, 1, 4, BF, 0.0)]


@case("lora_amd_conv_down_fwd", "lora_amd_conv_up_fwd", "lora_amd_conv_up_fwd_rowscale", "lora_amd_conv_bwd_g",
      "lora_amd_conv_bwd_x")
def case_conv_nchw():
    """The NCHW conv adapter (values: tests/test_gpu_kernels.py::test_conv_kernels_match_oracle): B = 1, the smallest maps,
    rank tiles not full, dropout; every workspace sized exactly as lora_amd_conv_plan says."""
    for B, Ci, Co, Hh, Ww, ks, r, dt, p in CONV_CASES:
        plan = _C.conv_plan(B, Ci, Co, Hh, Ww, ks, r)
        assert plan.native == 1
        HW = Hh * Ww

        def run(a):
            x, g = a.inp(rnd((B, Ci, Hh, Ww), dt, seed=1)), a.inp(rnd((B, Co, Hh, Ww), dt, seed=2))
            down, up = a.inp(rnd((r, Ci, ks, ks), F32, 0.2, seed=3)), a.inp(rnd((Co, r, 1, 1), F32, 0.3, seed=4))
            rs = a.inp(rnd((3, r), F32, seed=5))
            t_part, gt_part = a.out(max(int(plan.t_part_floats), 1)), a.out(max(int(plan.gt_part_floats), 1))
            t, gt = a.out((B, r, Hh, Ww)), a.out((B, r, Hh, Ww))
            up_part, down_part = a.out(int(plan.up_part_floats)), a.out(int(plan.down_part_floats))
            _C.conv_down_fwd(x, down, None, t_part, t, ks)
            y = a.out((B, Co, Hh, Ww), dt, fill=rnd((B, Co, Hh, Ww), dt, seed=6))
            _C.conv_up_fwd_(y, t, up, 0.7, p, 1234, 7)
            y2 = a.out((B, Co, Hh, Ww), dt, fill=rnd((B, Co, Hh, Ww), dt, seed=6))
            _C.conv_up_fwd_rowscale_(y2, t, up, 0.7, rs, p, 1234, 7)   # sample b takes row b % 3 of the table
            dx = a.out((B, Ci, Hh, Ww), dt, fill=rnd((B, Ci, Hh, Ww), dt, seed=8))
            _C.conv_bwd_g(g, t, up, None, gt_part, gt, up_part, 0.7, p, 1234, 7)
            _C.conv_bwd_x(x, dx, gt, down, down_part, ks)
            d_up, d_down = a.out((Co, r)), a.out((r, Ci * ks * ks))
            rows = _conv_rows(plan, Ci, Co, ks, r, up_part, down_part, d_up, d_down)
            _C.reduce_batched(*_C.make_reduce_table(rows, DEV))
            return [t, y, y2, gt, dx, d_up, d_down]

        _twin(run, f"conv nchw B={B} Ci={Ci} ks={ks} r={r}")


def _conv_rows(plan, Ci, Co, ks, r, up_part, down_part, d_up, d_down):
    return [(up_part, d_up, plan.ngroups_out, plan.rank_pad, Co, r, _C.FACTOR_KR, 1.0, 0.0),
            (down_part, d_down, plan.ngroups_in, plan.rank_pad, Ci * ks * ks, r, _C.FACTOR_RK, 1.0, 0.0)]


@case("lora_amd_conv3_nhwc_pack", "lora_amd_conv3_nhwc_down_fwd", "lora_amd_conv3_nhwc_bwd_dx", "lora_amd_conv3_nhwc_bwd_down")
def case_conv3_nhwc():
    """The channels-last 3x3 pieces: a partial pixel tile (W = 20), B = 1, a ksplit > 1 forward (t_part), csplit and nsplit
    partials, ranks 4 / 12 / 16; T and dDown against f64, dX against f64, partial rows >= r never read."""
    for B, Ci, Hh, Ww, r in ((1, 640, 12, 20, 16), (2, 64, 20, 20, 12), (1, 128, 9, 20, 4)):
        plan = _C.conv3_nhwc_plan(B, Ci, Hh, Ww, r)
        assert plan.native == 1
        M = B * Hh * Ww
        x = inp(rnd((B, Hh, Ww, Ci), BF, seed=1))
        down = inp(rnd((r, Ci, 3, 3), F32, 0.1, seed=2))
        gt = inp(rnd((M, r), F32, 0.5, seed=3))
        pf, pd = out(int(plan.pf_elems), BF), out(int(plan.pd_elems), BF)
        ok(lib().lora_amd_conv3_nhwc_pack(down.data_ptr(), r, Ci, _C.BF16, pf.ptr, pd.ptr, stream()), "conv3_nhwc_pack")
        t_part, t = out(max(int(plan.t_part_floats), 1)), out((M, r))
        ok(lib().lora_amd_conv3_nhwc_down_fwd(x.data_ptr(), pf.ptr, t_part.ptr if plan.t_part_floats else None, t.ptr, B, Ci,
                                              Hh, Ww, r, _C.BF16, stream()), "conv3_nhwc_down_fwd")
        dx0 = rnd((M, Ci), BF, seed=4)
        dx = MG.guarded_like(dx0)
        ok(lib().lora_amd_conv3_nhwc_bwd_dx(dx.ptr, gt.data_ptr(), pd.ptr, B, Ci, Hh, Ww, r, _C.BF16, stream()),
           "conv3_nhwc_bwd_dx")
        dnp = out(int(plan.down_part_floats))
        ok(lib().lora_amd_conv3_nhwc_bwd_down(x.data_ptr(), gt.data_ptr(), dnp.ptr, B, Ci, Hh, Ww, r, _C.BF16, stream()),
           "conv3_nhwc_bwd_down")
        check(pf, pd, t_part, t, dx, dnp, what=f"conv3_nhwc B={B} Ci={Ci} r={r}")
        MG.assert_written(pf.data, "conv3 pf")
        MG.assert_written(pd.data, "conv3 pd")
        X = d64(x).permute(0, 3, 1, 2)
        dn = d64(down) if r <= 8 else d64(down.to(BF))
        T = F.conv2d(X, dn, padding=1).permute(0, 2, 3, 1).reshape(M, r)
        close(t.data, T, F.conv2d(X.abs(), dn.abs(), padding=1).permute(0, 2, 3, 1).reshape(M, r), k=3e-5, msg="conv3 T")
        # the input-gradient and factor-gradient kernels take Gt and the factor in the activation dtype
        Gt = d64(gt.to(BF)).view(B, Hh, Ww, r).permute(0, 3, 1, 2)
        dnb = d64(down.to(BF))
        DX = F.conv_transpose2d(Gt, dnb, padding=1).permute(0, 2, 3, 1).reshape(M, Ci)
        DXabs = F.conv_transpose2d(Gt.abs(), dnb.abs(), padding=1).permute(0, 2, 3, 1).reshape(M, Ci)
        close(dx.data, d64(dx0) + DX, d64(dx0).abs() + DXabs, BF, k=3e-5, msg="conv3 dX")
        parts = d64(dnp.data).view(int(plan.nsplit), int(plan.rank_pad), Ci * 9)[:, :r].sum(0)
        # dDown[j, c, tap] = sum_p Gt[p, j] X[p + tap, c]: the weight gradient of the 3x3 convolution
        Xr = X.detach().clone().requires_grad_(False)
        want = torch.nn.grad.conv2d_weight(Xr, (r, Ci, 3, 3), Gt, padding=1).reshape(r, Ci * 9)
        wabs = torch.nn.grad.conv2d_weight(Xr.abs(), (r, Ci, 3, 3), Gt.abs(), padding=1).reshape(r, Ci * 9)
        close(parts, want, wabs, k=1e-4, msg="conv3 dDown")


# ----------------------------------------------------------------------------- the SVD distillation (cli_svd) family: twins
@case("lora_amd_rowdot_batched", "lora_amd_colreduce_batched", "lora_amd_chol_inverse_batched")
def case_svd_batched():
    """Stacks with M = 1 and K = 8 x odd, the colreduce workspace exactly batch * colreduce_workspace, l = 5 and 32."""
    for B, M, K, r in ((3, 1, 72, 5), (2, 257, 328, 16)):
        def run(a):
            x, f = a.inp(rnd((B, M, K), F32, seed=1)), a.inp(rnd((B, r, K), F32, 0.3, seed=2))
            t, d = a.out((B, M, r)), a.out((B, r, K))
            ok(lib().lora_amd_rowdot_batched(x.data_ptr(), K, M * K, f.data_ptr(), r * K, t.data_ptr(), M * r, B, M, K, r,
                                             _C.F32, _C.F32, _C.FACTOR_RK, 0.5, stream()), "rowdot_batched")
            wsb = int(lib().lora_amd_colreduce_workspace(M, K, r)) * B
            ws = a.out(max(wsb // 4, 1))
            ok(lib().lora_amd_colreduce_batched(x.data_ptr(), K, M * K, t.data_ptr(), M * r, d.data_ptr(), r * K, B, M, K, r,
                                                _C.F32, _C.FACTOR_RK, 1.0, ws.data_ptr(), wsb, stream()), "colreduce_batched")
            res = [t, d]
            for ll in (5, 32):
                z = rnd((B, 3 * ll, ll), F32, seed=ll)
                gram = a.inp(z.transpose(1, 2) @ z)
                o = a.out((B, ll, ll))
                ok(lib().lora_amd_chol_inverse_batched(gram.data_ptr(), o.data_ptr(), ll, B, 1e-4, stream()),
                   "chol_inverse_batched")
                res.append(o)
            return res

        _twin(run, f"svd batched B={B} M={M} K={K}")


@case("lora_amd_rowdot_ragged", "lora_amd_colreduce_ragged")
def case_svd_ragged():
    """Two stacks of different shapes whose outputs are adjacent slices of ONE buffer (M = 1, odd K)."""
    r = 4
    shapes = [(2, 33, 40), (1, 1, 72), (3, 257, 24)]

    def run(a):
        xs = [a.inp(rnd(sh, F32, seed=i)) for i, sh in enumerate(shapes)]
        fs = [a.inp(rnd((B, r, K), F32, 0.3, seed=10 + i)) for i, (B, M, K) in enumerate(shapes)]
        n_t = [B * M * r for B, M, K in shapes]
        n_d = [B * r * K for B, M, K in shapes]
        flat_t, flat_d = a.out(sum(n_t)), a.out(sum(n_d))
        ts = [flat_t[sum(n_t[:i]):sum(n_t[:i + 1])].view(B, M, r) for i, (B, M, K) in enumerate(shapes)]
        ds = [flat_d[sum(n_d[:i]):sum(n_d[:i + 1])].view(B, r, K) for i, (B, M, K) in enumerate(shapes)]
        parts = [a.out(max(int(lib().lora_amd_colreduce_workspace(M, K, r)) * B // 4, 1)) for B, M, K in shapes]
        prog = _C.RaggedProgram(DEV)
        h1 = prog.table(_C.RAGGED_ROWDOT, r, [(x, f, t, None) for x, f, t in zip(xs, fs, ts)])
        h2 = prog.table(_C.RAGGED_COLREDUCE, r, [(x, t, d, pt) for x, t, d, pt in zip(xs, ts, ds, parts)])
        prog.upload()
        prog.run(h1, _C.FACTOR_RK, 0.5)
        prog.run(h2, _C.FACTOR_RK, 1.0)
        return [flat_t, flat_d]

    _twin(run, "svd ragged")


@case("lora_amd_split16_ragged", "lora_amd_split16_transpose", "lora_amd_sub_ragged", "lora_amd_split16_residual")
def case_svd_split():
    """Flat arrays one chunk past a 4096-element block, 64 x 64 tiles with partial edges (72 x 136), sites adjacent in one
    plane buffer."""
    def run(a):
        srcs = [a.inp(rnd((n,), F32, seed=n)) for n in (8, 4104)]
        planes = a.out(2 * (8 + 4104), BF)
        his, los = [planes[:8], planes[8:4112]], [planes[4112:4120], planes[4120:]]
        _C.split16_ragged(srcs, his, los)
        stack = a.inp(rnd((2, 72, 136), F32, seed=3))
        h, l_, th, tl = (a.out(sh, BF) for sh in ((2, 72, 136), (2, 72, 136), (2, 136, 72), (2, 136, 72)))
        _C.split16_transpose([stack], [h], [l_], [th], [tl])
        pa = [(a.inp(rnd((n,), BF, seed=n + 1)), a.inp(rnd((n,), BF, seed=n + 2))) for n in (1, 4097)]
        flat = a.out(1 + 4097)
        _C.sub_ragged(pa, [flat[:1], flat[1:]])
        tuned = [a.inp(rnd((72, 136), BF, seed=7 + b)) for b in range(2)]
        base = [a.inp(rnd((72, 136), BF, seed=9 + b)) for b in range(2)]
        rh, rl, rth, rtl = (a.out(sh, BF) for sh in ((2, 72, 136), (2, 72, 136), (2, 136, 72), (2, 136, 72)))
        norms = _C.split16_residual([(tuned, base)], [(2, 72, 136)], [rh], [rl], [rth], [rtl])
        return [planes, h, l_, th, tl, flat, rh, rl, rth, rtl, norms]

    _twin(run, "svd split")


@case("lora_amd_rowdot16_planes", "lora_amd_rowdot16_planes_packed", "lora_amd_thin_pack")
def case_svd_planes():
    """Skinny products on (hi, lo) planes, M = 1 and one row past a slab, C = 32 (one fragment block), the packed factor
    (thin_pack) of sites adjacent in one buffer."""
    dims = [(2, 33, 64), (1, 1, 32), (1, 17, 96)]

    def run(a):
        res = []
        offs, tot = [], 0
        for B, M, Cc in dims:
            offs.append(tot)
            tot += B * Cc * 16
        flat = a.inp(rnd((tot,), F32, seed=1))
        X = [rnd((B, M, Cc), F32, seed=2 + i) for i, (B, M, Cc) in enumerate(dims)]
        hi = [a.inp(x.to(BF)) for x in X]
        lo = [a.inp((x - x.to(BF).float()).to(BF)) for x in X]
        Fs = [flat[o:o + B * Cc * 16].view(B, Cc, 16) for o, (B, M, Cc) in zip(offs, dims)]
        oa = [a.out((B, M, 16)) for B, M, Cc in dims]
        pa = _C.PlanesProgram(DEV, 16)
        ha = pa.table(list(zip(hi, lo, Fs, oa)))
        pa.upload()
        pa.run(ha)
        tab = _C.ThinTable([(o + b * Cc * 16, Cc) for o, (B, M, Cc) in zip(offs, dims) for b in range(B)], DEV)
        pk = a.out(tot * 2, BF)
        _C.thin_pack(tab, flat, pk)
        PK = [pk[2 * o: 2 * o + B * Cc * 32].view(B, Cc * 32) for o, (B, M, Cc) in zip(offs, dims)]
        for hi_only in (False, True):
            ob = [a.out((B, M, 16)) for B, M, Cc in dims]
            pb = _C.PlanesProgram(DEV, 16, packed=True)
            hb = pb.table(list(zip(hi, lo, PK, ob)))
            pb.upload()
            pb.run(hb, hi_only=hi_only)
            res += ob
        return res + oa + [pk]

    _twin(run, "svd planes")


@case("lora_amd_thin_gram", "lora_amd_thin_apply", "lora_amd_thin_rotate", "lora_amd_thin_select", "lora_amd_thin_clamp")
def case_svd_thin():
    """The fused small steps with their reductions finished by the last-arriving workgroup: sites of 1, 255, 256 and 257
    rows adjacent in one flat buffer, every counter back at zero after every launch."""
    rows = [1, 255, 256, 257]
    offs, tot = [], 0
    for n in rows:
        offs.append(tot)
        tot += -(-(n * 16) // 64) * 64

    def zero(c):
        assert int(c.abs().max()) == 0, "counters not back at zero"

    def run(a):
        flat = a.inp(rnd((tot,), F32, seed=1))
        tab = _C.ThinTable(list(zip(offs, rows)), DEV)
        tab.part, tab.counters = a.out(tab.total_blocks * 256), a.counters(len(rows))
        linv, ritz = a.out((len(rows), 16, 16)), a.out((len(rows), 2))
        _C.thin_gram(tab, flat, None, _C.thin_finish(tab, 1, 8, 1e-4, linv_out=linv, ritz_out=ritz))
        torch.cuda.synchronize()
        zero(tab.counters)
        dst, linv2 = a.out(tot, fill=torch.zeros(tot, device=DEV)), a.out((len(rows), 16, 16))
        _C.thin_apply(tab, flat, linv, dst, _C.thin_finish(tab, 1, 8, 0.0, linv_out=linv2))
        torch.cuda.synchronize()
        zero(tab.counters)
        ubt, vb, sv = a.out((len(rows), 8, 16)), a.out((len(rows), 8, 16)), a.out((len(rows), 16))
        _C.thin_gram(tab, flat, dst, _C.thin_finish(tab, 2, 8, 0.0, ubt=ubt, vb=vb, s_out=sv))
        torch.cuda.synchronize()
        zero(tab.counters)
        r = 5
        mats = a.inp(rnd((len(rows), r, 16), F32, seed=2))
        rot = a.out(tot // 16 * r, fill=torch.zeros(tot // 16 * r, device=DEV))
        sign = a.out((len(rows), 16), fill=torch.zeros(len(rows), 16, device=DEV))
        ws = (a.out(tab.total_blocks * 32), a.out(tab.total_blocks * 16, torch.int32))
        _C.thin_rotate(tab, flat, mats, r, rot, sign_ws=ws, sign_out=sign)
        torch.cuda.synchronize()
        zero(tab.counters)
        # order statistics + clamp over (u, v) pairs of every site, adjacent in two flat buffers
        nu, nv = [(1, 3), (64, 32), (1000, 9000)], r
        U = a.out(sum(x for x, _ in nu) * r, fill=rnd((sum(x for x, _ in nu) * r,), F32, 0.3, seed=3))
        V = a.inp(rnd((sum(y for _, y in nu) * r,), F32, 0.05, seed=4))
        ou, ov = [sum(x for x, _ in nu[:i]) * r for i in range(3)], [sum(y for _, y in nu[:i]) * r for i in range(3)]
        qt = _C.ThinQTable([(ou[i], nu[i][0] * r, ov[i], nu[i][1] * r) for i in range(3)], DEV)
        qt.hist, qt.counters = a.out(3 * 2048, torch.int32, fill=torch.zeros(3 * 2048, dtype=torch.int32, device=DEV)), \
            a.counters(3)
        st0 = torch.zeros(3, 8, dtype=torch.int32, device=DEV)
        st0[:, 1] = torch.tensor([(x + y) * r * 9 // 10 for x, y in nu], dtype=torch.int32)
        st0[:, 3] = -1
        state, out2 = a.out((3, 8), torch.int32, fill=st0), a.out((3, 2))
        sg = a.inp(torch.sign(rnd((3, 16), F32, seed=5)))
        for p_ in range(3):
            _C.thin_select(qt, U, V, sg, r, p_, state, out2)
            torch.cuda.synchronize()
            zero(qt.counters)
        hi = a.inp(out2[:, 0].clone())
        down = a.out(V.numel())
        _C.thin_clamp(qt, U, V, sg, hi, down, r)
        return [linv, ritz, dst, linv2, ubt, vb, sv, rot, sign, out2, U, down]

    _twin(run, "svd thin")


# ----------------------------------------------------------------------------- exemptions
# launcher -> one-line reason it has no case (none today); tests/test_capi_cpu.py::test_every_launcher_has_a_footprint_case
# fails for any launcher that is neither covered above nor listed here.
EXEMPT = {}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_footprint(name):
    torch.cuda.synchronize()
    CASES[name][1]()
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("row", range(len(REDUCE_ROWS)))
def test_a_reduce_row_one_column_too_wide_fails_the_adjacency_case(row):
    """The check itself: a table row describing C + 1 columns (its writes spill into the next slice, the gap or the guard,
    all memory the case owns) must fail."""
    with pytest.raises(AssertionError):
        case_reduce_batched(bad_row=row)


@pytest.mark.gpu
def test_counters_left_non_zero_fail_the_conv3_counter_case():
    """The check itself: counters as a launch that forgot its reset leaves them (ksplit per tile) must fail."""
    with pytest.raises(AssertionError):
        case_conv3_nhwc_fwd_fused(stale_counters=True)
