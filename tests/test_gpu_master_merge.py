"""The in-step merge from an f32 MASTER weight (csrc/merge_step.hip, ``lora_amd_mstep_site.src_f32``): W is read as f32,
W_eff = round16(W32 + alpha up down) and its transpose are written in the 16-bit output dtype — one rounding, where the
shadow-then-merge route (a 16-bit copy of W through the 16-bit-source kernel) rounds twice.

Inputs of the value tests: W ~ 0.05 N(0, 1) with a FULL f32 mantissa (not representable in 16 bits), up, down ~ 0.3 N(0, 1),
alpha = 0.7, the site list of test_gpu_parity_r4::test_merge_step_writes_w_eff_and_its_transpose_vs_oracle."""
import pytest
import torch

from lora_amd import _C
from tests import memguard as MG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
ALPHA = 0.7
# the launch takes alpha as a C float: the reference value is formed with THAT number (0.7f = 0.699999988...; against the
# double 0.7 a sum that cancels to 1e-7 would be compared with a value 1e-9 away: more than a bf16 ulp of it)
ALPHA_F32 = float(torch.tensor(ALPHA, dtype=torch.float32))
SITES = [(320, 320, 4, None, None, "bf16"), (1280, 320, 8, None, None, "bf16"), (320, 768, 16, None, None, "bf16"),
         (320, 320, 4, (40, 64), None, "bf16"), (320, 320, 4, None, (40, 64), "bf16"), (2560, 320, 4, None, None, "f16"),
         (10240, 1280, 4, None, None, "bf16"), (328, 72, 3, None, None, "bf16")]
# the share of elements that may differ from the f64 value rounded straight to 16 bits.  A condition, not a measurement: the
# f32 fma chain is off by a few 2^-24 of the terms, so only elements inside that band around a rounding tie can flip (a CPU
# restatement of the chain gives 2e-5 .. 2.2e-4 on these shapes); rounding W to 16 bits first moves 0.12 .. 0.20 of them
CAP = 1e-3


def rnd32(shape, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def ulp16(x64: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """The spacing of ``dt`` at |x| (f64 in, f64 out; exact: frexp, no logarithm)."""
    mant, emin = (7, -126) if dt == torch.bfloat16 else (10, -14)
    _, e = torch.frexp(x64)   # |x| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x64), (e - 1).clamp(min=emin) - mant)


def round16(x64: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """f64 -> ``dt`` with ONE nearest-even rounding (a cast through f32 would round twice)."""
    u = ulp16(x64, dt)
    return (torch.round(x64 / u) * u).to(dt)   # torch.round: half to even; the quotient and the product are exact


def steps_apart(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """How many 16-bit values lie between a and b (same sign: the storage bits are ordered like the magnitudes)."""
    return (a.view(torch.int16).int() - b.view(torch.int16).int()).abs()


def site_of(N, K, r, rh, ch, dt, seed=1, fill=9.0, with_t=True):
    w = rnd32((N, K), 0.05, seed)
    up, down = rnd32((N, r), 0.3, seed + 1), rnd32((r, K), 0.3, seed + 2)
    np_, kp = ((N // rh[0]) * rh[1] if rh else N), ((K // ch[0]) * ch[1] if ch else K)
    out = torch.full((np_, kp), fill, dtype=DT[dt], device=DEV)
    out_t = torch.full((kp, np_), fill, dtype=DT[dt], device=DEV) if with_t else None
    return dict(w=w, up=up, down=down, out=out, out_t=out_t, row_heads=rh, col_heads=ch, key=7)


def logical(out, N, K, rh, ch, fill=9.0):
    """The logical [N, K] part of a (head-padded) output; asserts that the pads still hold ``fill``."""
    got, kp = out, out.shape[1]
    if rh:
        assert torch.all(got.view(N // rh[0], rh[1], kp)[:, rh[0]:, :] == fill)
        got = got.view(N // rh[0], rh[1], kp)[:, :rh[0], :].reshape(N, kp)
    if ch:
        assert torch.all(got.view(N, K // ch[0], ch[1])[:, :, ch[0]:] == fill)
        got = got.view(N, K // ch[0], ch[1])[:, :, :ch[0]].reshape(N, K)
    return got


def sum64(st):
    return st["w"].double() + ALPHA_F32 * (st["up"].double() @ st["down"].double())


@pytest.mark.parametrize("N,K,r,rh,ch,dt", SITES)
def test_master_merge_rounds_once_and_the_shadow_route_does_not(N, K, r, rh, ch, dt):
    """ROUND_ONCE from the f32 master: W_eff^T is W_eff's transpose bit for bit, pads keep their fill, and against the f64
    value of W + alpha up down cast STRAIGHT to the 16-bit type at most 1e-3 of the elements differ, none by more than one
    ulp.  The same site through a 16-bit copy of W (the shadow-then-merge route, the 16-bit-source kernel) exceeds that cap
    tenfold: the test can tell the two apart.
    One ulp AT THE ELEMENT is more than an f32 chain alone gives where W and alpha up down cancel (a master is not on the
    16-bit grid: on these sites 1 element of 409 600 and 30 of 13 107 200 cancel below 4e-6 of the terms, and an f32 sum is
    then several 16-bit ulps of so small a result off): the kernel forms such elements again in f64."""
    st = site_of(N, K, r, rh, ch, dt)
    plan = _C.MergeStepPlan([st])
    assert plan.src_f32 and plan.w_dtype == DT[dt]
    assert plan.bytes_algorithmic == N * K * (4 + 2 + 2) + (N + K) * r * 4
    plan.launch(ALPHA, _C.ROUND_ONCE)
    assert torch.equal(st["out_t"], st["out"].t())
    got = logical(st["out"], N, K, rh, ch)
    assert bool(torch.isfinite(got).all())
    want = round16(sum64(st), DT[dt])
    share = float((got != want).double().mean())
    apart = int(steps_apart(got, want).max())
    sh = dict(st, w=st["w"].to(DT[dt]), out=torch.full_like(st["out"], 9.0), out_t=torch.full_like(st["out_t"], 9.0))
    plan16 = _C.MergeStepPlan([sh])
    assert not plan16.src_f32 and plan16.bytes_algorithmic == N * K * 6 + (N + K) * r * 4
    plan16.launch(ALPHA, _C.ROUND_ONCE)
    share16 = float((logical(sh["out"], N, K, rh, ch) != want).double().mean())
    s64 = sum64(st)
    absref = st["w"].double().abs() + ALPHA_F32 * (st["up"].double().abs() @ st["down"].double().abs())
    far = steps_apart(got, want) > 1
    print(f"\n[master merge {N}x{K} r{r} {dt} rows{rh} cols{ch}] differing share: master {share:.3e}, "
          f"shadow-then-merge {share16:.3e}; worst distance {apart} ulp; {int(far.sum())} of {N * K} elements further than one, "
          f"their |sum| / terms at most {float((s64.abs() / absref)[far].max()) if bool(far.any()) else 0.0:.2e}")
    assert share <= CAP, share
    assert share16 > 10 * CAP, share16
    # the f32 value before the rounding: each of the r + 1 fmas is off by at most 2^-24 of the terms' magnitude (plus half a
    # 16-bit ulp of the result for the rounding itself)
    assert bool(((got.double() - s64).abs() <= (r + 2) * 2.0 ** -24 * absref + 0.5 * ulp16(s64, DT[dt])).all())
    assert apart <= 1, apart


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_master_merge_dither_picks_a_neighbour_is_fixed_and_unbiased(dt):
    """ROUND_DITHER from the f32 master: every element is one of the two 16-bit neighbours of the f32 sum, the same inputs
    give the same bits, W_eff^T is the exact transpose, and over 819 200 elements the mean of (W_eff - (W32 + alpha delta))
    in ulps is within 0.01 of zero (the dither's standard error there is 5e-4)."""
    N, K, r = 1280, 640, 4
    st = site_of(N, K, r, None, None, dt)
    _C.MergeStepPlan([st]).launch(ALPHA, _C.ROUND_DITHER)
    got = st["out"].clone()
    assert torch.equal(st["out_t"], got.t())
    s = sum64(st)
    u = ulp16(s, DT[dt])
    err = (got.double() - s) / u
    # a neighbour of the f32 sum, which itself is within a few 2^-24 of the f64 sum (2^-14 of a 16-bit ulp at most)
    assert float(err.abs().max()) <= 1.0 + 2.0 ** -10, float(err.abs().max())
    assert N * K >= 600_000
    print(f"\n[master merge dither {dt}] mean error {float(err.mean()):+.5f} ulp over {N * K} elements")
    assert abs(float(err.mean())) <= 0.01, float(err.mean())
    again = site_of(N, K, r, None, None, dt)
    _C.MergeStepPlan([again]).launch(ALPHA, _C.ROUND_DITHER)
    assert torch.equal(again["out"], got) and torch.equal(again["out_t"], got.t())
    once = site_of(N, K, r, None, None, dt)
    _C.MergeStepPlan([once]).launch(ALPHA, _C.ROUND_ONCE)
    assert not torch.equal(once["out"], got)


def test_master_merge_tile_geometries_agree():
    """All four tile geometries of the tuning hook write the same bits from an f32 source, nearest-even and dithered, on
    dense, ragged and head-padded sites."""
    cases = [(320, 320, 4, None, None), (328, 72, 3, None, None), (1280, 320, 8, (40, 64), None), (640, 640, 4, None, (80, 128)),
             (2560, 320, 16, None, None)]
    for N, K, r, rh, ch in cases:
        res = {}
        for tl in range(4):
            for rounding in (_C.ROUND_ONCE, _C.ROUND_DITHER):
                st = site_of(N, K, r, rh, ch, "bf16")
                _C.merge_step_set_tuning(tl, -1)
                try:
                    plan = _C.MergeStepPlan([st])
                finally:
                    _C.merge_step_set_tuning(2, -1)
                assert plan.plan_value >> 48 == 1 and (plan.plan_value >> 40) & 0xFF == tl
                plan.launch(ALPHA, rounding)
                assert torch.equal(st["out_t"], st["out"].t())
                res[(tl, rounding)] = st["out"]
        for rounding in (_C.ROUND_ONCE, _C.ROUND_DITHER):
            for tl in (1, 2, 3):
                assert torch.equal(res[(0, rounding)], res[(tl, rounding)]), (N, K, r, rh, ch, rounding, tl)
        assert not torch.equal(res[(0, _C.ROUND_ONCE)], res[(0, _C.ROUND_DITHER)])


def test_master_merge_sites_share_one_buffer():
    """q / k / v as row ranges of ONE scratch weight and column ranges of one transposed buffer, each read from its own f32
    master: every range equals the site merged alone."""
    K, r, lay = 320, 4, (40, 64)
    ws = [rnd32((320, K), 0.05, 10 + i) for i in range(3)]
    ups = [rnd32((320, r), 0.3, 20 + i) for i in range(3)]
    downs = [rnd32((r, K), 0.3, 30 + i) for i in range(3)]
    for rounding in (_C.ROUND_ONCE, _C.ROUND_DITHER):
        cat = torch.zeros(3 * 512, K, dtype=torch.bfloat16, device=DEV)
        cat_t = torch.zeros(K, 3 * 512, dtype=torch.bfloat16, device=DEV)
        sites = [dict(w=w, up=u, down=d, out=cat[i * 512:(i + 1) * 512], out_t=cat_t[:, i * 512:(i + 1) * 512],
                      row_heads=lay, col_heads=None, key=i) for i, (w, u, d) in enumerate(zip(ws, ups, downs))]
        _C.MergeStepPlan(sites).launch(ALPHA, rounding)
        assert torch.equal(cat_t, cat.t())
        for i, (w, u, d) in enumerate(zip(ws, ups, downs)):
            one = torch.zeros(512, K, dtype=torch.bfloat16, device=DEV)
            _C.MergeStepPlan([dict(w=w, up=u, down=d, out=one, out_t=None, row_heads=lay, col_heads=None, key=i)]
                             ).launch(ALPHA, rounding)
            assert torch.equal(cat[i * 512:(i + 1) * 512], one)
            assert float(one.abs().max()) > 0


def test_master_merge_plan_refuses_other_source_types():
    w = rnd32((320, 320), 0.05, 1)
    up, down = rnd32((320, 4), 0.3, 2), rnd32((4, 320), 0.3, 3)
    bf = lambda: torch.zeros(320, 320, dtype=torch.bfloat16, device=DEV)  # noqa: E731
    with pytest.raises(TypeError):   # f16 source, bf16 output
        _C.MergeStepPlan([dict(w=w.half(), up=up, down=down, out=bf())])
    with pytest.raises(TypeError):   # one f32 and one bf16 source in one plan
        _C.MergeStepPlan([dict(w=w, up=up, down=down, out=bf()), dict(w=w.bfloat16(), up=up, down=down, out=bf())])
    with pytest.raises((ValueError, RuntimeError)):   # f32 outputs stay on lora_amd_merge_batched
        _C.MergeStepPlan([dict(w=w, up=up, down=down, out=torch.zeros(320, 320, device=DEV))])


def test_master_merge_footprint_with_guards_and_poisoned_sources():
    """Guarded outputs (sentinel NaN in the data: pads and gaps must keep it), f32 sources and factors in poisoned
    allocations: three head-padded sites in one wider buffer with their transposes, a site with head-padded columns, a dense
    site one chunk past a tile edge in both directions (N = 136, K = 72: the last column tile holds one 32-byte chunk of nine).
    Guards intact, no NaN in the written set, pads and gaps untouched, both roundings."""
    BF = torch.bfloat16
    N, K, r, d, D = 320, 320, 4, 40, 64
    Np = N // d * D

    def heads(n, dd, DD):
        i = torch.arange(n, device=DEV)
        return (i // dd) * DD + i % dd

    for rounding in (_C.ROUND_ONCE, _C.ROUND_DITHER):
        qkv, qkv_t = MG.Guarded((3 * Np, K + 8), BF, DEV), MG.Guarded((K, 3 * Np + 16), BF, DEV)
        w_o, dense = MG.Guarded((N, K // d * D), BF, DEV), MG.Guarded((136, 72), BF, DEV)
        dense_t = MG.Guarded((72, 136), BF, DEV, align=16)
        sites, refs = [], []
        for i in range(3):
            w = MG.poisoned(rnd32((N, K), 0.05, i))
            up, dn = MG.poisoned(rnd32((N, r), 0.3, 10 + i)), MG.poisoned(rnd32((r, K), 0.3, 20 + i))
            o, ot = qkv.data[i * Np:(i + 1) * Np, :K], qkv_t.data[:, i * Np:(i + 1) * Np]
            sites.append(dict(w=w, up=up, down=dn, out=o, out_t=ot, row_heads=(d, D), key=i + 1))
            refs.append((w, up, dn, o, ot, (d, D), None))
        w = MG.poisoned(rnd32((N, K), 0.05, 5))
        up, dn = MG.poisoned(rnd32((N, r), 0.3, 15)), MG.poisoned(rnd32((r, K), 0.3, 25))
        sites.append(dict(w=w, up=up, down=dn, out=w_o.data, col_heads=(d, D), key=7))
        refs.append((w, up, dn, w_o.data, None, None, (d, D)))
        w = MG.poisoned(rnd32((136, 72), 0.05, 6), align=16)
        up, dn = MG.poisoned(rnd32((136, 16), 0.3, 16)), MG.poisoned(rnd32((16, 72), 0.3, 26))
        sites.append(dict(w=w, up=up, down=dn, out=dense.data, out_t=dense_t.data, key=9))
        refs.append((w, up, dn, dense.data, dense_t.data, None, None))
        plan = _C.MergeStepPlan(sites)
        assert plan.src_f32
        plan.launch(ALPHA, rounding)
        torch.cuda.synchronize()
        for i, g in enumerate((qkv, qkv_t, w_o, dense, dense_t)):
            g.check(f"master merge_step operand {i}")
        MG.assert_untouched(qkv.data[:, K:], "qkv gap columns")
        MG.assert_untouched(qkv_t.data[:, 3 * Np:], "qkv_t gap columns")
        for w, up, dn, o, ot, rh, ch in refs:
            Nn, Kk = w.shape
            rows = heads(Nn, *rh) if rh else torch.arange(Nn, device=DEV)
            cols = heads(Kk, *ch) if ch else torch.arange(Kk, device=DEV)
            got = o[rows][:, cols]
            assert bool(torch.isfinite(got).all()), "a NaN reached W_eff"
            want = w.double() + ALPHA_F32 * (up.double() @ dn.double())
            # half an ulp (dithered: one) for the rounding + the f32 chain's own error: r + 1 fmas, each off by at most
            # 2^-24 of the terms' magnitude
            absref = w.double().abs() + ALPHA_F32 * (up.double().abs() @ dn.double().abs())
            err = ((got.double() - want).abs() - (up.shape[1] + 2) * 2.0 ** -24 * absref) / ulp16(want, BF)
            assert float(err.max()) <= (0.5 if rounding == _C.ROUND_ONCE else 1.0)
            keep = torch.ones(o.shape, dtype=torch.bool, device=DEV)
            keep[rows[:, None], cols[None, :]] = False
            MG.assert_untouched(o[keep], "master merge_step pads")
            if ot is not None:
                assert torch.equal(ot[cols][:, rows], got.t()), "W_eff^T differs from W_eff"
                keep_t = torch.ones(ot.shape, dtype=torch.bool, device=DEV)
                keep_t[cols[:, None], rows[None, :]] = False
                MG.assert_untouched(ot[keep_t], "master merge_step transposed pads")
