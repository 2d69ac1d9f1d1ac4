"""The optimiser step (csrc/optim.hip) at full size, under capture and in mixed modes, against f64.

Every reference here is a plain f64 restatement of ``torch.optim.AdamW``, ``clip_grad_norm_`` and ``GradScaler``; none
of them touches ``optim.hip`` or ``FlatLoraState``'s CPU path.  The kernels take their hyper-parameters (lr, weight
decay, betas, eps, max_norm, grad_scale) as f32, so the references use the f32-rounded values as *inputs*: 1 - f32(0.999)
differs from 0.001 by 1.3e-5 relative, which is a property of the call, not an error of the kernel.  ``1 - beta`` is exact
in f32 for 0.5 <= beta <= 1 (Sterbenz), so the kernel and the reference then agree on every constant.

u = 2^-24 is the unit roundoff of f32 (one rounding: relative error <= u).  Tolerances are derived from the kernels'
operation chains (stated where they are used) or are numbers the suite already uses for the same kernel; none of them
was fitted to what the GPU returns.
"""
import functools
import math
import random

import numpy as np
import pytest
import torch

from lora_amd import _C
from lora_amd import trainer as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24

# launch geometry of csrc/optim.hip (kOptThreads, kSumsqMaxBlocks, the 2048-block cap of clip_adamw)
THREADS, SUMSQ_MAX_BLOCKS, ADAMW_MAX_BLOCKS = 256, 1024, 2048
SUMSQ_TRIP = SUMSQ_MAX_BLOCKS * THREADS * 4      # 1 048 576 elements per grid trip of sumsq_stage1
ADAMW_TRIP = ADAMW_MAX_BLOCKS * THREADS          # 524 288 elements per grid trip of clip_adamw_kernel
N_BIG = 2 * SUMSQ_TRIP + 3 * 1024 + 3            # 2 100 227: some threads make 3 trips, others 2; 3-element tail
B1, B2, EPS = 0.9, 0.999, 1e-8
SENTINEL = 0.25


def f32(x):
    """The f64 value of x rounded to f32: what a kernel receives for a python float."""
    return np.float64(np.float32(x))


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)     # a copy: the cached arrays are read-only


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view(np.int32)


# ----------------------------------------------------------------------------------------------------- sumsq (§1)
def sumsq_blocks(n):
    return min(max((n // 4 + THREADS - 1) // THREADS, 1), SUMSQ_MAX_BLOCKS)


def sumsq_roundings(n):
    """L: the roundings on the longest path from an element to out[0] (every term is >= 0, so the relative error of the
    sum is at most (L + 2) u; the + 2 covers the second-order terms and the final conversion)."""
    nblk = sumsq_blocks(n)
    n4 = n // 4
    trips = -(-n4 // (nblk * THREADS))            # grid-stride trips of the busiest thread of stage 1
    tail_trips = -(-(n - 4 * n4) // THREADS)      # block 0 only: at most 3 elements, one per thread
    L = 4 * trips + tail_trips                    # one fmaf per element: 4 per float4 trip, 1 per tail trip
    L += 6 + 4                                    # block_sum of stage 1: 6 xor-shuffle adds per wave, 4 waves folded
    L += -(-nblk // THREADS) + 6 + 4              # stage 2: one thread adds ceil(nblk/256) partials, then block_sum
    return L


def sumsq_tol(n):
    return (sumsq_roundings(n) + 2) * U


def sentinel_indices(n):
    """Where a dropped element must show: the tail, the last full float4, the first element of every later grid trip."""
    n4 = n // 4
    idx = set(range(4 * n4, n))
    if n4:
        idx.update(range(4 * (n4 - 1), 4 * n4))
    trip = sumsq_blocks(n) * THREADS * 4
    idx.update(range(trip, 4 * n4, trip))
    return sorted(idx)


@functools.lru_cache(maxsize=None)
def grad_data(n, seed=0):
    """N(0, 1e-2) noise with a 0.25 sentinel on every index of ``sentinel_indices``; read-only."""
    x = (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 1e-2).numpy()
    x[sentinel_indices(n)] = SENTINEL
    x.setflags(write=False)
    return x


SUMSQ_NS = [1, 3, 4, 5, 1023, 1027, 262147, N_BIG]


def test_sumsq_tolerance_and_sentinel_plan():
    """The derivation above gives L = 37 and 2.32e-6 at n_big; the sentinels sit on the tail, the last float4 and the
    first element of each later grid trip."""
    assert sumsq_roundings(N_BIG) == 4 * 3 + 1 + 10 + 4 + 10
    assert 2.2e-6 < sumsq_tol(N_BIG) < 2.5e-6
    s = sentinel_indices(N_BIG)
    assert {SUMSQ_TRIP, 2 * SUMSQ_TRIP, N_BIG - 1, N_BIG - 2, N_BIG - 3, N_BIG - 4, N_BIG - 7} <= set(s)
    assert sentinel_indices(3) == [0, 1, 2] and sentinel_indices(5) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("n", SUMSQ_NS)
def test_sumsq_matches_f64_across_loop_regimes(n):
    x = grad_data(n)
    x64 = x.astype(np.float64)
    want = float(np.sum(x64 * x64))
    tol = sumsq_tol(n)
    # the data must make a dropped element visible: losing any one sentinel moves the sum by >= 10 x the tolerance
    for i in sentinel_indices(n):
        assert want - (want - x64[i] ** 2) >= 10 * tol * want, (n, i)
    g = dev(x)
    ws = torch.full((SUMSQ_MAX_BLOCKS,), float("nan"), device=DEV)
    out = torch.full((1,), float("nan"), device=DEV)
    _C.sumsq(g, out, ws)                      # every partial that stage 2 reads must have been written by stage 1
    got = float(out.item())
    print(f"sumsq n={n}: L={sumsq_roundings(n)} tol={tol:.3e} rel err={abs(got - want) / want:.3e}")
    assert math.isfinite(got)
    assert abs(got - want) <= tol * want, (n, got, want, abs(got - want) / want, tol)
    first = bits(out).copy()
    ws.fill_(float("nan")), out.fill_(float("nan"))
    _C.sumsq(g, out, ws)
    assert np.array_equal(bits(out), first)   # deterministic: two-stage, no atomics
    # a 16-byte aligned view at an offset
    buf = torch.zeros(n + 4, device=DEV)
    buf[:4] = 1e3                             # would be seen if the view's offset were dropped
    buf[4:].copy_(g)
    out.fill_(float("nan"))
    _C.sumsq(buf[4:], out, ws)
    assert np.array_equal(bits(out), first)
    with pytest.raises(ValueError):           # the alignment check of the wrapper; nothing is launched
        _C.sumsq(buf[1:], out, ws)
    rc = _C.require().lora_amd_sumsq(buf[1:].data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel() * 4, None)
    assert rc == -1                           # ... and the launcher's own (LORA_AMD_EINVAL)


# ------------------------------------------------------------------------------------------------ clip_adamw (§2)
def ref_coef(sumsq64, grad_scale, max_norm):
    """clip_grad_norm_ of grad_scale * g, folded with grad_scale: what multiplies the stored gradient."""
    gs = f32(grad_scale)
    if max_norm > 0:
        total = math.sqrt(sumsq64) * abs(gs)
        return gs * min(1.0, f32(max_norm) / (total + f32(1e-6)))
    return gs


def ref_adamw(p, g, m, v, groups, step, coef):
    """torch.optim.AdamW (decoupled decay, then moments, then the bias-corrected update) in f64 over the group ranges;
    a later group wins where two overlap; elements of no group are returned unchanged.  Returns p', m', v' and the
    quantities the tolerances are built from."""
    n = p.size
    lr, wd, own = np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool)
    for b, e, l, w in groups:
        lr[b:e], wd[b:e], own[b:e] = f32(l), f32(w), True
    b1, b2, eps = f32(B1), f32(B2), f32(EPS)
    grad = g * coef
    m2 = m + (grad - m) * (1 - b1)                       # exp_avg.lerp_(grad, 1 - beta1)
    v2 = v * b2 + (1 - b2) * grad * grad                 # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = np.sqrt(v2) / math.sqrt(bc2) + eps
    upd = (lr / bc1) * (m2 / denom)
    p2 = p * (1 - lr * wd) - upd                         # param.mul_(1 - lr wd); param.addcdiv_(m, denom, -lr / bc1)
    aux = {"own": own, "upd": upd, "gain": (lr / bc1) / denom, "grad": grad}
    return np.where(own, p2, p), np.where(own, m2, m), np.where(own, v2, v), aux


def adamw_tolerances(p, g_eff, m, v2, aux):
    """u = 2^-24; roundings counted on the kernel's chain, the constants leave a margin over the count:
    m' = m + (grad - m)(1 - b1): subtraction, product, sum = 3 roundings, each of a quantity <= |m| + |grad|  -> 4u
    v' = fma((1 - b2) grad, grad, v b2): v b2, (1 - b2) grad, the fma = 3 roundings of non-negative terms      -> 4u v'
    p' : 1 - lr wd (2), p * that (1), the final subtraction (1), each <= u (|p| + |U|)                        -> 4u |p|
         U = (lr / bc1) * (m' / denom): bc1 -> f32, lr / bc1, sqrt(v') (half of v's 3, + 1), bc2 -> f32, the division,
         + eps, m' / denom, the product: about 9 roundings, plus the share of the last subtraction             -> 16u |U|
         and the error of m' carried through (lr / bc1) / denom."""
    tol_m = 4 * U * (np.abs(m) + np.abs(g_eff))
    tol_v = 4 * U * v2
    tol_p = 4 * U * np.abs(p) + aux["gain"] * tol_m + 16 * U * np.abs(aux["upd"])
    return tol_p, tol_m, tol_v


def default_groups(n):
    cut = (2 * n // 3) | 1                     # odd: no block or float4 boundary
    return [(0, cut, 1e-2, 1e-2), (cut, n, 5e-3, 1e-2)]


@functools.lru_cache(maxsize=None)
def state_data(n):
    """p ~ N(0, 0.1), m ~ N(0, 1e-2), v = N(0, 1e-2)^2: a state some way into training; read-only."""
    gen = torch.Generator().manual_seed(100 + n % 97)
    p = (torch.randn(n, generator=gen) * 0.1).numpy()
    m = (torch.randn(n, generator=gen) * 1e-2).numpy()
    v = (torch.randn(n, generator=gen) * 1e-2).numpy() ** 2
    for a in (p, m, v):
        a.setflags(write=False)
    return p, m, v


def run_adamw(p, g, m, v, groups, step, grad_scale, max_norm, zero_grad=True, scaler=None, need_sumsq=None):
    """One launch of clip_adamw on fresh device copies; returns the device tensors p, g, m, v and the sumsq tensor."""
    tp, tg, tm, tv = dev(p), dev(g), dev(m), dev(v)
    gd = _C.make_adamw_groups(groups, DEV)
    ss = None
    if max_norm > 0 or scaler is not None or need_sumsq:
        ss = torch.zeros(1, device=DEV)
        _C.sumsq(tg, ss)
    _C.clip_adamw(tp, tg, tm, tv, gd, len(groups), ss, grad_scale, max_norm, B1, B2, EPS, step, zero_grad, scaler=scaler)
    return tp, tg, tm, tv, ss


def assert_within(got, want, tol, what):
    err = np.abs(got.astype(np.float64) - want)
    bad = err > tol
    if bad.any():
        i = int(np.argmax(err - tol))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outside tolerance; worst at {i}: got {got[i]!r} "
                             f"want {want[i]!r} err {err[i]:.3e} tol {tol[i]:.3e}")
    return float(np.max(err / np.maximum(tol, 1e-300)))


@pytest.mark.parametrize("n", [1027, N_BIG])
@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_clip_adamw_elementwise_without_clipping(n, grad_scale, step):
    """§2(a): clipping off or inactive -> coef == grad_scale exactly (a power of two, so grad_scale * g is exact)."""
    p, m, v = state_data(n)
    g = grad_data(n)
    groups = default_groups(n)
    p2, m2, v2, aux = ref_adamw(*(a.astype(np.float64) for a in (p, g, m, v)), groups, step, f32(grad_scale))
    tol_p, tol_m, tol_v = adamw_tolerances(p.astype(np.float64), aux["grad"], m.astype(np.float64), v2, aux)
    tp, tg, tm, tv, _ = run_adamw(p, g, m, v, groups, step, grad_scale, 0.0, zero_grad=False)
    worst = [assert_within(host(t), w, tol, name) for t, w, tol, name in
             ((tm, m2, tol_m, "exp_avg"), (tv, v2, tol_v, "exp_avg_sq"), (tp, p2, tol_p, "param"))]
    print(f"clip_adamw n={n} gs={grad_scale} step={step}: worst err / tol  m {worst[0]:.3f}  v {worst[1]:.3f}  p {worst[2]:.3f}")
    # every owned element moved -- but for the handful whose f64 move is itself within the tolerance at p (the decay
    # and the update nearly cancel): there p' == p is a correct result
    same = host(tp) == p
    assert same.sum() <= 8 and (np.abs(p2 - p)[same] <= tol_p[same]).all(), int(same.sum())
    assert np.array_equal(bits(tg), g.view(np.int32))     # zero_grad = 0 leaves g alone
    # a norm below max_norm: the clamp gives exactly 1, the same bits as no clipping at all
    norm = math.sqrt(float(np.sum(g.astype(np.float64) ** 2))) * grad_scale
    assert norm < 64.0
    cp, cg, cm, cv, _ = run_adamw(p, g, m, v, groups, step, grad_scale, 64.0, zero_grad=False)
    for a, b in ((cp, tp), (cm, tm), (cv, tv), (cg, tg)):
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("n", [1027, N_BIG])
@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
def test_clip_coefficient_is_the_norm_of_the_scaled_gradient(n, grad_scale):
    """§2(b): fresh state, step 1, clipping active: m' = g * coef * (1 - beta1) with no cancellation.  Chain: sumsq
    ((L + 2) u, halved by the square root), sqrtf, + 1e-6, the division, coef *= c, g * coef, * (1 - beta1): 6 more
    roundings of u / 2 each -> ((L + 2) / 2 + 3) u, asserted at ((L + 2) / 2 + 8) u."""
    g = grad_data(n)
    g64 = g.astype(np.float64)
    max_norm = 2.0 ** -6
    ss64 = float(np.sum(g64 * g64))
    assert math.sqrt(ss64) * grad_scale > 2 * max_norm    # clipping is active for both scales
    coef = ref_coef(ss64, grad_scale, max_norm)
    want = g64 * coef * (1 - f32(B1))
    z = np.zeros(n, dtype=np.float32)
    p = state_data(n)[0]
    tp, tg, tm, tv, ss = run_adamw(p, g, z, z, default_groups(n), 1, grad_scale, max_norm)
    rel = ((sumsq_roundings(n) + 2) / 2 + 8) * U
    err = np.abs(host(tm).astype(np.float64) - want)
    print(f"clip coef n={n} gs={grad_scale}: rel tol {rel:.3e} worst rel err {np.max(err / np.abs(want)):.3e}")
    assert (err <= rel * np.abs(want)).all(), (float(np.max(err / np.abs(want))), rel)
    assert float(tg.abs().sum()) == 0.0                   # zero_grad fused


def test_three_clipped_steps_follow_the_f64_trajectory():
    """§2(c): 3 clipped steps at n_big, lr 1e-2 / 5e-3; rtol 3e-6 / atol 3e-7 on p are the numbers
    test_sumsq_and_clip_adamw_match_torch_vectors uses for the same kernel over the same 3 steps."""
    n = N_BIG
    groups = default_groups(n)
    p0 = state_data(n)[0]
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    tp, tm, tv = dev(p0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    gd = _C.make_adamw_groups(groups, DEV)
    ss = torch.zeros(1, device=DEV)
    for step in (1, 2, 3):
        g = grad_data(n, seed=step)
        g64 = g.astype(np.float64)
        coef = ref_coef(float(np.sum(g64 * g64)), 1.0, 1.0)
        assert coef < 0.5                                  # the clip is active
        p, m, v, _ = ref_adamw(p, g64, m, v, groups, step, coef)
        tg = dev(g)
        _C.sumsq(tg, ss)
        _C.clip_adamw(tp, tg, tm, tv, gd, 2, ss, 1.0, 1.0, B1, B2, EPS, step, True)
        np.testing.assert_allclose(host(tp), p, rtol=3e-6, atol=3e-7, err_msg=f"step {step}")
        assert float(tg.abs().sum()) == 0.0


def sixteen_groups(n):
    """16 groups with their own lr / weight decay: an empty one, lr = 0, weight_decay = 0, a gap, boundaries on both
    sides of (and straddling) 524 288 where the second grid trip of clip_adamw begins, and an unowned tail."""
    t = ADAMW_TRIP
    edges = [0, 1000, 1000, 5003, 300001, t - 1, t + 1, None, t + 12, 600000, 700001, 3 * t - 7, 3 * t + 9, 1800000,
             1900003, 2000001, 2050000, 2075001, n - 5]
    groups, k = [], 0
    for a, b in zip(edges[:-1], edges[1:]):
        if a is None or b is None:      # the gap [t + 1, t + 12)
            continue
        groups.append([a, b, 1e-2 / (k + 1), 1e-2 * (1 + k % 3)])
        k += 1
    assert len(groups) == 16 and groups[1][0] == groups[1][1]
    groups[3][2] = 0.0                  # lr = 0 over [5003, 300001)
    groups[4][3] = 0.0                  # weight_decay = 0 over [300001, t - 1)
    return [tuple(r) for r in groups]


def test_sixteen_groups_gap_empty_group_and_zero_lr():
    """§2(d).  With lr = 0 torch's decay factor 1 - lr * weight_decay is 1: p keeps its bits, m and v still update."""
    n = N_BIG
    groups = sixteen_groups(n)
    p, m, v = state_data(n)
    g = grad_data(n)
    p2, m2, v2, aux = ref_adamw(*(a.astype(np.float64) for a in (p, g, m, v)), groups, 7, 1.0)
    own = aux["own"]
    assert not own[ADAMW_TRIP + 1:ADAMW_TRIP + 12].any() and not own[n - 5:].any() and own.sum() == n - 16
    tol_p, tol_m, tol_v = adamw_tolerances(p.astype(np.float64), aux["grad"], m.astype(np.float64), v2, aux)
    tp, tg, tm, tv, _ = run_adamw(p, g, m, v, groups, 7, 1.0, 0.0, zero_grad=True)
    for t, w, tol, name in ((tm, m2, tol_m, "exp_avg"), (tv, v2, tol_v, "exp_avg_sq"), (tp, p2, tol_p, "param")):
        assert_within(host(t), w, np.where(own, tol, 0.0), name)
    # unowned elements keep their bits everywhere, the gradient included although zero_grad is on
    for t, a in ((tp, p), (tg, g), (tm, m), (tv, v)):
        assert np.array_equal(bits(t)[~own], a.view(np.int32)[~own])
    assert float(tg[torch.from_numpy(own).to(DEV)].abs().sum()) == 0.0
    a, b = groups[3][:2]
    assert np.array_equal(bits(tp)[a:b], p.view(np.int32)[a:b])                      # lr = 0: p untouched ...
    assert (host(tm)[a:b] != m[a:b]).mean() > 0.999 and (host(tv)[a:b] != v[a:b]).mean() > 0.999   # the moments move
    a, b = groups[4][:2]
    assert (host(tp)[a:b] != p[a:b]).mean() > 0.999                                  # weight_decay = 0 still steps
    gd = _C.make_adamw_groups(list(groups) + [(0, 1, 1e-3, 0.0)], DEV)
    with pytest.raises((ValueError, RuntimeError), match="n_groups=17"):   # the launcher refuses; nothing is launched
        _C.clip_adamw(tp, tg, tm, tv, gd, 17, None, 1.0, 0.0, B1, B2, EPS, 1, True)


@pytest.mark.parametrize("n", [1027, N_BIG])
@pytest.mark.parametrize("k", [1, 7, 1000])
def test_device_step_gives_the_bits_of_the_host_step(n, k):
    """§2(e): lora_amd_clip_adamw with step_dev[0] == k is lora_amd_clip_adamw with step = k and no step_dev."""
    p, m, v = state_data(n)
    g = grad_data(n)
    groups = default_groups(n)
    a = run_adamw(p, g, m, v, groups, k, 0.25, 2.0 ** -6)
    b = run_adamw(p, g, m, v, groups, torch.tensor([k], dtype=torch.int64, device=DEV), 0.25, 2.0 ** -6)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(bits(x), bits(y))
    assert not np.array_equal(bits(a[0]), p.view(np.int32))


@pytest.mark.parametrize("n", [1027, N_BIG])
@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("max_norm", [0.0, 2.0 ** -6])
def test_scaler_operand_is_exact_for_power_of_two_scales(n, grad_scale, max_norm):
    """§2(f): scaler = [s, ., 1/s, 1], s = 1024, gradient pre-multiplied by s.  Every scaling is by a power of two: the
    sum of squares is s^2 times the unscaled one bit for bit, sqrtf gives s times the norm, grad_scale / s and the
    products are exact -> p, m, v carry the bits of the unscaled run."""
    s = 1024.0
    p, m, v = state_data(n)
    g = grad_data(n)
    groups = default_groups(n)
    step = torch.tensor([3], dtype=torch.int64, device=DEV)
    plain = run_adamw(p, g, m, v, groups, step, grad_scale, max_norm, need_sumsq=True)
    scaler = torch.tensor([s, 0.0, 1.0 / s, 1.0], device=DEV)
    scaled = run_adamw(p, g * np.float32(s), m, v, groups, step, grad_scale, max_norm, scaler=scaler)
    assert float(scaled[4].item()) == s * s * float(plain[4].item())
    for name, x, y in zip(("p", "g", "m", "v"), plain[:4], scaled[:4]):
        assert np.array_equal(bits(x), bits(y)), name
    assert not np.array_equal(bits(plain[0]), p.view(np.int32))
    # flag 0: nothing but the (owned) gradient is written
    skip = torch.tensor([s, 0.0, 1.0 / s, 0.0], device=DEV)
    sk = run_adamw(p, g * np.float32(s), m, v, groups, step, grad_scale, max_norm, scaler=skip)
    for x, a in zip((sk[0], sk[2], sk[3]), (p, m, v)):
        assert np.array_equal(bits(x), a.view(np.int32))
    assert float(sk[1].abs().sum()) == 0.0


# --------------------------------------------------------------------------------------- loss_scale_update (§3)
def scaler_model(state, finite, growth, backoff, interval):
    """torch.cuda.amp.GradScaler: state = [scale, finite steps in a row, 1 / scale of this step, finite flag] (np.float32);
    returns whether the step is applied."""
    scale = state[0]
    state[2], state[3] = np.float32(1.0) / scale, np.float32(1.0 if finite else 0.0)
    if not finite:
        state[0], state[1] = max(scale * np.float32(backoff), np.float32(1.0)), np.float32(0.0)
        return False
    state[1] += np.float32(1.0)
    if state[1] >= interval:
        state[0], state[1] = scale * np.float32(growth), np.float32(0.0)
    return True


def scaler_sequence():
    """40 updates, pseudo-random but fixed, with a non-finite run that reaches the floor of 1.0 from 4 and stays there,
    and finite runs that hit the growth interval of 3 exactly, twice in a row."""
    rnd = random.Random(7)
    seq = [rnd.choice([1.5, 1.5, 3e4, float("inf"), float("nan")]) for _ in range(40)]
    seq[4:9] = [float("inf"), float("nan"), float("inf"), float("nan"), float("inf")]
    seq[12:18] = [2.0, 0.0, 7.5, 1e-3, 4.0, 3e38]
    return seq


@pytest.mark.parametrize("with_step", [True, False])
def test_loss_scale_update_is_gradscaler_step_by_step(with_step):
    growth, backoff, interval = 2.0, 0.5, 3
    want = np.array([4.0, 0.0, 0.25, 1.0], dtype=np.float32)
    state = dev(want)
    step_dev = torch.zeros(1, dtype=torch.int64, device=DEV) if with_step else None
    ss = torch.zeros(1, device=DEV)
    steps, floor_hit, grown = 0, False, 0
    for i, x in enumerate(scaler_sequence()):
        ss.fill_(x)
        before = float(want[0])
        steps += scaler_model(want, math.isfinite(x), growth, backoff, interval)
        _C.loss_scale_update(state, ss, step_dev, growth, backoff, interval)
        assert np.array_equal(bits(state), want.view(np.int32)), (i, x, host(state), want)
        if with_step:
            assert int(step_dev.item()) == steps, (i, x)
        floor_hit |= (not math.isfinite(x)) and before == 1.0 and want[0] == 1.0
        grown += want[0] > before
    assert floor_hit and grown >= 2 and 0 < steps < 40     # the sequence does what its docstring says


# ------------------------------------------------------------------------------------- FlatLoraState.step (§4)
N_FLAT = 4096 + 5
FLAT_GROUPS = [(0, 4096, 1e-2, 1e-2), (4096, N_FLAT, 5e-3, 0.0)]


def make_state(max_grad_norm=1.0, scaling=None):
    """Two parameter tensors (4096 and 5 elements) in two groups: a flat buffer of 4096 + 5 floats."""
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(N_FLAT, generator=gen) * 0.1
    a = torch.nn.Parameter(p0[:4096].clone().to(DEV))
    b = torch.nn.Parameter(p0[4096:].clone().to(DEV))
    st = T.FlatLoraState([{"params": [a], "lr": FLAT_GROUPS[0][2], "weight_decay": FLAT_GROUPS[0][3]},
                          {"params": [b], "lr": FLAT_GROUPS[1][2], "weight_decay": FLAT_GROUPS[1][3]}],
                         max_grad_norm=max_grad_norm, device=torch.device(DEV))
    if scaling is not None:
        st.enable_loss_scaling(**scaling)
    return st, p0.numpy()


def flat_grads(k):
    """Norm about 3.4: above max_grad_norm = 1, so the clip is active."""
    return [grad_data(N_FLAT, seed=50 + i) * np.float32(4.0) for i in range(k)]


class RefOptimiser:
    """clip_grad_norm_ + AdamW (+ GradScaler) over one flat f64 buffer: the trajectory FlatLoraState.step must follow."""

    def __init__(self, p0, groups, max_norm, scaling=None):
        self.p, self.m, self.v = p0.astype(np.float64), np.zeros(p0.size), np.zeros(p0.size)
        self.groups, self.max_norm, self.t = [list(g) for g in groups], max_norm, 0
        self.cfg = None
        if scaling is not None:
            s = np.float32(scaling["init_scale"])
            self.sc = np.array([s, 0.0, np.float32(1.0) / s, 1.0], dtype=np.float32)
            self.cfg = (scaling.get("growth_factor", 2.0), scaling.get("backoff_factor", 0.5), scaling["growth_interval"])

    def set_lrs(self, lrs):
        for g, lr in zip(self.groups, lrs):
            g[2] = lr

    def step(self, g, grad_scale=1.0):
        """``g``: the gradient as stored (scaled by the loss scale when scaling is on; may hold inf / nan)."""
        g64 = g.astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            ss = float(np.sum(g64 * g64))
        gs = f32(grad_scale)
        if self.cfg is not None:
            if not scaler_model(self.sc, math.isfinite(ss), *self.cfg):
                return False                                  # GradScaler.step skips; the step does not count
            gs = gs * np.float64(self.sc[2])                  # unscale: exact for power-of-two scales
        self.t += 1
        self.p, self.m, self.v, _ = ref_adamw(self.p, g64, self.m, self.v, self.groups, self.t,
                                              ref_coef(ss, gs, self.max_norm))
        return True


def assert_follows(st, ref, what):
    np.testing.assert_allclose(host(st.flat_p), ref.p, rtol=3e-6, atol=3e-7, err_msg=str(what))   # §2(c)'s tolerance


def assert_same_bits(a, b, what):
    for name in ("flat_p", "exp_avg", "exp_avg_sq", "flat_g"):
        assert np.array_equal(bits(getattr(a, name)), bits(getattr(b, name))), (what, name)


def feed(st, g):
    st.flat_g.copy_(dev(g))


def test_graph_safe_steps_called_eagerly_equal_eager_steps():
    """§4(a): the device-step form without a scaler (step_advance, then clip_adamw on the device step) through FlatLoraState."""
    (sg, p0), (se, _) = make_state(), make_state()
    ref = RefOptimiser(p0, FLAT_GROUPS, 1.0)
    for k, g in enumerate(flat_grads(5)):
        feed(sg, g), feed(se, g)
        sg.step(1.0, graph_safe=True)
        se.step(1.0)
        ref.step(g)
        assert_same_bits(sg, se, k)
        assert_follows(sg, ref, k)
    assert int(sg._step_dev.item()) == sg.step_count == se.step_count == 5
    assert not np.array_equal(bits(sg.flat_p), p0.view(np.int32))


def capture_step(st, g_warm, grad_scale=1.0):
    """Warm up one graph_safe step on a side stream (it is a real step on ``g_warm``), then capture
    [flat_g <- static_g; step] as one linear chain.  Returns (graph, static_g)."""
    static_g = dev(g_warm)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        st.flat_g.copy_(static_g)
        st.step(grad_scale, graph_safe=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.flat_g.copy_(static_g)
        st.step(grad_scale, graph_safe=True)
    return graph, static_g


def test_captured_step_replays_as_eager_steps():
    """§4(b) without loss scaling: warm-up + 4 replays == 5 eager steps of the twin, new gradients every replay, new
    learning rates (set_lrs) from the third replay on."""
    (sg, p0), (se, _) = make_state(), make_state()
    ref = RefOptimiser(p0, FLAT_GROUPS, 1.0)
    gs = flat_grads(5)
    graph, static_g = capture_step(sg, gs[0])
    feed(se, gs[0]), se.step(1.0), ref.step(gs[0])
    assert_same_bits(sg, se, "warm-up")
    for k, g in enumerate(gs[1:]):
        if k == 2:
            for o in (sg, se, ref):
                o.set_lrs([2e-3, 7e-2])
        static_g.copy_(dev(g))
        graph.replay()
        feed(se, g), se.step(1.0), ref.step(g)
        assert_same_bits(sg, se, k)
        assert_follows(sg, ref, k)
    assert int(sg._step_dev.item()) == 5
    # the new rates were used: the same replay with the old ones lands elsewhere (5 elements of group 2: lr x 14)
    assert float((sg.flat_p[4096:] - dev(p0)[4096:]).abs().max()) > 5e-2
    # after a capture the host count is stale: an eager host-step call must refuse, a graph_safe one goes on correctly
    with pytest.raises(RuntimeError, match="graph_safe"):
        sg.step(1.0)
    g = grad_data(N_FLAT, seed=77) * np.float32(4.0)
    feed(sg, g), sg.step(1.0, graph_safe=True)
    feed(se, g), se.step(1.0)
    assert_same_bits(sg, se, "graph_safe after replays")
    assert int(sg._step_dev.item()) == 6


def test_captured_step_with_loss_scaling_skips_an_inf_replay():
    """§4(b) with loss scaling (init 1024, growth interval 2): the replay at index 2 carries one inf -> skipped, the
    scale backs off, the step counter stays, flat_g is zero; checked against the GradScaler model + f64 AdamW and, bit
    for bit, against the twin's eager steps."""
    scaling = dict(init_scale=1024.0, growth_interval=2)
    (sg, p0), (se, _) = make_state(scaling=scaling), make_state(scaling=scaling)
    ref = RefOptimiser(p0, FLAT_GROUPS, 1.0, scaling)
    gs = flat_grads(5)
    g0 = gs[0] * ref.sc[0]
    graph, static_g = capture_step(sg, g0)
    feed(se, g0), se.step(1.0), ref.step(g0)
    scales = []
    for k, g in enumerate(gs[1:]):
        g = g * ref.sc[0]                       # the backward would have multiplied the loss by the current scale
        if k == 2:
            g[13] = float("inf")
        scales.append(float(ref.sc[0]))
        p_before, t_before = bits(sg.flat_p).copy(), ref.t
        static_g.copy_(dev(g))
        graph.replay()
        feed(se, g), se.step(1.0)
        applied = ref.step(g)
        assert applied == (k != 2)
        assert np.array_equal(bits(sg.scaler), ref.sc.view(np.int32)), (k, host(sg.scaler), ref.sc)
        assert int(sg._step_dev.item()) == ref.t == t_before + (k != 2)
        assert float(sg.flat_g.abs().sum()) == 0.0 and bool(torch.isfinite(sg.flat_g).all())
        assert np.array_equal(bits(sg.flat_p), p_before) == (k == 2)
        assert_same_bits(sg, se, k)
        assert_follows(sg, ref, k)
    assert scales == [1024.0, 2048.0, 2048.0, 1024.0] and ref.t == 4


def test_eager_steps_then_graph_safe_steps_continue_the_count():
    """§4(c): three eager steps (host step count) followed by two graph_safe steps (device counter) are five eager
    steps.  Before the counter was seeded the fourth step ran with bias correction 1 - 0.9^1 instead of 1 - 0.9^4."""
    (sm, p0), (se, _) = make_state(), make_state()
    ref = RefOptimiser(p0, FLAT_GROUPS, 1.0)
    for k, g in enumerate(flat_grads(5)):
        feed(sm, g), feed(se, g)
        sm.step(1.0, graph_safe=k >= 3)
        se.step(1.0)
        ref.step(g)
        assert_same_bits(sm, se, k)
        assert_follows(sm, ref, k)
    assert int(sm._step_dev.item()) == 5


def test_graph_safe_steps_then_eager_steps_continue_the_count(monkeypatch):
    """§4(c), the reverse order, nothing captured: the host count moved with every call, so eager steps are right; and
    back again.  Capturing after host-count steps without a graph_safe warm-up must refuse (the graph would replay
    from a stale device counter)."""
    (sm, p0), (se, _) = make_state(), make_state()
    ref = RefOptimiser(p0, FLAT_GROUPS, 1.0)
    for k, g in enumerate(flat_grads(6)):
        feed(sm, g), feed(se, g)
        sm.step(1.0, graph_safe=k in (0, 1, 4))
        se.step(1.0)
        ref.step(g)
        assert_same_bits(sm, se, k)
        assert_follows(sm, ref, k)
    assert int(sm._step_dev.item()) == 5 and sm.step_count == 6   # the device counter was last used at step 5
    before = bits(sm.flat_p).copy()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="warm-up"):
        sm.step(1.0, graph_safe=True)
    assert sm.step_count == 6 and np.array_equal(bits(sm.flat_p), before)   # refused before anything was launched


@pytest.mark.parametrize("max_grad_norm,grad_scale", [(0.0, 1.0), (1.0, 0.5)])
def test_loss_scaling_without_clipping_and_with_grad_scale(max_grad_norm, grad_scale):
    """§4(d): a scaler with max_norm = 0, and a scaler with grad_scale != 1 (clipping the norm of the unscaled, averaged
    gradient), 4 steps against the f64 model."""
    scaling = dict(init_scale=1024.0, growth_interval=2)
    st, p0 = make_state(max_grad_norm=max_grad_norm, scaling=scaling)
    ref = RefOptimiser(p0, FLAT_GROUPS, max_grad_norm, scaling)
    for k, g in enumerate(flat_grads(4)):
        g = g * ref.sc[0] * np.float32(30.0 if k == 1 else 1.0)     # one step far above max_norm, the others near it
        feed(st, g)
        st.step(grad_scale, graph_safe=bool(k % 2))
        assert ref.step(g, grad_scale)
        assert np.array_equal(bits(st.scaler), ref.sc.view(np.int32)), k
        assert_follows(st, ref, k)
    assert int(st._step_dev.item()) == 4 and float(ref.sc[0]) == 4096.0


# ------------------------------------------------------------------------------------------- ti_rows_step (§5)
TI_DT = {"f32": (torch.float32, 0.0), "bf16": (torch.bfloat16, 2.0 ** -8), "f16": (torch.float16, 2.0 ** -11)}


def ref_ti_rows(rows, m, v, grad, lr, wd, grad_scale, step, lam, target=0.4):
    """AdamW on the rows, then F.normalize(row) * (norm + lam (target - norm)) when lam >= 0; f64."""
    lr, wd, gs, b1, b2, eps = f32(lr), f32(wd), f32(grad_scale), f32(B1), f32(B2), f32(EPS)
    g = grad * gs
    p = rows * (1 - lr * wd)
    m = m + (g - m) * (1 - b1)
    v = v * b2 + (1 - b2) * g * g
    p = p - (lr / (1 - b1 ** step)) * (m / (np.sqrt(v) / math.sqrt(1 - b2 ** step) + eps))
    if lam >= 0:
        norm = np.sqrt((p * p).sum(-1, keepdims=True))
        p = p / np.maximum(norm, 1e-12) * (norm + f32(lam) * (f32(target) - norm))
    return p, m, v


@pytest.mark.parametrize("lam", [-1.0, 0.5])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("ids", [[10], [10, 0, 7]])
@pytest.mark.parametrize("hidden", [5, 100, 257, 768])
def test_ti_rows_step_shapes_dtypes_and_decay(hidden, ids, dt, lam):
    """Rows 0 and V - 1 among unsorted ids, hidden below / not a multiple of / above the 256 threads, grad_scale 0.5,
    steps 1..3.  Tolerances: those of test_ti_rows_step_matches_full_table_adamw."""
    tdt, eps_dt = TI_DT[dt]
    V, lr, wd, gs = 11, 5e-3, 0.01, 0.5
    gen = torch.Generator().manual_seed(hidden + len(ids))
    table0 = (torch.randn(V, hidden, generator=gen) * 0.02).to(tdt)
    table = table0.clone().to(DEV)
    idt = torch.tensor(ids, device=DEV)
    rows = table[idt].float().clone()
    m, v = torch.zeros_like(rows), torch.zeros_like(rows)
    rp = table0[ids].double().numpy()
    rm, rv = np.zeros_like(rp), np.zeros_like(rp)
    for step in (1, 2, 3):
        g = (torch.randn(V, hidden, generator=gen) * 0.1).to(tdt)
        rp, rm, rv = ref_ti_rows(rp, rm, rv, g[ids].double().numpy(), lr, wd, gs, step, lam)
        _C.ti_rows_step(table, g.to(DEV), idt, rows, m, v, lr, step, weight_decay=wd, grad_scale=gs, decay_lambda=lam)
        np.testing.assert_allclose(host(rows), rp, rtol=2e-5, atol=2e-6, err_msg=f"rows, step {step}")
        np.testing.assert_allclose(host(table[idt].float()), rp, rtol=eps_dt + 2e-5, atol=2e-6, err_msg=f"table, step {step}")
    np.testing.assert_allclose(host(m), rm, rtol=2e-5, atol=2e-6 * 0.1)
    np.testing.assert_allclose(host(v), rv, rtol=2e-5, atol=2e-6 * 0.01)
    assert torch.equal(table[idt].cpu(), rows.to(tdt).cpu())          # the table holds the rounded master rows
    keep = torch.ones(V, dtype=torch.bool)
    keep[ids] = False
    assert torch.equal(table.cpu()[keep].view(torch.uint8), table0[keep].view(torch.uint8))   # other rows: same bits


@pytest.mark.parametrize("lam", [-1.0, 0.5])
@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_ti_rows_step_zero_row_stays_zero(dt, lam):
    """A zero row with a zero gradient: norm = 0 takes the fmaxf(norm, 1e-12) branch; 0 * (0.2 / 1e-12) must be 0."""
    tdt, _ = TI_DT[dt]
    V, hidden, ids = 11, 100, [10, 0, 7]
    gen = torch.Generator().manual_seed(3)
    table0 = (torch.randn(V, hidden, generator=gen) * 0.02).to(tdt)
    table0[7] = 0
    table = table0.clone().to(DEV)
    idt = torch.tensor(ids, device=DEV)
    rows = table[idt].float().clone()
    m, v = torch.zeros_like(rows), torch.zeros_like(rows)
    for step in (1, 2, 3):
        g = (torch.randn(V, hidden, generator=gen) * 0.1).to(tdt)
        g[7] = 0
        _C.ti_rows_step(table, g.to(DEV), idt, rows, m, v, 5e-3, step, weight_decay=0.01, grad_scale=0.5, decay_lambda=lam)
        for t in (rows[2], m[2], v[2], table[7].float()):
            assert float(t.abs().max()) == 0.0 and bool(torch.isfinite(t).all())
        assert bool(torch.isfinite(rows).all()) and float(rows[:2].abs().max()) > 0


def test_ti_rows_step_rejects_malformed_state():
    table = torch.zeros(11, 8, device=DEV)
    grad = torch.zeros_like(table)
    ids = torch.tensor([3, 9], device=DEV)
    rows, m, v = (torch.zeros(2, 8, device=DEV) for _ in range(3))
    wide = torch.zeros(2, 16, device=DEV)
    bad = [
        dict(ids=torch.tensor([3, 0, 9, 0], device=DEV)[::2]),      # non-contiguous ids
        dict(m=wide[:, ::2]),                                       # non-contiguous m
        dict(v=wide[:, ::2]),                                       # non-contiguous v
        dict(m=m.double()),                                         # m not f32
        dict(v=v.half()),                                           # v not f32
        dict(m=torch.zeros(2, 7, device=DEV)),                      # m not of rows' shape
        dict(v=torch.zeros(3, 8, device=DEV)),                      # v not of rows' shape
    ]
    for kw in bad:
        a = dict(ids=ids, m=m, v=v)
        a.update(kw)
        with pytest.raises(ValueError):
            _C.ti_rows_step(table, grad, a["ids"], rows, a["m"], a["v"], 1e-3, 1)
    _C.ti_rows_step(table, grad, ids, rows, m, v, 1e-3, 1)          # the well-formed call goes through
    assert float(table.abs().max()) == 0.0
