"""The timed step, site by site (BASELINE configs[1]: SD1.5 size, rank 4, batch 4, 512^2, bf16, channels-last, head-padded
and grouped projections, the hostops passes, the merged-weight route that bench.py times, up != 0).

1. Per-site factor gradients, element by element: in one eager step after the warm-up, every site's (G, X) is recorded where
   the merged route hands them to the factor kernels (``ops.MergedWeights.owe``); each site's slices of ``flat_g`` must equal
   f64 ``s G^T (X down^T)`` and ``s (G up)^T X`` on those operands within 1e-4 of the absolute bound (the kernel tests'
   tolerance).  No oracle twin is needed: the reference is f64 on the operands the step itself produced.
2. Replay against eager: two eager steps on the same inputs and state give the spread of the library's attention / GEMM
   picks; the step captured with ``T.GraphedForwardBackward`` and replayed on the same inputs must give the loss and every
   element of ``flat_g`` within ``SPREAD_FACTOR`` x that spread plus ``FLOOR`` x the largest gradient (the floor covers a
   bit-reproducible eager step: replayed kernels may sum in another order).
3. Poisoned free memory: ``tests/memguard.poison_free_blocks`` before each eager step and each replay; same bounds, no NaN or
   Inf in the loss, ``flat_g`` or the scratch weights.
4. The same checks in a child process under the benchmark's convolution picks (``bench.private_miopen_db``: a temporary copy
   of bench_tuning/miopen; the parent's ``MIOPEN_USER_DB_PATH`` removed from the child's environment).
5. Check 1 on the per-site route (``bench.py --merged 0``, the r3 test's ``bench_fused_sites``): every site's (G, X) is
   recorded where its autograd backward receives them (``ops.LoraLinearFunction``, ``LoraLinearHeadsFunction``,
   ``LoraLinearGroupFunction``; a grouped q / k / v launch yields three sites) and judged by the same ``site_errors``; in the
   pytest process and in the child of check 4.

Run as a script (``python tests/test_gpu_step_sites.py [--seeded-db]``) it prints the measurements as one JSON line.
"""
from __future__ import annotations

import contextlib
import json
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

DEV = "cuda:0"
D1_K = 1e-4            # factor gradients: 1e-4 of the absolute bound
SPREAD_FACTOR = 4.0    # replay / poisoned runs vs eager: 4 x the eager-vs-eager spread ...
FLOOR = 1e-5           # ... plus 1e-5 of the largest |flat_g| element (and of |loss|)
N_SITES = 144


def _heads_cols(n, d, D, device):
    i = torch.arange(n, device=device)
    return (i // d) * D + i % d


def _logical(t, heads):
    """Head-padded rows (heads, d, D) -> the logical [M, heads * d] columns."""
    if not heads:
        return t
    h, d, D = heads
    return t[:, _heads_cols(h * d, d, D, t.device)]


def site_errors(records, modules, st, k=D1_K):
    """Per recorded site: max |flat_g - f64| / tolerance over d_up and d_down (> 1 = outside the bound)."""
    by_ptr = {(m.lora_up.weight.data_ptr(), m.lora_down.weight.data_ptr()): m for m in modules}
    worst = {}
    for g2, x2, down, up, scale, g_heads, x_heads in records:
        m = by_ptr[(up.data_ptr(), down.data_ptr())]
        G, X = _logical(g2, g_heads).double(), _logical(x2, x_heads).double()
        A, U = down.double(), up.double()
        T = X @ A.t()
        want_up, ref_up = scale * G.t() @ T, scale * G.abs().t() @ (X.abs() @ A.abs().t())
        Gt = G @ U
        want_dn, ref_dn = scale * Gt.t() @ X, scale * (G.abs() @ U.abs()).t() @ X.abs()
        e = 0.0
        for got, want, ref in ((st.grad_view(m.lora_up.weight), want_up, ref_up),
                               (st.grad_view(m.lora_down.weight), want_dn, ref_dn)):
            got = got.double()
            if not bool(torch.isfinite(got).all()):
                e = float("inf")
                break
            e = max(e, float(((got - want).abs() / (k * ref + 1e-30)).max()))
        worst[id(m)] = max(worst.get(id(m), 0.0), e)
    return worst


def _scratch_finite(merged) -> bool:
    for e in merged.entries.values():
        for key in ("w_eff", "w_eff_t", "b_eff"):
            t = e.get(key)
            if t is not None and t.is_floating_point() and not bool(torch.isfinite(t).all()):
                return False
    return True


@contextlib.contextmanager
def per_site_records(records):
    """Record (G, X, down, up, scale, G's head layout, X's head layout) of every site where the per-site route's autograd
    backward receives them, in the form ``site_errors`` takes.  A backward that detours through dense copies enters
    ``LoraLinearFunction.backward`` a second time: that site is then recorded twice, padded and dense."""
    from lora_amd import _C, ops

    classes = (ops.LoraLinearFunction, ops.LoraLinearHeadsFunction, ops.LoraLinearGroupFunction)
    orig = {c: c.__dict__["backward"] for c in classes}

    def single(fn):
        def backward(ctx, g):
            x2, weight, down, up = ctx.saved_tensors[:4]
            ih, oh = getattr(ctx, "in_heads", None), getattr(ctx, "out_heads", None)
            g2 = ops._rows2d(g, _C.heads_width(weight.shape[0], oh))
            records.append((g2.detach().clone(), x2.detach().clone(), down.detach(), up.detach(), float(ctx.scale), oh, ih))
            return fn(ctx, g)
        return staticmethod(backward)

    def group(fn):
        def backward(ctx, *grads):
            saved, n = ctx.saved_tensors, ctx.n
            x2, rest = saved[0].detach().clone(), saved[1 + n:]
            for i in range(n):
                weight, down, up = rest[3 * i:3 * i + 3]
                if grads[i] is not None:
                    g2 = ops._rows2d(grads[i], weight.shape[0])
                    records.append((g2.detach().clone(), x2, down.detach(), up.detach(), float(ctx.meta[i][0]), None, None))
            return fn(ctx, *grads)
        return staticmethod(backward)

    for c in classes:
        c.backward = (group if c is ops.LoraLinearGroupFunction else single)(orig[c].__func__)
    try:
        yield records
    finally:
        for c in classes:
            c.backward = orig[c]


def build_step(merged=True):
    """The device UNet as bench.py builds it, adapters with up != 0, the merged route's state (``merged=False``: the per-site
    fused kernels, bench.py --merged 0), inputs; -> dict."""
    from bench import build_unet
    import lora_amd as L
    from lora_amd import trainer as T
    from lora_amd.standin import DDPMScheduler

    unet = build_unet(torch.device(DEV), torch.bfloat16, seed=0)
    L.inject_trainable_lora(unet, r=4)
    T.promote_lora_to_fp32(unet)
    mods = [m for m in unet.modules() if isinstance(m, L.LoraInjectedLinear)]
    assert len(mods) == N_SITES
    g = torch.Generator().manual_seed(11)
    for m in mods:
        m.lora_up.weight.data.copy_(torch.randn(m.lora_up.weight.shape, generator=g) * 0.02)
        m.lora_down.weight.data.copy_(torch.randn(m.lora_down.weight.shape, generator=g) / 4)
    unet.train()
    unet.to(memory_format=torch.channels_last)
    st = T.FlatLoraState([{"params": T.lora_params(unet), "lr": 1e-4, "weight_decay": 1e-2}], max_grad_norm=1.0,
                         device=torch.device(DEV))
    st.attach_direct_grads(unet)
    merged = st.enable_merged_weights(unet) if merged else None
    g = torch.Generator().manual_seed(123)
    B = 4
    lat = (torch.randn(B, 4, 64, 64, generator=g) * 0.18215).to(DEV).to(torch.bfloat16)
    lat = lat.contiguous(memory_format=torch.channels_last)
    ehs = torch.randn(B, 77, 768, generator=g).to(DEV).to(torch.bfloat16)
    noise = torch.randn(B, 4, 64, 64, generator=g).to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    ts = torch.randint(0, 1000, (B,), generator=g).to(DEV)
    sched = DDPMScheduler()

    def fwd_bwd(l_, c_):
        return T.forward_backward(unet, sched, l_, c_, T.StepConfig(), noise=noise, timesteps=ts, merged=merged)

    return dict(unet=unet, mods=mods, st=st, merged=merged, lat=lat, ehs=ehs, fwd_bwd=fwd_bwd)


def measure(s, mutate=None):
    """Checks 1-3 on a built step; returns the measurements (no assertion).  ``mutate(st, records)`` runs after the
    recorded step's reduce (a hook for showing that check 1 fails on a wrong gradient)."""
    from lora_amd import ops
    from lora_amd import trainer as T
    from tests import memguard as MG

    st, merged, fwd_bwd, lat, ehs = s["st"], s["merged"], s["fwd_bwd"], s["lat"], s["ehs"]
    for _ in range(2):      # attention choices are timed on first use; the padded layout applies from the second call
        fwd_bwd(lat, ehs)
        st.zero_grad()
    # ---- 1. one eager step with every site's (G, X) recorded where the merged route hands them to the factor kernels
    records = []
    orig = ops.MergedWeights.owe

    def owe(self, g2, x2, down, up, up_part, down_part, scale, g_heads, x_heads, *a, **kw):
        records.append((g2.detach().clone(), x2.detach().clone(), down.detach(), up.detach(), float(scale), g_heads, x_heads))
        return orig(self, g2, x2, down, up, up_part, down_part, scale, g_heads, x_heads, *a, **kw)

    ops.MergedWeights.owe = owe
    try:
        loss_e = float(fwd_bwd(lat, ehs))
        st.reduce_pending()
    finally:
        ops.MergedWeights.owe = orig
    torch.cuda.synchronize()
    flat_e = st.flat_g.clone()
    if mutate is not None:
        mutate(st, records)
    worst = site_errors(records, s["mods"], st)
    del records
    st.flat_g.copy_(flat_e)
    st.zero_grad()
    # ---- 2. the eager spread, then replay against eager
    loss_b = float(fwd_bwd(lat, ehs))
    st.reduce_pending()
    torch.cuda.synchronize()
    spread_g = float((st.flat_g - flat_e).abs().max())
    spread_l = abs(loss_b - loss_e)
    st.zero_grad()
    gmax = float(flat_e.abs().max())
    graphed = T.GraphedForwardBackward(fwd_bwd, lat, ehs, st)
    st.zero_grad()
    loss_r = float(graphed(lat, ehs))
    torch.cuda.synchronize()
    replay_g = float((st.flat_g - flat_e).abs().max())
    replay_l = abs(loss_r - loss_e)
    # ---- 3. poisoned free blocks before an eager step and before a replay
    poisoned = []
    for kind in ("eager", "replay"):
        st.zero_grad()
        nbytes = MG.poison_free_blocks()
        if kind == "eager":
            loss_p = float(fwd_bwd(lat, ehs))
            st.reduce_pending()
        else:
            loss_p = float(graphed(lat, ehs))
        torch.cuda.synchronize()
        finite = bool(torch.isfinite(st.flat_g).all()) and bool(torch.isfinite(torch.tensor(loss_p))) and \
            _scratch_finite(merged)
        poisoned.append(dict(kind=kind, bytes=nbytes, finite=finite, loss_diff=abs(loss_p - loss_e),
                             g_diff=float((st.flat_g - flat_e).abs().max())))
    st.zero_grad()
    return dict(n_sites=len(worst), d1_worst=max(worst.values()), d1_bad=sum(v > 1.0 for v in worst.values()),
                loss=loss_e, gmax=gmax, spread_g=spread_g, spread_l=spread_l, replay_g=replay_g, replay_l=replay_l,
                poisoned=poisoned, refreshes=merged.refreshes)


def measure_per_site(s):
    """Check 1 on the per-site route: one eager step after the warm-up, every site's (G, X) recorded at its backward."""
    st, fwd_bwd, lat, ehs = s["st"], s["fwd_bwd"], s["lat"], s["ehs"]
    assert s["merged"] is None
    for _ in range(2):
        fwd_bwd(lat, ehs)
        st.zero_grad()
    with per_site_records([]) as records:
        loss = float(fwd_bwd(lat, ehs))
        st.reduce_pending()
    torch.cuda.synchronize()
    worst = site_errors(records, s["mods"], st)
    n_records = len(records)
    # that the check can fail: one site's d_down 5 % too large must leave the bound (arithmetic on flat_g, no kernel changed).
    # The tolerance is 1e-4 of the ABSOLUTE bound, about sqrt(M) = 128 x a typical element over 16384 rows: 1 % is borderline
    m = s["mods"][len(s["mods"]) // 2]
    st.grad_view(m.lora_down.weight).mul_(1.05)
    negative = site_errors(records, s["mods"], st)[id(m)]
    del records
    st.zero_grad()
    return dict(n_sites=len(worst), n_records=n_records, d1_worst=max(worst.values()),
                d1_bad=sum(v > 1.0 for v in worst.values()), negative=negative, loss=loss)


def assert_per_site(r):
    assert r["n_sites"] == N_SITES, f"{r['n_sites']} of {N_SITES} sites recorded on the per-site route"
    assert r["d1_bad"] == 0, f"{r['d1_bad']} sites outside 1e-4 of the bound (worst {r['d1_worst']:.3g} x the tolerance)"
    assert r["negative"] > 1.0, f"a gradient 5 % too large passed the check ({r['negative']:.3g} x the tolerance)"


def assert_measurements(r):
    assert r["n_sites"] == N_SITES, f"{r['n_sites']} of {N_SITES} sites recorded on the merged route"
    assert r["d1_bad"] == 0, f"{r['d1_bad']} sites outside 1e-4 of the bound (worst {r['d1_worst']:.3g} x the tolerance)"
    tol_g = SPREAD_FACTOR * r["spread_g"] + FLOOR * r["gmax"]
    tol_l = SPREAD_FACTOR * r["spread_l"] + FLOOR * abs(r["loss"])
    assert r["replay_g"] <= tol_g and r["replay_l"] <= tol_l, f"replay vs eager outside the spread: {r}"
    for p in r["poisoned"]:
        assert p["finite"], f"non-finite loss, gradient or scratch weight after poisoning free memory: {p}"
        assert p["bytes"] > 0
        assert p["g_diff"] <= tol_g and p["loss_diff"] <= tol_l, f"poisoned {p['kind']} run outside the spread: {r}"


@pytest.fixture(scope="module")
def step():
    from lora_amd.standin import fused

    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("LORA_AMD_HEAD_PAD", "1")
        mp.setenv("LORA_AMD_GROUP_QKV", "1")
        mp.setattr(fused, "_ENABLED", True)
        s = build_step()
        try:
            yield s
        finally:
            for m in s["unet"].modules():
                m.__dict__.pop("_grad_sink", None)
                m.__dict__.pop("_merged", None)
            del s
            torch.cuda.empty_cache()


def _release(s):
    for m in s["unet"].modules():
        m.__dict__.pop("_grad_sink", None)
        m.__dict__.pop("_merged", None)


@pytest.mark.gpu
def test_per_site_route_site_by_site():
    """Check 5: the fused per-site kernels' factor gradients at step level, all 144 sites."""
    from lora_amd.standin import fused

    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("LORA_AMD_HEAD_PAD", "1")
        mp.setenv("LORA_AMD_GROUP_QKV", "1")
        mp.setattr(fused, "_ENABLED", True)
        s = build_step(merged=False)
        try:
            r = measure_per_site(s)
        finally:
            _release(s)
            del s
            torch.cuda.empty_cache()
    print(json.dumps(r))
    assert_per_site(r)


@pytest.mark.gpu
def test_timed_step_site_by_site_replay_and_poisoned_free_memory(step):
    r = measure(step)
    print(json.dumps(r))
    assert_measurements(r)


@pytest.fixture(scope="module")
def seeded_child():
    """Checks 4 and 5's child process (never exec) without MIOPEN_USER_DB_PATH: it calls bench.private_miopen_db() before its
    first convolution, so MIOpen runs on a temporary copy of bench_tuning/miopen and the user's database is never written."""
    env = {k: v for k, v in os.environ.items() if k != "MIOPEN_USER_DB_PATH"}
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--seeded-db"], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [x for x in p.stdout.splitlines() if x.startswith("{")][-1]
    print(line)
    return json.loads(line)


@pytest.mark.gpu
def test_the_same_under_the_benchmarks_convolution_picks(seeded_child):
    """Check 4: the merged route's three checks on the benchmark's convolution picks."""
    r = seeded_child
    assert r["seeded_db"], "the child did not run on the seeded database"
    assert_measurements(r)


@pytest.mark.gpu
def test_per_site_route_under_the_benchmarks_convolution_picks(seeded_child):
    """Check 5 in the child of check 4."""
    r = seeded_child
    assert r["seeded_db"], "the child did not run on the seeded database"
    assert_per_site(r["per_site"])


def _main(argv):
    seeded = "--seeded-db" in argv
    if seeded:
        import bench
        bench.private_miopen_db()
    os.environ["LORA_AMD_HEAD_PAD"] = "1"
    os.environ["LORA_AMD_GROUP_QKV"] = "1"
    from lora_amd.standin import fused
    fused._ENABLED = True
    s = build_step()
    r = measure(s)
    _release(s)
    del s
    torch.cuda.empty_cache()
    r["per_site"] = measure_per_site(build_step(merged=False))
    r["seeded_db"] = seeded and bool(os.environ.get("MIOPEN_USER_DB_PATH"))
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    _main(sys.argv[1:])
