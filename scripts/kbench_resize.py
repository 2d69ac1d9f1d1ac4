#!/usr/bin/env python
"""Rank resize of a LoRA from its factors (``cli_svd.resize_pairs``) against what the package could do before it.

Two workloads on the SD1.5 stand-in's site shapes, factors seeded here (column j of ``up`` ~ 0.05 * 0.93^j N(0, 1), ``down``
~ 0.3 N(0, 1) / sqrt(K): products whose spectrum decays but has no exact rank):

  extended   all 224 sites of the extended injection, rank 64 -> 8
  join       the 144 Linear sites, three rank-16 members joined to rank 48 with member weights (0.5, 1.0, 0.25) -> 16

Three routes, alternating in one process, host clock around work that ends in a device synchronise:

  native   ``resize_pairs`` on the kernels of csrc/lora_resize.hip (one table, four launches; the table is built inside the
           timed region), plus each launch on its own between device events
  dense    what the package offered before: the dense product of every site, then ``distill_model`` against a zero base at
           the same rank (randomized subspace iteration over ~3 GB of residuals and their planes; default clamp).  The time of
           forming the products is reported separately
  exact    ``resize_pairs`` with ``RESIZE_NATIVE = False`` (f64 SVD of the dense product on the host) on ONE SITE PER SHAPE,
           smallest first, until ``--exact-limit-s`` is used up: labelled with the number of sites it covers

and each route's excess e = (|dW - up' down'|_F - opt) / |dW|_F on one site per shape, with opt from the f64 eigenvalues of
the smaller Gram matrix of the dense f64 product (the dense route without its clamp: ``topr_svd_ragged``).  One JSON line per
measurement.

    python scripts/kbench_resize.py [--repeats 5] [--exact-limit-s 60]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lora_amd import _C  # noqa: E402
from lora_amd import cli_svd as S  # noqa: E402
from lora_amd.standin import sd15_lora_site_shapes  # noqa: E402

DEV = torch.device("cuda", 0)


def emit(d):
    print(json.dumps(d), flush=True)


def make_factors(shapes, R, gen):
    decay = 0.05 * 0.93 ** torch.arange(R, device=DEV, dtype=torch.float32)
    ups = [torch.randn(N, R, device=DEV, generator=gen) * decay for N, K in shapes]
    downs = [torch.randn(R, K, device=DEV, generator=gen) * (0.3 / K ** 0.5) for N, K in shapes]
    return ups, downs


def clock(fn, repeats):
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 3), "best_ms": round(ts[0], 3), "repeats": repeats}


def launches(sites, repeats):
    """Each of the four launches between device events (median over ``repeats``), the table built once."""
    tab = _C.ResizeTable(sites)
    tab.run()
    out = {}
    for name in ("gram", "core", "apply", "sign"):
        ts = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            getattr(tab, name)()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        out[name + "_ms"] = round(sorted(ts)[len(ts) // 2], 3)
    out["workspace_mb"] = round(tab.geo.workspace_bytes / 2 ** 20, 1)
    return out


def optimum(W, r):
    """(opt, |W|_F) in f64 from the eigenvalues of the smaller Gram matrix."""
    W = W.double()
    G = W @ W.t() if W.shape[0] <= W.shape[1] else W.t() @ W
    ev = torch.linalg.eigvalsh(G).flip(0).clamp_min(0.0)
    return float(ev[r:].sum().sqrt()), float(ev.sum().sqrt())


def excess_of(W, up, down, r):
    opt, nrm = optimum(W, r)
    return (float(torch.linalg.norm(W.double() - up.double() @ down.double())) - opt) / nrm


def workload(name, shapes, R, r, scale, args, gen):
    ups, downs = make_factors(shapes, R, gen)
    scales = None if scale is None else [scale] * len(shapes)
    scaled = ups if scale is None else [u * scale for u in ups]
    head = {"workload": name, "sites": len(shapes), "R": R, "r": r}
    first = {}
    for i, sh in enumerate(shapes):
        first.setdefault(sh, i)
    subset = sorted(first.values(), key=lambda i: shapes[i][0] * shapes[i][1])

    # dense route: the products, then distill_model per shape group against a zero base
    def products():
        return [a @ d for a, d in zip(scaled, downs)]

    def distill(prods):
        groups, zero = {}, {}
        for sh, w in zip(shapes, prods):
            groups.setdefault(sh, []).append(w)
        for sh in groups:
            zero[sh] = torch.zeros(sh, device=DEV)
        return S.distill_model([(ws, [zero[sh]] * len(ws)) for sh, ws in groups.items()], r,
                               generator=torch.Generator(device=DEV).manual_seed(1))

    native = lambda: S.resize_pairs(ups, downs, r, scales=scales)   # noqa: E731
    prods = products()
    for _ in range(2):   # warm every route
        native()
        distill(prods)
    t_native, t_dense = [], []
    for _ in range(args.repeats):   # alternating
        t_native.append(clock(native, 1)["best_ms"])
        t_dense.append(clock(lambda: distill(prods), 1)["best_ms"])
    med = lambda ts: round(sorted(ts)[len(ts) // 2], 3)   # noqa: E731
    emit({**head, "route": "native", "median_ms": med(t_native), "best_ms": min(t_native), "repeats": args.repeats,
          **launches(list(zip(ups, downs, [scale] * len(ups), [r] * len(ups))), args.repeats)})
    emit({**head, "route": "dense", "median_ms": med(t_dense), "best_ms": min(t_dense), "repeats": args.repeats,
          "products": clock(products, args.repeats), "routes": dict(S.ROUTES), "iterations": S.LAST_ITERATIONS})

    # excess on one site per shape
    nat = native()
    e_nat = max(excess_of(prods[i], *nat[i], r) for i in subset)
    trip = []
    for i in subset:
        N, K = shapes[i]
        if S.group_supported(N, K, r):
            U, Sg, Vh = S.topr_svd_ragged([prods[i][None].contiguous()], r,
                                          generator=torch.Generator(device=DEV).manual_seed(2))[0]
            trip.append((U[0] * Sg[0], Vh[0]))
        else:
            U, Sg, Vh = S.topr_svd(prods[i], r)
            trip.append((U * Sg, Vh))
    e_dense = max(excess_of(prods[i], u, d, r) for i, (u, d) in zip(subset, trip))
    emit({**head, "excess_on": f"{len(subset)} sites, one per shape", "native": e_nat, "dense_unclamped": e_dense})

    # exact host route on the subset, smallest first, under a time limit
    S.RESIZE_NATIVE = False
    try:
        t0, done, e_exact = time.perf_counter(), 0, 0.0
        for i in subset:
            if time.perf_counter() - t0 > args.exact_limit_s:
                break
            (u, d), = S.resize_pairs([ups[i]], [downs[i]], r, scales=None if scale is None else [scale])
            torch.cuda.synchronize()
            e_exact = max(e_exact, excess_of(prods[i], u, d, r))
            done += 1
        emit({**head, "route": "exact", "subset": f"{done} of {len(shapes)} sites (one per shape, smallest first)",
              "total_ms": round((time.perf_counter() - t0) * 1e3, 1), "excess": e_exact,
              "largest_site": list(shapes[subset[done - 1]]) if done else None})
    finally:
        S.RESIZE_NATIVE = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--exact-limit-s", type=float, default=60.0)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_resize.py measures on the GPU"
    _C.require()
    gen = torch.Generator(device=DEV).manual_seed(0)
    if args.only in ("", "extended"):
        workload("extended 64->8", sd15_lora_site_shapes(True), 64, 8, None, args, gen)
    if args.only in ("", "join"):
        member = torch.repeat_interleave(torch.tensor([0.5, 1.0, 0.25]), 16).to(DEV)
        workload("join 3x16->16", sd15_lora_site_shapes(False), 48, 16, member, args, gen)


if __name__ == "__main__":
    main()
