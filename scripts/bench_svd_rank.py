#!/usr/bin/env python
"""cli_svd distillation of the SD1.5 UNet (224 sites of the extended injection, the shape groups of bench.py --svd) at LoRA
ranks 8, 16, 32 and 64, with ``cli_svd.WIDE`` 0 and 1 alternating in one process.

The residual of every site is planted with rank r + 4, singular values 0.6 0.95^i, plus noise of singular values ~1e-3.  Per
leg one JSON line: milliseconds per distillation (``distill_model`` over all shape groups), the sites per route
(``cli_svd.ROUTES``) and, on one site per shape group, the relative distance of the un-clamped rank-r product from the exact
truncation (float64: the projection of the residual onto the top-r eigenvectors of its smaller Gram matrix).

The WIDE=0 leg at rank 64 is one full ``torch.linalg.svd`` per site: it is timed on ONE SITE PER SHAPE GROUP (31 sites) only,
under ``--exact-limit-s`` checked between repeats, and labelled ``"subset": "31 of 224 sites"``.

    python scripts/bench_svd_rank.py [--ranks 8,16,32,64] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time
from collections import Counter

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lora_amd import cli_svd as S  # noqa: E402
from lora_amd.standin import sd15_lora_site_shapes  # noqa: E402

DEV = torch.device("cuda", 0)


def planted_groups(shapes, rank, bases, gen):
    """bench.py's svd workload (base ~ 0.05 N(0, 1) per shape group) with the spectrum of this script planted on top."""
    k = rank + 4
    sv = 0.6 * 0.95 ** torch.arange(k, device=DEV, dtype=torch.float32)
    groups = []
    for ((N, K), cnt), base in zip(shapes, bases):
        u, _ = torch.linalg.qr(torch.randn(cnt, N, k, device=DEV, generator=gen))
        v, _ = torch.linalg.qr(torch.randn(cnt, K, k, device=DEV, generator=gen))
        tuned = base + torch.bmm(u * sv, v.transpose(1, 2)) \
            + 1e-3 / (N ** 0.5 + K ** 0.5) * torch.randn(cnt, N, K, device=DEV, generator=gen)
        groups.append((list(tuned), list(base)))
    return groups


def exact_truncation(res, rank):
    """U_r S_r V_r^T of one f32 residual in float64, through the eigenvectors of the smaller Gram matrix."""
    r64 = res.double()
    if r64.shape[0] <= r64.shape[1]:
        _, vec = torch.linalg.eigh(r64 @ r64.t())
        top = vec[:, -rank:]
        return top @ (top.t() @ r64)
    _, vec = torch.linalg.eigh(r64.t() @ r64)
    top = vec[:, -rank:]
    return (r64 @ top) @ top.t()


def product_distance(firsts, exact, rank):
    """Largest relative distance over the one-site-per-group subset, through the route the current WIDE setting gives."""
    deltas = [(t - b).float()[None].contiguous() for t, b in firsts]
    gen = torch.Generator(device=DEV).manual_seed(2)
    if all(S.group_supported(d.shape[1], d.shape[2], rank) for d in deltas):
        by_l = {}
        for i, d in enumerate(deltas):   # one ragged iteration per sketch width (ranks <= 16 on narrow matrices differ)
            by_l.setdefault(S._sketch_width(rank, 8, d.shape[1], d.shape[2]), []).append(i)
        trip = [None] * len(deltas)
        for idx in by_l.values():
            for i, t in zip(idx, S.topr_svd_ragged([deltas[i] for i in idx], rank, generator=gen)):
                trip[i] = tuple(x[0] for x in t)
    else:
        trip = [S.topr_svd(d[0], rank, generator=gen) for d in deltas]
    worst = 0.0
    for (U, Sg, Vh), ex in zip(trip, exact):
        worst = max(worst, float(((U * Sg).double() @ Vh.double() - ex).norm() / ex.norm()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="8,16,32,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--exact-limit-s", type=float, default=240.0, help="stop repeating the per-site exact leg after this long")
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0), flush=True)
    shapes = sorted(Counter(sd15_lora_site_shapes(extended=True)).items())
    elems = sum(N * K * c for (N, K), c in shapes)
    gen = torch.Generator(device=DEV).manual_seed(0)
    bases = [torch.randn(cnt, N, K, device=DEV, generator=gen) * 0.05 for (N, K), cnt in shapes]
    print(json.dumps({"sites": sum(c for _, c in shapes), "shape_groups": len(shapes), "residual_elements": elems,
                      "both_planes_bytes_per_product": 4 * elems}), flush=True)
    default_wide = S.WIDE
    for rank in (int(r) for r in a.ranks.split(",")):
        groups = planted_groups(shapes, rank, bases, gen)
        firsts = [(t[0], b[0]) for t, b in groups]
        exact = [exact_truncation((t - b).float(), rank) for t, b in firsts]
        subset = [([t], [b]) for t, b in firsts]
        times = {0: [], 1: []}
        info = {}
        t_exact = 0.0
        for rep in range(a.repeats + 1):          # repeat 0 warms both legs up
            for wide in (0, 1):
                S.WIDE = bool(wide)
                per_site = rank > 32 and not wide   # every site one full SVD: the 31-site subset
                if per_site and rep > 1 and t_exact > a.exact_limit_s:
                    continue
                work = subset if per_site else groups
                before = dict(S.ROUTES)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                S.distill_model(work, rank, 0.99, torch.Generator(device=DEV).manual_seed(1))
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if per_site:
                    t_exact += dt
                if rep:
                    times[wide].append(dt * 1e3)
                if wide not in info:
                    info[wide] = {"routes": {k: S.ROUTES[k] - v for k, v in before.items() if S.ROUTES[k] != v},
                                  "sites": sum(len(t) for t, _ in work), "product_rel_distance": product_distance(firsts, exact, rank)}
        S.WIDE = default_wide
        for wide in (0, 1):
            ts = sorted(times[wide])
            line = {"rank": rank, "WIDE": wide, "ms_median": round(ts[len(ts) // 2], 2), "ms_all": [round(t, 2) for t in times[wide]],
                    "spread_ms": round(ts[-1] - ts[0], 2), **info[wide]}
            if info[wide]["sites"] != sum(c for _, c in shapes):
                line["subset"] = f"{info[wide]['sites']} of {sum(c for _, c in shapes)} sites (one per shape group)"
            if S._wide(rank) and wide:
                l = S._sketch_width(rank, 8, 320, 320)
                line["sketch_columns"] = l
                line["plane_passes"] = 10   # sketch + 4 x (dW^T Q, dW Qz) + b, each both planes
                line["plane_bytes_read"] = 10 * 4 * elems
            print(json.dumps(line), flush=True)
        del groups, firsts, exact, subset
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
