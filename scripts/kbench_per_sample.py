#!/usr/bin/env python
"""Per-sample LoRA multipliers: what the rowscale routes cost.  One JSON line per measurement.

  --what kernel  lora_amd_linear_gemm_fwd_rowscale against lora_amd_linear_gemm_fwd at the same tile, and the library
                 route (GEMM + rowdot + rank_update_rowscale), per SD1.5 shape at batch 8 (us per call, hipGraph-timed);
                 the NCHW conv up-projection with the multiplier inside (conv_up_fwd_rowscale) against a separate pass
                 over T followed by conv_up_fwd
  --what rank_update  lora_amd_rank_update_rowscale at ranks 16 / 32 / 64, p = 0 / 0.1, on the eight shapes of DESIGN
                 §3.4b's rank_update table (batch-8 rows per sample): the row-table form of the matrix-core kernel (hook
                 on) against the VALU kernel (hook off), alternating, and the plain lora_amd_rank_update matrix-core
                 launch of the same shape beside them; --what rank_update_near: the maskless launch on a grid of shapes
                 around the one line of that table the VALU kernel wins
  --what unet    no-grad SD1.5 stand-in UNet forward at 512^2, bf16, batch 8 (CFG over 4 settings), reference-default
                 injection rank 4: (a) one scale for the batch (today's routes), (b) four per-sample alphas in one call,
                 (c) four sequential batch-2 calls with tune_lora_scale (ms per batch of 8).
                 With --members 3 --rank 16: a LoRAManager of three rank-16 member files (joined rank 48) and four member
                 mixes through tune_per_sample, hook on and off alternating in the one call
  --what trace   (b) alone, a few calls: the run to put under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lora_amd as L  # noqa: E402
from lora_amd import _C, ops  # noqa: E402
from scripts.kbench import timeit  # noqa: E402

DEV = "cuda:0"
# (M at batch 8, K, N): 64x64 / 32x32 / 16x16 / 8x8 latent rows, 77-token text rows, time-embedding rows
SHAPES = [(32768, 320, 320), (32768, 320, 2560), (8192, 640, 640), (8192, 640, 5120), (2048, 1280, 1280),
          (2048, 1280, 10240), (512, 1280, 1280), (616, 768, 320), (616, 768, 640), (616, 768, 1280), (8, 1280, 320),
          (8, 1280, 1280)]


def emit(d):
    print(json.dumps(d), flush=True)


def kernel(args):
    r, nsel = args.rank, 4
    for M, K, N in SHAPES:
        x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
        w = (torch.randn(N, K, device=DEV) * 0.03).to(torch.bfloat16)
        b = torch.zeros(N, device=DEV, dtype=torch.bfloat16)
        down, up = torch.randn(r, K, device=DEV) * 0.2, torch.randn(N, r, device=DEV) * 0.05
        rows = torch.rand(nsel, r, device=DEV)
        rps = max(M // 8, 1)
        row = {"M": M, "K": K, "N": N, "r": r}
        ring_ok = _C.gemm_supported(x, w, N, r)
        if ring_ok:
            row["ring_us"] = timeit(lambda: _C.linear_gemm_fwd(x, w, b, down, up, 0.7, 0))[0] * 1e6
            row["ring_rowscale_us"] = timeit(lambda: _C.linear_gemm_fwd_rowscale(x, w, b, down, up, 0.7, rows, rps, 0))[0] * 1e6
            row["ratio"] = row["ring_rowscale_us"] / row["ring_us"]
        lib_rows = torch.rand(nsel, r, device=DEV)

        def lib():
            y = torch.nn.functional.linear(x, w, b)
            t = _C.rowdot(x, down, _C.FACTOR_RK)
            _C.rank_update_rowscale_(y, t, up, _C.FACTOR_KR, 0.7, lib_rows, rps)

        row["lib_rowscale_us"] = timeit(lib)[0] * 1e6
        row["static_choice"] = "ring" if ops.static_rowscale_choice(M, K, N, ring_ok) == ops.PS_RING else "lib"
        emit(row)
    for B, C, H in ((8, 320, 64), (8, 640, 32), (8, 1280, 16), (8, 1280, 8)):
        y = torch.randn(B, C, H, H, device=DEV).to(torch.bfloat16)
        t = torch.randn(B, r, H, H, device=DEV)
        up = torch.randn(C, r, device=DEV) * 0.05
        rows = torch.rand(nsel, r, device=DEV)
        inside = timeit(lambda: _C.conv_up_fwd_rowscale_(y, t, up, 0.7, rows))[0] * 1e6
        mult = rows[torch.arange(B, device=DEV) % nsel].view(B, r, 1, 1).contiguous()

        def separate():
            t.mul_(mult)
            _C.conv_up_fwd_(y, t, up, 0.7, 0.0, 0, 0)

        emit({"conv_up": [B, C, H, H], "r": r, "rowscale_inside_us": inside, "pass_then_conv_up_us": timeit(separate)[0] * 1e6})


# (M, N) of DESIGN §3.4b's rank_update table: batch-8 rows of the 64x64 .. 8x8 maps and of the text tokens
RU_SHAPES = [(9216, 320), (9216, 2560), (2304, 640), (2304, 5120), (576, 1280), (576, 10240), (144, 1280), (77, 1280)]


def rank_update(args):
    """lora_amd_rank_update_rowscale with the hook on (row-table form of the matrix-core kernel) and off (VALU kernel),
    alternating, and the plain lora_amd_rank_update matrix-core launch of the same shape beside it."""
    nsel = 4
    for M, N in RU_SHAPES:
        for r in (16, 32, 64):
            for p in (0.0, 0.1):
                y = torch.randn(M, N, device=DEV).to(torch.bfloat16)
                t = torch.randn(M, r, device=DEV) * 1e-3
                up = torch.randn(N, r, device=DEV) * 0.05
                rows = torch.rand(nsel, r, device=DEV)
                rps = max(M // 8, 1)
                fns = {"mfma": lambda: _C.rank_update_rowscale_(y, t, up, _C.FACTOR_KR, 0.7, rows, rps, p, 5, 9),
                       "valu": lambda: _C.rank_update_rowscale_(y, t, up, _C.FACTOR_KR, 0.7, rows, rps, p, 5, 9),
                       "plain_mfma": lambda: _C.rank_update_(y, t, up, _C.FACTOR_KR, 0.7, p, 5, 9)}
                takes = _C.rank_update_rowscale_takes(y, r)
                meds = {k: [] for k in fns}
                for _ in range(args.rounds):
                    for tag, fn in fns.items():
                        prev = _C.rank16_mfma(0 if tag == "valu" else 1)
                        try:
                            meds[tag].append(timeit(fn, args.reps)[0] * 1e6)
                        finally:
                            _C.rank16_mfma(prev)
                res = {"M": M, "N": N, "r": r, "p": p, "rps": rps, "takes": takes}
                for tag, v in meds.items():
                    res[tag + "_us"] = round(min(v), 2)
                    res[tag + "_rounds_us"] = [round(u, 2) for u in v]
                res["valu_over_mfma"] = round(res["valu_us"] / res["mfma_us"], 2)
                res["mfma_over_plain"] = round(res["mfma_us"] / res["plain_mfma_us"], 3)
                emit(res)


def rank_update_near(args):
    """The maskless launch around the one line of --what rank_update that the VALU kernel wins (2304 x 5120, rank 32):
    ranks 17 / 24 / 32 / 48 on a grid of row counts and widths, hook on / off twice each, alternating."""
    for r in (17, 24, 32, 48):
        for M in (1024, 2048, 2304, 4096, 8192):
            for N in (2560, 5120, 10240):
                y = torch.randn(M, N, device=DEV).to(torch.bfloat16)
                t = torch.randn(M, r, device=DEV) * 1e-3
                up = torch.randn(N, r, device=DEV) * 0.05
                rows = torch.rand(4, r, device=DEV)
                rps = max(M // 8, 1)
                fn = lambda: _C.rank_update_rowscale_(y, t, up, _C.FACTOR_KR, 0.7, rows, rps)
                res = {"M": M, "N": N, "r": r}
                for tag, hook in (("mfma", 1), ("valu", 0), ("mfma2", 1), ("valu2", 0)):
                    prev = _C.rank16_mfma(hook)
                    try:
                        res[tag] = round(timeit(fn, args.reps)[0] * 1e6, 2)
                    finally:
                        _C.rank16_mfma(prev)
                res["valu_over_mfma"] = round(min(res["valu"], res["valu2"]) / min(res["mfma"], res["mfma2"]), 3)
                emit(res)


def build_joined(args):
    """The stand-in UNet with a LoRAManager of ``args.members`` member files of rank ``args.rank`` each (written to a
    temporary directory from freshly drawn factors): one joined adapter of rank members * rank per site."""
    import tempfile
    import types

    from bench import build_unet
    from lora_amd import trainer as T
    from lora_amd.lora_manager import LoRAManager

    torch.manual_seed(0)
    unet = build_unet(torch.device(DEV), torch.bfloat16, seed=0)
    unet.to(memory_format=torch.channels_last)
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        L.inject_trainable_lora(unet, r=args.rank)
        for i in range(args.members):
            for up, down in L.extract_lora_ups_down(unet):
                up.weight.data.normal_(0, 0.02)
                down.weight.data.normal_(0, 1.0 / args.rank)
            paths.append(os.path.join(tmp, f"member{i}.safetensors"))
            L.save_safeloras({"unet": (unet, L.DEFAULT_TARGET_REPLACE)}, paths[-1])
        L.monkeypatch_remove_lora(unet)
        pipe = types.SimpleNamespace(unet=unet, text_encoder=torch.nn.Identity(), tokenizer=None)
        mgr = LoRAManager(paths, pipe)
    T.promote_lora_to_fp32(unet)
    unet.eval()
    return mgr, unet


def build(args):
    from bench import build_unet
    from lora_amd import trainer as T

    torch.manual_seed(0)
    unet = build_unet(torch.device(DEV), torch.bfloat16, seed=0)
    unet.to(memory_format=torch.channels_last)
    L.inject_trainable_lora(unet, r=args.rank)
    T.promote_lora_to_fp32(unet)
    for up, _ in L.extract_lora_ups_down(unet):
        up.weight.data.normal_(0, 0.02)
    unet.eval()
    return (unet,) + inputs()


def inputs():
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(8, 4, 64, 64, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    t = torch.full((8,), 500, device=DEV)
    ehs = torch.randn(8, 77, 768, device=DEV, generator=g).to(torch.bfloat16)
    return x, t, ehs


def time_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2], out[0]


@torch.no_grad()
def unet_joined(args):
    """Four member mixes through LoRAManager.tune_per_sample at joined rank members * rank: the per-sample rank update of
    every site on the matrix cores (hook on) and on the VALU kernel (hook off), alternating in one call."""
    mgr, net = build_joined(args)
    x, t, ehs = inputs()
    mixes = [[1.0] + [0.0] * (args.members - 1), [0.0] * (args.members - 1) + [1.0], [0.5] * args.members,
             [1.5, 0.25] + [1.0] * (args.members - 2)]
    mgr.tune_per_sample(mixes)
    ops.PATH_LOG = log = []
    net(x, t, ehs)
    ops.PATH_LOG = None
    routes = {}
    for _, path, *_ in log:
        routes[path] = routes.get(path, 0) + 1
    res = {"on": [], "off": []}
    for _ in range(args.rounds):
        for tag, hook in (("on", 1), ("off", 0)):
            prev = _C.rank16_mfma(hook)
            try:
                res[tag].append(time_ms(lambda: net(x, t, ehs), args.reps))
            finally:
                _C.rank16_mfma(prev)
    on, off = min(m for m, _ in res["on"]), min(m for m, _ in res["off"])
    emit({"metric": "SD1.5 stand-in UNet forward, 512^2, bf16, batch 8, no grad, LoRAManager.tune_per_sample of 4 mixes "
                    "(ms, median / best per round)", "members": args.members, "member_rank": args.rank,
          "joined_rank": args.members * args.rank, "routes": routes, "hook_on": res["on"], "hook_off": res["off"],
          "hook_on_ms": on, "hook_off_ms": off, "off_over_on": off / on})


@torch.no_grad()
def unet(args):
    if args.members > 1:
        return unet_joined(args)
    net, x, t, ehs = build(args)
    alphas = [0.25, 0.5, 1.0, 1.5]

    def uniform():
        net(x, t, ehs)

    def sequential():
        for q, a in enumerate(alphas):
            L.tune_lora_scale(net, a)
            idx = [q, q + 4]
            net(x[idx], t[idx], ehs[idx])

    L.tune_lora_scale(net, 1.0)
    a_ms = time_ms(uniform, args.reps)
    c_ms = time_ms(sequential, args.reps)
    L.tune_lora_scale(net, 1.0)
    L.tune_lora_scale_per_sample(net, alphas)
    b_ms = time_ms(uniform, args.reps)
    L.clear_lora_per_sample(net)
    emit({"metric": "SD1.5 stand-in UNet forward, 512^2, bf16, batch 8, no grad (ms, median / best)",
          "a_uniform": a_ms, "b_per_sample_alphas": b_ms, "c_four_batch2_calls": c_ms,
          "b_over_a": b_ms[0] / a_ms[0], "b_over_c": b_ms[0] / c_ms[0]})


@torch.no_grad()
def trace(args):
    net, x, t, ehs = build(args)
    L.tune_lora_scale_per_sample(net, [0.25, 0.5, 1.0, 1.5])
    for _ in range(args.reps):
        net(x, t, ehs)
    torch.cuda.synchronize()
    emit({"trace": "per-sample alphas, batch 8", "calls": args.reps})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["kernel", "rank_update", "rank_update_near", "unet", "trace"], default="kernel")
    ap.add_argument("--rank", type=int, default=4)
    ap.add_argument("--members", type=int, default=1,
                    help="--what unet: > 1 joins that many member files of --rank through a LoRAManager")
    ap.add_argument("--rounds", type=int, default=2, help="alternating hook-on / hook-off rounds of one call")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    {"kernel": kernel, "rank_update": rank_update, "rank_update_near": rank_update_near, "unet": unet,
     "trace": trace}[a.what](a)
