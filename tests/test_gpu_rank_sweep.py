"""Every LoRA rank 1..64 (and a few past 64) through each adapter route, module level, against float64.

The rank decides more than any other argument: the rank tile (4 / 8 / 16 / 32 / 64), VALU or matrix-core form of the
primitives (ranks 9..64 on bf16 rows), 1..4 rank-16 slices with 1..16 live ranks in the last one, register or chunked in-step
merge, factor gradients in the site's backward or in the trainer's deferred pass, three routes of a channels-last 3x3 site, and
rank chunks of 64 past ``_C.MAX_RANK``.  The module tests of those routes pick a few ranks each; this sweep builds ONE adapter
module per (site kind, activation dtype, rank), runs forward and backward with the matrix-core hook on and off
(``_C.rank16_mfma``) and compares ``y``, ``y - y0`` (``y0``: the same forward with ``lora_up`` zeroed), ``dx``, ``d lora_down`` and
``d lora_up`` with ``oracle/torch_ref``'s op sequence under autograd in float64 on the CPU, on the values the device sees (inputs
and frozen weights rounded to the activation dtype first; the dropout mask restated by ``helpers.philox_dropout_mask``).

Inputs: x, g ~ N(0, 1); frozen weight and ``lora_down`` ~ N(0, 1 / fan_in); ``lora_up`` ~ N(0, (LOW_TO_FROZEN / SCALE)^2 / r), so
that at EVERY rank the low-rank term of y (and of dx) has LOW_TO_FROZEN times the norm of the frozen term: the frozen weight
cannot drown the branch, and ``y - y0`` is held to the low-rank term alone.  tests/test_rank_sweep_cpu.py checks without a GPU
that with these inputs a dropped last rank exceeds four times every bound below.

Bounds (``_check_module`` of tests/test_gpu_conv_nhwc_wide.py without its absolute term; one route has three
measured bounds of its own, BRANCH_BF16 below):
  16-bit activations, e = 2^-7 (bf16) / 2^-9 (f16): max|y - ref| <= e max|ref|, the same for y - y0 against the low-rank term,
  max|dx - ref| <= 2 e max|ref|, each factor gradient within 4e-3 max|ref|;
  f32 activations: |got - want| <= 2e-5 absref elementwise, absref = the same expression on absolute values (the sum of
  |terms|, tests/test_gpu_kernels.close); y - y0 is the difference of two stored sums, each within 2e-5 of y's absref, so it is
  held to y's absref too.

Routes: ``expected_route`` below is the table kind x dtype x rank x hook -> route, written from the conditions documented in
include/lora_amd.h and on the route constants and predicates of lora_amd/ops.py and lora_amd/_C.py.  The observed route is
``ops.PATH_LOG`` where the route logs itself, call spies on the ``_C`` launch wrappers and ``ops.lora_conv_branch`` elsewhere, and
for every primitive call ``_C.rank16_mfma_takes`` on the live tensors (VALU or matrix-core form).  A rank on a route the table
does not name fails even if its numbers are right.

Shapes that differ from a plain 1..64 walk, because the modules accept r <= min(in, out) only (lora.py:38-41, 89-92):
``conv3_nchw`` runs 16 -> 24 channels up to rank 16 (the native NCHW kernels) and 64 -> 64 channels above (the frozen conv +
``lora_conv_branch`` from an NCHW-contiguous input, in bf16 and in f32), ``lin_ring`` (64 -> 64, 4097 rows) walks 1..16 plus 17
and 64, and the past-the-limit ranks 65 and 68 of ``conv3_cl`` run on 128 -> 128 channels (the next C_in % 64 == 0).
"""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple

import pytest
import torch
import torch.nn.functional as F

import lora_amd as L
from lora_amd import _C, ops
from lora_amd import trainer as T
from oracle import torch_ref as TR
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

E16 = {"bf16": 2.0 ** -7, "f16": 2.0 ** -9}
K_F32 = 2e-5
GRAD16 = 4e-3
SCALE = 0.8
P_DROP = 0.1
SEED, OFF = 0x5EED0042, 991       # the dropout streams: call i of a forward to ops.next_dropout_stream gets (SEED, OFF + i)
LOW_TO_FROZEN = 1.5               # norm of the low-rank term over norm of the frozen term, in y and in dx
# The library route of a 3x3 site (frozen conv + ops.lora_conv_branch: channels-last ranks outside {4, 8, .., 64} and past 64,
# NCHW ranks above 16) in bf16 cannot meet three of the bounds above.  The route computes T with the library's convolution on
# ``lora_down`` ROUNDED to bf16 (ops.lora_conv_branch casts the factor to the activation dtype; the float64 restatement keeps
# the f32 factor), stores T in bf16, and hands that T to the backward.  Taken apart on MI355X (ranks 3, 35, 39 channels-last,
# 17, 35 NCHW), everything relative to max|T| resp. max|d lora_up|:
#   library T against the float64 convolution of the f32 factor            6.5e-3  5.5e-3  4.8e-3  4.7e-3  4.6e-3
#   library T against the float64 convolution of the bf16-ROUNDED factor   6.7e-3  5.2e-3  4.4e-3  4.3e-3  4.4e-3
#   one rounding to bf16 of that float64 T (what storing T costs)          1.6e-3  1.8e-3  2.2e-3  2.1e-3  2.2e-3
#   d lora_up restated in float64 from the library's T                     5.9e-3  4.6e-3  3.9e-3  4.6e-3  4.3e-3
#   d lora_up restated from bf16(float64 conv of the rounded factor)       2.3e-3  2.7e-3  2.2e-3  3.1e-3  2.4e-3
# i.e. rounding the factor and storing T in bf16 explain 2.2e-3 .. 3.1e-3 of d lora_up (inside 4e-3); the rest is the library
# convolution's own arithmetic, which no kernel of this project touches, and the restatement from the library's T reproduces
# the sweep's d lora_up error (5.939e-3 at rank 3).  Measured by the sweep on this route alone (it prints them), as multiples
# of the bounds above, worst rank of conv3_cl / conv3_cl_drop / conv3_nchw, identical with the matrix-core hook on and off (the
# route runs the library and the VALU kernels under both settings):
#     y       0.963 (rank 1)   1.016 (rank 1)   0.725 (rank 27)     x 2^-7
#     d down  1.005 (rank 45)  0.981 (rank 54)  0.987 (rank 51)     x 4e-3
#     d up    1.485 (rank 3)   1.315 (rank 3)   1.145 (rank 17)     x 4e-3
# f16 and f32 stay inside the bounds above on this route (f16: y 0.58, d down 0.62, d up 0.16 of them; f32: 0.002).
# Bound = the worst measured value + 10 % (the ladder rule); y - y0 and dx keep the bounds above (measured 0.972, 0.494 of them).
BRANCH_BF16 = {"y": 1.016 * 1.10 * 2.0 ** -7, "ddown": 1.005 * 1.10 * 4e-3, "dup": 1.485 * 1.10 * 4e-3}
QUANTITIES = ("y", "low", "dx", "ddown", "dup")

R64 = tuple(range(1, 65))
LIN_WS, LIN_LIB = ((2, 77), 320, 320), ((2, 77), 128, 192)
CONV3 = (2, 64, 64, 3, 12, 20)


class Kind(NamedTuple):
    site: str            # "lin": dims = (leading shape, K, N); "conv": dims = (B, C_in, C_out, ks, H, W)
    dims: tuple
    dtypes: tuple
    ranks: tuple
    p: float = 0.0       # > 0: train() with nn.Dropout(p) on the branch
    sel: bool = False    # set_selector_from_diag(linspace(0.5, 1.5, r))
    trainer: bool = False  # FlatLoraState + attach_direct_grads + enable_merged_weights; gradients read from flat_g
    half: bool = False   # module.half() (f16 factors too), eval, forward only
    cl: bool = True      # conv: channels-last input


KINDS = {
    "lin_ws": Kind("lin", LIN_WS, ("bf16", "f16"), R64),                       # M = 154, K in the weight-stationary set
    "lin_lib": Kind("lin", LIN_LIB, ("bf16", "f16", "f32"), R64 + (65, 96, 128)),  # library GEMM + linear_fwd / primitives
    "lin_ring": Kind("lin", ((4097,), 64, 64), ("bf16",), tuple(range(1, 17)) + (17, 64)),  # LDS ring from M >= 4096
    "lin_sel": Kind("lin", LIN_LIB, ("bf16", "f32"), R64, sel=True),
    "lin_drop@ws": Kind("lin", LIN_WS, ("bf16",), R64, p=P_DROP),
    "lin_drop@lib": Kind("lin", LIN_LIB, ("bf16",), R64 + (65, 96, 128), p=P_DROP),
    "lin_merged": Kind("lin", LIN_WS, ("bf16", "f16"), R64, trainer=True),
    "lin_drop_tr": Kind("lin", LIN_WS, ("bf16",), R64, p=P_DROP, trainer=True),
    "conv3_cl": Kind("conv", CONV3, ("bf16", "f16"), R64 + (65, 68)),         # W = 20: a masked 16-column pixel tile
    "conv3_cl_drop": Kind("conv", CONV3, ("bf16",), R64, p=P_DROP),
    "conv1_cl": Kind("conv", (2, 64, 96, 1, 12, 20), ("bf16",), R64),          # the Linear site on the pixel rows
    "conv3_nchw": Kind("conv", (2, 16, 24, 3, 6, 8), ("bf16", "f32"), R64, cl=False),   # r > 16: 64 -> 64 channels (dims_of)
    "half_infer@lin": Kind("lin", LIN_WS, ("f16",), R64, half=True),
    "half_infer@conv3": Kind("conv", CONV3, ("f16",), R64, half=True),
}
TESTS = [(kind, dt, hook) for kind, kd in KINDS.items() for dt in kd.dtypes for hook in (True, False)]
N_CASES = 2628   # (kind, dtype, hook, rank) cases of the sweep; tests/test_rank_sweep_cpu.py recounts it


def cases():
    for kind, dt, hook in TESTS:
        for r in KINDS[kind].ranks:
            yield kind, dt, hook, r


def dims_of(kind: str, r: int) -> tuple:
    kd = KINDS[kind]
    if kd.site == "conv" and r > min(kd.dims[1], kd.dims[2]):   # the module wants r <= min(in, out): the next channel count
        B, _, _, ks, Hh, Ww = kd.dims
        C = 64 if r <= 64 else 128
        return (B, C, C, ks, Hh, Ww)
    return kd.dims


# ----------------------------------------------------------------------------- the route table
WS_K = (320, 640, 768, 1280)                    # contraction lengths of the weight-stationary kernel (_C._WS_K)
CONV3_NARROW = (4, 8, 12, 16)                   # lora_amd_conv3_nhwc_plan: native ranks
CONV3_WIDE = tuple(range(20, 65, 4))            # lora_amd_conv3_nhwc_wide_plan: native ranks
NCHW_LAUNCHES = ("conv_down_fwd", "conv_up_fwd_", "conv_bwd_g", "conv_bwd_x")
SPIED = NCHW_LAUNCHES + ("linear_bwd_g", "linear_bwd_g_folded", "sum_parts", "linear_bwd_x", "conv3_nhwc_bwd_dx_",
                         "conv3_nhwc_bwd_down", "conv3_nhwc_wide_bwd_dx_", "conv3_nhwc_wide_bwd_down")


class Route(NamedTuple):
    log: tuple            # the (phase, path) entries of ops.PATH_LOG, in order
    launches: frozenset   # which of SPIED / "lora_conv_branch" ran
    prims: frozenset      # (primitive, columns of its row operand, rank of the call, "mfma" | "valu")


def _chunks(r: int):
    """ops._rank_chunks: ranks past LORA_AMD_MAX_RANK run as chunks of at most 64."""
    return [min(64, r - a) for a in range(0, r, 64)]


def _form(op: str, act: str, fac: str, cols: int, r: int, sel: bool, hook: bool) -> str:
    """include/lora_amd.h on lora_amd_rowdot / lora_amd_rank_update / lora_amd_colreduce: bf16 rows, 9 <= r <= 64, 16-byte
    aligned rows (every tensor of the sweep), and per primitive — rowdot: f32 factors, no selector, K % 32 == 0; rank_update:
    f32 factors, N % 8 == 0; colreduce: K % 32 == 0 — run the matrix-core form while lora_amd_rank16_mfma is on (colreduce:
    and lora_amd_colreduce_mfma, which the sweep leaves on); anything else the VALU kernel."""
    ok = hook and act == "bf16" and 9 <= r <= 64
    if op == "rowdot":
        ok = ok and fac == "f32" and not sel and cols % 32 == 0
    elif op == "rank_update":
        ok = ok and fac == "f32" and cols % 8 == 0
    else:
        ok = ok and cols % 32 == 0
    return "mfma" if ok else "valu"


def _prims(calls, act: str, fac: str, hook: bool) -> set:
    """``calls``: (primitive, columns, rank, selector) as the autograd layer issues them through the ``*_any`` wrappers."""
    return {(op, cols, c, _form(op, act, fac, cols, c, sel, hook)) for op, cols, r, sel in calls for c in _chunks(r)}


def _linear_route(M, K, N, act, fac, r, hook, sel=False, p=0.0, trainer=False, backward=True) -> Route:
    """ops.lora_linear on dense rows (and lora.LoraInjectedLinear._forward_merged in front of it)."""
    a16 = act in ("bf16", "f16")
    # lora_amd_linear_plan: the fused entry points take rank <= 16 with 16-byte lanes and row segments of >= 4 chunks
    fused_shape = r <= 16 and K % 32 == 0 and N % 32 == 0
    # lora_amd_factors_mfma_plan: 16-bit rows, N and K multiples of 32 (ranks 17..64 as rank-16 slices: ops.WIDE_*)
    pass_takes = a16 and fac == "f32" and not sel and K % 32 == 0 and N % 32 == 0 and r <= 64
    if trainer and p == 0.0 and pass_takes:
        # ops.merged_ok (maskless, frozen 16-bit weight in the compute dtype, f32 factors; MERGED_WIDE above rank 16) and
        # ops._merged_factor_grads under a trainer state: both factor gradients in the deferred matrix-core pass
        return Route((("fwd", "merged"), ("bwd", "merged_dx+factors_deferred_mfma")), frozenset(), frozenset())
    one_launch = a16 and fac == "f32" and not sel               # LoraLinearFunction.forward: the matrix-core GEMM kernels
    ws_ok = one_launch and K in WS_K and r <= 16 and N % 4 == 0  # _C.ws_supported
    ring_ok = one_launch and K % 64 == 0 and N >= 16 and N % 8 == 0 and r <= 16   # lora_amd_linear_gemm_fwd
    wide = N >= 4 * K
    # _C.static_fwd_choice: weight-stationary while a panel is amortised over few enough columns, the LDS ring for the wide
    # projections at K >= 640 and for K < 640 from 4096 rows, else the library GEMM
    if ws_ok and (K <= 320 or K == 768 or (not wide and (K == 640 or M <= 512))):
        tile = "ws"
    elif ring_ok and wide and K >= 640:
        tile = "ring24" if K == 640 else None
    elif ring_ok and K < 640 and M >= 4096:
        tile = "ring24" if wide else "ring22"
    else:
        tile = None
    if p > 0.0:   # WS_DROPOUT / WS_DROPOUT_WIDE: only the weight-stationary kernel regenerates the mask
        if tile != "ws" and ws_ok and not (K == 1280 and wide):
            tile = "ws"
        if tile != "ws" or N % 8:
            tile = None
    calls, launches = [], set()
    if tile:
        log = [("fwd", tile)]
    elif fused_shape:
        log = [("fwd", "lib+linear_fwd")]
    else:
        log = [("fwd", "lib+primitives")]
        calls.append(("rowdot", K, r, sel))
        if not (p > 0.0 and r > 64):
            calls.append(("rank_update", N, r, False))
    prims = _prims(calls, act, fac, hook)
    if not tile and not fused_shape and p > 0.0 and r > 64:
        prims.add(("rank_update", N, 1, "valu"))   # ops.rank_update_any_: the mask of the SUM over the chunks, drawn on f32 rows
    if not backward:
        return Route(tuple(log), frozenset(), frozenset(prims))
    calls = []
    deferred = trainer and pass_takes       # ops._deferred_plan: a trainer state that runs the pass, and the pass takes the site
    if fused_shape:
        # _C.static_bwd_choice (N = 320 / 640 from 2048 rows) and WS_DROPOUT_WIDE_BWD (from 256 rows)
        ws_g = one_launch and N in WS_K and K % 4 == 0
        if ws_g and ((N in (320, 640) and M >= 2048) or (p > 0.0 and M >= 256 and K % 8 == 0)):
            log.append(("bwd", "ws_dx+factors_deferred_mfma" if deferred else "ws_dx+factors"))
        elif deferred and r > 8:
            log.append(("bwd", "rowdot+lib+rank_update+factors_deferred_mfma"))
            calls += [("rowdot", N, r, False), ("rank_update", K, r, False)]
        else:
            log.append(("bwd", "g+lib+x"))
            launches |= {"linear_bwd_g", "linear_bwd_x"}
    elif deferred and 17 <= r <= 64:        # ops._wide_site_plan (WIDE_DROPOUT)
        log.append(("bwd", "rowdot+lib+rank_update+factors_deferred_mfma"))
        calls += [("rowdot", N, r, False), ("rank_update", K, r, False)]
    else:
        log.append(("bwd", "primitives"))
        calls += [("rowdot", N, r, sel), ("colreduce", N, r, False), ("colreduce", K, r, False), ("rank_update", K, r, False)]
    prims |= _prims(calls, act, fac, hook)
    return Route(tuple(log), frozenset(launches), frozenset(prims))


def _conv_route(kind, dt, r, hook) -> Route:
    """ops.lora_conv."""
    kd = KINDS[kind]
    B, Ci, Co, ks, Hh, Ww = dims_of(kind, r)
    fac = "f16" if kd.half else "f32"
    HW, M = Hh * Ww, B * Hh * Ww
    bwd = not kd.half
    if kd.cl and dt in ("bf16", "f16") and ks == 1:     # ops.conv_nhwc_ok: the Linear site on the [B*H*W, C] rows
        return _linear_route(M, Ci, Co, dt, fac, r, hook, kd.sel, kd.p, kd.trainer, bwd)
    nhwc = kd.cl and dt in ("bf16", "f16") and ks == 3 and Ci % 64 == 0 and Ww <= 128     # lora_amd_conv3_nhwc_plan
    if nhwc and r in CONV3_NARROW:
        # CONV3_FUSED: bf16 rows, C_out % 32 == 0, f32 factors handed over as they are (no selector in the conv kinds)
        fused = dt == "bf16" and Co % 32 == 0 and fac == "f32"
        if fused:
            log, prims = [("fwd", "conv3_nhwc_fused")], set()
        else:
            log = [("fwd", "conv3_nhwc_pack+down+update")]
            prims = _prims([("rank_update", Co, r, False)], dt, "f32", hook)   # up enters as an f32 copy
        if not bwd:
            return Route(tuple(log), frozenset(), frozenset(prims))
        # the G pass: lora_amd_linear_bwd_g_folded is the matrix-core form only (bf16 rows, f32 factors, rank 9..16, the hook
        # on) and needs the fused forward's counters; its documented other path is linear_bwd_g + sum_parts
        g_pass = {"linear_bwd_g_folded"} if (fused and 9 <= r <= 16 and hook) else {"linear_bwd_g", "sum_parts"}
        return Route(tuple(log), frozenset(g_pass | {"conv3_nhwc_bwd_dx_", "conv3_nhwc_bwd_down"}), frozenset(prims))
    if nhwc and r in CONV3_WIDE:            # ops.CONV3_WIDE: LoraConv3NhwcWideFunction
        prims = _prims([("rank_update", Co, r, False)], dt, "f32", hook)
        if not bwd:
            return Route((("fwd", "conv3_nhwc_wide"),), frozenset(), frozenset(prims))
        prims |= _prims([("rowdot", Co, r, False), ("colreduce", Co, r, False)], dt, "f32", hook)
        return Route((("fwd", "conv3_nhwc_wide"), ("bwd", "conv3_nhwc_wide")),
                     frozenset({"conv3_nhwc_wide_bwd_dx_", "conv3_nhwc_wide_bwd_down"}), frozenset(prims))
    # lora_amd_conv_plan: NCHW-contiguous, 1x1 or 3x3 "same", H*W % 8 == 0 (3x3: W % 8 == 0, W <= 512), rank <= 16
    if r <= 16 and HW % 8 == 0 and (ks == 1 or (Ww % 8 == 0 and Ww <= 512)):
        return Route((), frozenset(NCHW_LAUNCHES), frozenset())
    # frozen convolution + ops.lora_conv_branch: T from a library convolution in the ACTIVATION dtype, so the per-sample
    # primitives on the [C_out, H*W] planes see a 16-bit "factor" (T_b) or H*W columns — the VALU kernels either way here
    calls = [("rank_update", HW, r, False)]
    if bwd:
        calls += [("colreduce", HW, r, False), ("rowdot", HW, r, False)]
    return Route((), frozenset({"lora_conv_branch"}), frozenset(_prims(calls, dt, dt, hook)))


def expected_route(kind: str, dt: str, r: int, hook: bool) -> Route:
    kd = KINDS[kind]
    if r not in kd.ranks or dt not in kd.dtypes:
        raise KeyError((kind, dt, r))
    if kd.site == "conv":
        return _conv_route(kind, dt, r, hook)
    lead, K, N = kd.dims
    M = 1
    for d in lead:
        M *= d
    return _linear_route(M, K, N, dt, "f16" if kd.half else "f32", r, hook, kd.sel, kd.p, kd.trainer, not kd.half)


def mask_layout(kind: str, dt: str, r: int) -> str:
    """Element order of the dropout mask: "rows" = [M, N] row-major (Linear sites; the channels-last 3x3 kernels on the
    [B*H*W, C_out] pixel rows), "planes" = one draw per sample over its [C_out, H*W] planes (ops.lora_conv_branch: sample b
    is the forward's call b to the stream, so a backward that regenerated another sample's mask would show)."""
    if KINDS[kind].site == "lin":
        return "rows"
    return "planes" if "lora_conv_branch" in expected_route(kind, dt, r, True).launches else "rows"


# ----------------------------------------------------------------------------- inputs and the float64 restatement
def _randn(shape, *key):
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    return torch.randn(*shape, generator=g)


def _round(t, dt):
    return t.to(DT[dt]).double()


@functools.lru_cache(maxsize=4)
def _shared(kind: str, dt: str, dims: tuple) -> dict:
    """x, g, frozen weight and bias of a (kind, dtype): the same for every rank, rounded to the activation dtype."""
    kd = KINDS[kind]
    if kd.site == "lin":
        lead, K, N = dims
        xs, gs, ws, fan = lead + (K,), lead + (N,), (N, K), K
    else:
        B, Ci, Co, ks, Hh, Ww = dims
        xs, gs, ws, fan, N = (B, Ci, Hh, Ww), (B, Co, Hh, Ww), (Co, Ci, ks, ks), Ci * ks * ks, Co
    return dict(x=_round(_randn(xs, "x", dims), dt), g=_round(_randn(gs, "g", dims), dt),
                W=_round(_randn(ws, "w", dims) / fan ** 0.5, dt), b=_round(0.1 * _randn((N,), "b", dims), dt))


def inputs(kind: str, dt: str, r: int) -> dict:
    """float64 CPU tensors holding exactly the values the device sees."""
    kd, dims = KINDS[kind], dims_of(kind, r)
    out = dict(_shared(kind, dt, dims))
    if kd.site == "lin":
        _, K, N = dims
        ds, us, fan = (r, K), (N, r), K
    else:
        _, Ci, Co, ks, _, _ = dims
        ds, us, fan = (r, Ci, ks, ks), (Co, r, 1, 1), Ci * ks * ks
    down = _randn(ds, "down", dims, r) / fan ** 0.5
    up = _randn(us, "up", dims, r) * (LOW_TO_FROZEN / SCALE) / r ** 0.5
    fdt = "f16" if kd.half else "f32"
    out.update(down=_round(down, fdt), up=_round(up, fdt), diag=torch.linspace(0.5, 1.5, r).double() if kd.sel else None)
    return out


@functools.lru_cache(maxsize=4)
def _philox(numel: int, p: float, call: int = 0) -> torch.Tensor:
    return H.philox_dropout_mask(numel, p, SEED, OFF + call).double()


def _mask(kind, dt, r, gshape):
    kd = KINDS[kind]
    if kd.p == 0.0:
        return None
    if kd.site == "lin":
        return _philox(gshape.numel(), kd.p).view(gshape)
    B, Co, Hh, Ww = gshape
    if mask_layout(kind, dt, r) == "rows":
        return _philox(gshape.numel(), kd.p).view(B, Hh, Ww, Co).permute(0, 3, 1, 2)
    return torch.stack([_philox(Co * Hh * Ww, kd.p, b).view(Co, Hh, Ww) for b in range(B)])


def _restate(kind, v, mask, live):
    """The reference's op sequence (oracle/torch_ref) under autograd on ``live`` ranks -> y, y - frozen, dx, d down, d up."""
    kd = KINDS[kind]
    x = v["x"].clone().requires_grad_(True)
    down = v["down"][:live].clone().requires_grad_(True)
    up = v["up"][:, :live].clone().requires_grad_(True)
    diag = v["diag"][:live] if v["diag"] is not None else None
    if kd.site == "lin":
        y = TR.linear_adapter_forward(x, v["W"], v["b"], down, up, SCALE, selector=torch.diag(diag) if kd.sel else None,
                                      mask=mask)
        y0 = F.linear(v["x"], v["W"], v["b"])
    else:
        pad = (v["W"].shape[2] - 1) // 2
        sel = torch.diag(diag).reshape(live, live, 1, 1) if kd.sel else None
        y = TR.conv_adapter_forward(x, v["W"], v["b"], down, up, SCALE, 1, pad, 1, 1, selector=sel, mask=mask)
        y0 = F.conv2d(v["x"], v["W"], v["b"], 1, pad)
    (y * v["g"]).sum().backward()
    r = v["down"].shape[0]
    ddown, dup = torch.zeros_like(v["down"]), torch.zeros_like(v["up"])
    ddown[:live], dup[:, :live] = down.grad, up.grad
    assert ddown.shape[0] == r
    return dict(y=y.detach(), low=(y - y0).detach(), dx=x.grad, ddown=ddown, dup=dup)


def reference(kind: str, dt: str, r: int, drop_last: bool = False) -> dict:
    """The float64 restatement of one case; ``drop_last``: the same with the last rank removed (its gradient rows zero).
    f32 activations: with ``abs_*`` = the same expressions on absolute values (the sums of |terms|)."""
    v = inputs(kind, dt, r)
    mask = _mask(kind, dt, r, v["g"].shape)
    ref = _restate(kind, v, mask, r - 1 if drop_last else r)
    if dt == "f32":
        va = {k: (t.abs() if t is not None else None) for k, t in v.items()}
        for k, t in _restate(kind, va, mask, r).items():
            ref["abs_" + k] = t
    return ref


def on_library_conv_route(kind: str, dt: str, r: int) -> bool:
    return "lora_conv_branch" in expected_route(kind, dt, r, True).launches


def bounds(dt: str, ref: dict, library_conv: bool = False) -> dict:
    """Quantity -> the bound the sweep applies (a scalar for 16-bit activations, elementwise for f32).  ``library_conv``:
    the case runs the frozen conv + ``lora_conv_branch`` (BRANCH_BF16 in bf16)."""
    if dt == "f32":
        return dict(y=K_F32 * ref["abs_y"], low=K_F32 * ref["abs_y"], dx=K_F32 * ref["abs_dx"],
                    ddown=K_F32 * ref["abs_ddown"], dup=K_F32 * ref["abs_dup"])
    e = E16[dt]
    k = dict(y=e, low=e, dx=2 * e, ddown=GRAD16, dup=GRAD16)
    if library_conv and dt == "bf16":
        k.update(BRANCH_BF16)
    return {q: kq * ref[q].abs().max() for q, kq in k.items()}


def worst(got: torch.Tensor, want: torch.Tensor, bound) -> float:
    """max over the elements of |got - want| / bound: <= 1 passes."""
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got.double() - want).abs()
    if not torch.is_tensor(bound) or bound.dim() == 0:
        return float(err.max() / bound)
    assert bool((bound > 0).all())
    return float((err / bound).max())


_REFS = {}   # (kind, dtype) of the running test -> {rank: reference}: the two hook settings share it, then it is dropped


def cached_reference(kind, dt, r):
    if (kind, dt) not in _REFS:
        _REFS.clear()
        _REFS[(kind, dt)] = {}
    refs = _REFS[(kind, dt)]
    if r not in refs:
        refs[r] = reference(kind, dt, r)
    return refs[r]


# ----------------------------------------------------------------------------- the device side
class Spies:
    def __init__(self):
        self.launches, self.prims = set(), set()
        self.stream_calls = 0     # calls to ops.next_dropout_stream since the last clear()

    def next_dropout_stream(self, device):
        self.stream_calls += 1
        return SEED, OFF + self.stream_calls - 1

    def clear(self):
        self.launches.clear()
        self.prims.clear()
        self.stream_calls = 0


@pytest.fixture(autouse=True)
def hooks_restored():
    prev = (_C.rank16_mfma(-1), _C.colreduce_mfma(-1))
    yield
    _C.rank16_mfma(prev[0])
    _C.colreduce_mfma(prev[1])


@pytest.fixture
def spies(monkeypatch):
    """Which launch wrappers ran, and for every primitive call what ``_C.rank16_mfma_takes`` says on its live tensors."""
    s = Spies()

    def launch_spy(mod, name):
        inner = getattr(mod, name)

        def wrapper(*a, **k):
            s.launches.add(name)
            return inner(*a, **k)
        monkeypatch.setattr(mod, name, wrapper)

    for name in SPIED:
        launch_spy(_C, name)
    launch_spy(ops, "lora_conv_branch")
    rowdot, rank_update_, colreduce = _C.rowdot, _C.rank_update_, _C.colreduce

    def form(op, rows, r, fdt=torch.float32, has_sel=False):
        return "mfma" if _C.rank16_mfma_takes(op, rows, r, fdt, has_sel) else "valu"

    def spy_rowdot(x, factor, layout, scale=1.0, sel=None, *a, **k):
        r = factor.shape[0] if layout == _C.FACTOR_RK else factor.shape[1]
        s.prims.add(("rowdot", x.shape[1], r, form(0, x, r, factor.dtype, sel is not None)))
        return rowdot(x, factor, layout, scale, sel, *a, **k)

    def spy_rank_update(y, t, factor, *a, **k):
        s.prims.add(("rank_update", y.shape[1], t.shape[1], form(1, y, t.shape[1], factor.dtype)))
        return rank_update_(y, t, factor, *a, **k)

    def spy_colreduce(x, t, *a, **k):
        s.prims.add(("colreduce", x.shape[1], t.shape[1], form(2, x, t.shape[1])))
        return colreduce(x, t, *a, **k)

    monkeypatch.setattr(_C, "rowdot", spy_rowdot)
    monkeypatch.setattr(_C, "rank_update_", spy_rank_update)
    monkeypatch.setattr(_C, "colreduce", spy_colreduce)
    return s


def build_module(kind, dt, r, v):
    kd, dims = KINDS[kind], dims_of(kind, r)
    if kd.site == "lin":
        m = L.LoraInjectedLinear(dims[1], dims[2], True, r=r, dropout_p=kd.p, scale=SCALE)
    else:
        _, Ci, Co, ks, _, _ = dims
        m = L.LoraInjectedConv2d(Ci, Co, ks, 1, (ks - 1) // 2, r=r, dropout_p=kd.p, scale=SCALE)
    frozen = m._frozen()
    frozen.weight.data, frozen.bias.data = v["W"].float(), v["b"].float()
    m.lora_down.weight.data, m.lora_up.weight.data = v["down"].float(), v["up"].float()
    frozen.requires_grad_(False)
    if kd.sel:
        m.set_selector_from_diag(v["diag"].float())
    m.to(DEV)
    frozen.to(DT[dt])
    if kd.half:
        m.half()
    m.train(kd.p > 0.0)
    return m


def run_case(kind, dt, r, v, spies, log):
    """One module, forward (twice: ``lora_up`` zeroed, then as given) and backward -> the five quantities (float64, CPU) and
    the observed route of the second forward and the backward."""
    kd = KINDS[kind]
    m = build_module(kind, dt, r, v)
    st = mw = None
    if kd.trainer:
        st = T.FlatLoraState([{"params": [m.lora_up.weight, m.lora_down.weight], "lr": 1e-3}], device=torch.device(DEV))
        assert st.attach_direct_grads(m) == 1
        mw = st.enable_merged_weights(m)
    x = v["x"].to(DT[dt]).to(DEV)
    if kd.site == "conv" and kd.cl:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(not kd.half)
    up = m.lora_up.weight
    keep = up.detach().clone()
    with torch.no_grad():
        up.zero_()          # in place: the factor's version moves, the packs of the fused 3x3 forward are rebuilt
        if mw is not None:
            mw.refresh()
        y0 = m(x).detach().double().cpu()
        up.copy_(keep)
        if mw is not None:
            mw.refresh()
    spies.clear()
    del log[:]
    got = {}
    if kd.half:
        with torch.no_grad():
            y = m(x)
    else:
        y = m(x)
        (y.float() * v["g"].float().to(DEV)).sum().backward()
        if st is not None:
            st.reduce_pending()
            got["ddown"], got["dup"] = st.grad_view(m.lora_down.weight), st.grad_view(up)
        else:
            got["ddown"], got["dup"] = m.lora_down.weight.grad, up.grad
        got["dx"] = x.grad
    got["y"] = y
    got = {k: t.detach().double().cpu() for k, t in got.items()}
    got["low"] = got["y"] - y0
    seen = Route(tuple((ph, path) for ph, path, *_ in log), frozenset(spies.launches), frozenset(spies.prims))
    ranks_logged = {e[5] for e in log}
    assert ranks_logged <= {r}, (r, log)
    m.__dict__.pop("_grad_sink", None)
    m.__dict__.pop("_merged", None)
    return got, seen


RAN = {}   # (kind, dtype, hook) -> ranks that ran to the end of their comparison


@pytest.mark.parametrize("kind,dt,hook", TESTS, ids=[f"{k}-{d}-{'mfma' if h else 'valu'}" for k, d, h in TESTS])
def test_rank_sweep(kind, dt, hook, spies, monkeypatch):
    kd = KINDS[kind]
    log = []
    monkeypatch.setattr(ops, "PATH_LOG", log)
    monkeypatch.setattr(ops, "next_dropout_stream", spies.next_dropout_stream)
    _C.rank16_mfma(1 if hook else 0)
    _C.colreduce_mfma(1)
    assert _C.rank16_mfma(-1) == (1 if hook else 0)
    failures, peak = [], {q: (0.0, 0) for q in QUANTITIES}
    peak_lib = {q: (0.0, 0) for q in QUANTITIES}     # the library conv route alone, against the UNMEASURED bounds
    RAN[(kind, dt, hook)] = 0
    for r in kd.ranks:                       # ascending
        ref = cached_reference(kind, dt, r)
        try:
            got, seen = run_case(kind, dt, r, inputs(kind, dt, r), spies, log)
        except Exception as exc:             # nothing more is launched after a rank that raised
            if any(w in str(exc) for w in ("HIP error", "hipError", "illegal memory access")):
                pytest.exit(f"GPU fault at {kind} {dt} hook {'on' if hook else 'off'} rank {r}: {exc}", returncode=3)
            raise AssertionError(f"{kind} {dt} hook {'on' if hook else 'off'}: rank {r} raised {type(exc).__name__}: {exc}; "
                                 f"failures before it: {failures}") from exc
        lib = on_library_conv_route(kind, dt, r)
        bnd = bounds(dt, ref, lib)
        ratios = {q: worst(got[q], ref[q], bnd[q]) for q in QUANTITIES if q in got}
        if lib:
            plain = bounds(dt, ref)
            for q in ratios:
                v_ = worst(got[q], ref[q], plain[q])
                if v_ > peak_lib[q][0]:
                    peak_lib[q] = (v_, r)
        for q, v_ in ratios.items():
            if v_ > peak[q][0]:
                peak[q] = (v_, r)
        bad = {q: round(v_, 3) for q, v_ in ratios.items() if not v_ <= 1.0}
        want = expected_route(kind, dt, r, hook)
        if seen != want:
            bad["route"] = f"saw {tuple(seen)}, the table says {tuple(want)}"
        if bad:
            failures.append((r, bad))
        RAN[(kind, dt, hook)] += 1
    print(f"\n[rank sweep] {kind} {dt} hook {'on' if hook else 'off'}: worst error / bound (at rank) "
          + ", ".join(f"{q} {peak[q][0]:.3f} ({peak[q][1]})" for q in QUANTITIES if peak[q][1]))
    if any(v_[1] for v_ in peak_lib.values()):
        print(f"[rank sweep] {kind} {dt} hook {'on' if hook else 'off'}: frozen conv + lora_conv_branch alone, error / bound "
              "before BRANCH_BF16 (at rank) " + ", ".join(f"{q} {peak_lib[q][0]:.3f} ({peak_lib[q][1]})"
                                                         for q in QUANTITIES if peak_lib[q][1]))
    assert not failures, (f"{kind} {dt} hook {'on' if hook else 'off'}: {len(failures)} of {len(kd.ranks)} ranks fail "
                          f"(error / bound per quantity, > 1 fails): {failures}")


def test_the_sweep_ran_every_case(request):
    """No case is skipped: every selected sweep test walked all its ranks, and a full run makes N_CASES of them.
    Reads the module-global ``RAN``, so it wants the sweep tests to have run before it in the same process (pytest's default:
    file order, one process); under pytest-xdist or a reordering plugin it fails for reasons unrelated to the library."""
    selected = [it.callspec.params for it in request.session.items
                if getattr(it, "originalname", None) == "test_rank_sweep" and hasattr(it, "callspec")]
    want = {(p["kind"], p["dt"], p["hook"]): len(KINDS[p["kind"]].ranks) for p in selected}
    assert RAN == want, {k: (RAN.get(k), n_) for k, n_ in want.items() if RAN.get(k) != n_}
    if len(want) == len(TESTS):
        assert sum(RAN.values()) == N_CASES
