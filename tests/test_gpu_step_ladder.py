"""The timed step, boundary by boundary (BASELINE configs[1]: SD1.5 size, rank 4, batch 4, 512^2; the `bench` configuration of
tests/test_gpu_parity_r3.py: bf16, channels-last, head-padded and grouped projections, the hostops passes, merged weights).

The ladder.  Three runs of the same op sequence on the same values (``helpers.sd15_twins``, the inputs of the r3 fixture):
``f32`` (the oracle twin in f32), ``bf16 ref`` (the oracle twin under torch.autocast(bf16), the reference's own arithmetic;
both inside ``helpers.oracle_on_device``: library kernels only, MIOpen off) and ``dev`` (the device step, eager and replayed
from ``GraphedForwardBackward``).  At every boundary (conv_in, every ResnetBlock2D with its conv1 / conv2 / conv_shortcut,
every Transformer2DModel, Downsample2D, Upsample2D, mid_block, conv_out) the output activation and, where it requires grad, the
gradient that arrives at it are cloned into buffers that outlive the step (under capture the clones are graph nodes, so the
buffers hold the replayed values).  Per boundary, in logical NCHW order: ``e = |t - f32| / |f32|`` for dev and bf16 ref, their
ratio (the bracket rule on one tensor), and the signed part ``mean(t - f32) / mean|f32|``.

The transplant check takes the accumulated error out: for every convolution the device step's OWN input and arriving output
gradient (bf16, the strides they had) go through the same convolution in f64 with MIOpen off; the device's output and data
gradient are measured against that, beside the f64 result rounded to nearest bf16 (what a perfect bf16 convolution shows) and
ATen's native bf16 convolution on the same operands (the path the bf16-autocast oracle takes).

Two sessions: in the pytest process (MIOpen in immediate mode on an empty database) and in a child process on the benchmark's
Find picks (``bench.private_miopen_db``, ``cudnn.benchmark``, the naive solvers off, as bench.py sets them).  One eager step
under torch.profiler names the kernels each convolution geometry ran.

Every bound is one of three kinds: taken from the project (``D1_K``), computed in the test from the reference (``e_ref``, the
round-to-nearest tensor), or a measured ratio + 10 % with the measured value beside the constant.

WHAT THE LADDER SHOWS is written at ``FINDINGS`` below and in DESIGN.md section 6; the table is profiles/ladder.json.

Run as a script (``python tests/test_gpu_step_ladder.py [--seeded-db] [--no-aten]``) it prints one session's measurements as
one JSON line; ``--table FILE`` runs both sessions and writes the compact table (profiles/ladder.json).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

DEV = "cuda:0"
D1_K = 1e-4                 # taken from the project: the accumulation-order allowance, 1e-4 of the absolute bound
SKIP_REL = 1e-3             # helpers.bracket's rule: a tensor below 1e-3 of the largest norm of its kind is numerically nothing
MAX_SKIPPED = 0.05          # at most 5 % of the boundaries may be skipped
BOUNDARY_CLASSES = ("ResnetBlock2D", "Transformer2DModel", "Downsample2D", "Upsample2D")
RESNET_CONVS = ("conv1", "conv2", "conv_shortcut")


# ----------------------------------------------------------------------------- recording
class _FShim:
    """``torch.nn.functional`` as standin/unet.py sees it, with ``conv2d`` reported: ResnetBlock2D.forward calls F.conv2d
    directly for conv1 (the bias rides the time embedding), which no module hook sees.  The call itself is untouched."""

    def __init__(self, recorder):
        self._rec = recorder

    def __getattr__(self, name):
        return getattr(F, name)

    def conv2d(self, x, weight, bias=None, stride=1, padding=0, dilation=1, groups=1):
        out = F.conv2d(x, weight, bias, stride, padding, dilation, groups)
        name = self._rec.by_weight.get(weight.data_ptr())
        if name is not None:
            self._rec.on_conv(name, x, weight, bias, stride, padding, out)
        return out


class Recorder:
    """Hooks on one UNet2DConditionModel (either twin; module names match one to one).  ``acts`` / ``grads``: boundary name ->
    clone of the output / of the gradient arriving at it; ``order`` / ``gorder``: boundaries in forward / backward execution
    order; ``convs`` (``operands=True``): convolution name -> its input, output, arriving output gradient and data gradient as
    the step had them (clones keep the strides), from a hook on the convolution's own autograd node."""

    def __init__(self, unet, operands=False):
        self.unet, self.operands = unet, operands
        self.acts, self.grads, self.order, self.gorder, self.convs = {}, {}, [], [], {}
        self.by_weight, self._handles, self._F = {}, [], None
        self.boundaries = set()
        for name, m in unet.named_modules():
            if type(m).__name__ in BOUNDARY_CLASSES or name in ("conv_in", "conv_out", "mid_block"):
                self.boundaries.add(name)
            if type(m).__name__ == "ResnetBlock2D":
                self.boundaries.update(f"{name}.{c}" for c in RESNET_CONVS if getattr(m, c) is not None)
                self.by_weight[m.conv1.weight.data_ptr()] = f"{name}.conv1"

    def take(self):
        """The records so far (tensors stay alive with the returned dict); the recorder starts afresh."""
        out = dict(acts=self.acts, grads=self.grads, order=self.order, gorder=self.gorder, convs=self.convs)
        self.acts, self.grads, self.order, self.gorder, self.convs = {}, {}, [], [], {}
        return out

    # -- hooks
    def on_boundary(self, name, out):
        if name not in self.acts:
            self.order.append(name)
        self.acts[name] = out.detach().clone()
        if out.requires_grad:
            def hook(g, name=name):
                if name not in self.grads:
                    self.gorder.append(name)
                self.grads[name] = g.detach().clone()
            out.register_hook(hook)

    def on_conv(self, name, x, weight, bias, stride, padding, out):
        if name in self.boundaries:
            self.on_boundary(name, out)
        if not self.operands:
            return
        rec = dict(x=x.detach().clone(), y=out.detach().clone(), w=weight.detach(), b=None if bias is None else bias.detach(),
                   stride=tuple(stride) if not isinstance(stride, int) else (stride, stride),
                   padding=tuple(padding) if not isinstance(padding, int) else (padding, padding), go=None, gi=None,
                   node=type(out.grad_fn).__name__ if out.grad_fn is not None else None)
        self.convs[name] = rec
        if out.requires_grad and out.grad_fn is not None:
            def node_hook(grad_inputs, grad_outputs, rec=rec):
                rec["go"] = grad_outputs[0].detach().clone()
                if grad_inputs[0] is not None:
                    rec["gi"] = grad_inputs[0].detach().clone()
            out.grad_fn.register_hook(node_hook)

    def __enter__(self):
        import lora_amd.standin.unet as U

        for name, m in self.unet.named_modules():
            if isinstance(m, nn.Conv2d) and m.weight.data_ptr() not in self.by_weight:   # conv1: through the F shim
                self._handles.append(m.register_forward_hook(
                    lambda mod, inp, out, name=name: self.on_conv(name, inp[0], mod.weight, mod.bias, mod.stride, mod.padding,
                                                                  out)))
            elif name in self.boundaries and not isinstance(m, nn.Conv2d):
                self._handles.append(m.register_forward_hook(lambda mod, inp, out, name=name: self.on_boundary(name, out)))
        self._F, U.F = U.F, _FShim(self)
        return self

    def __exit__(self, *exc):
        import lora_amd.standin.unet as U

        U.F = self._F
        for h in self._handles:
            h.remove()
        self._handles = []


# ----------------------------------------------------------------------------- comparisons (arithmetic on recorded tensors)
def truncate_to_bf16(v64):
    """f64 -> bf16 by dropping the low 16 bits of the f32 value (toward zero): what a kernel stores when it converts
    its f32 accumulators without rounding."""
    bits = v64.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(torch.bfloat16)


def shrink_of(d, ref):
    """The part of an error ``d`` that lies along the values' own signs, ``sum(d sign(ref)) / sum|ref|``: rounding to
    nearest leaves 0, truncation toward zero about -2^-8 / E[mantissa] = -2.7e-3 in bf16, and unlike a random error it adds up
    linearly from layer to layer."""
    return float((d * torch.sign(ref)).sum() / ref.abs().sum())


def rel_and_bias(t, ref):
    """(|t - ref| / |ref|, mean(t - ref) / mean|ref|, shrink, finite) in f64, in logical index order whatever the strides."""
    t, ref = t.double(), ref.double()
    d = t - ref
    finite = bool(torch.isfinite(t).all())
    return float(d.norm() / ref.norm()), float(d.mean() / ref.abs().mean()), shrink_of(d, ref), finite


def ladder_rows(f32, bfr, dev):
    """One row per boundary and kind (activation in forward order, then gradient in backward order): the f32 norm, e_dev,
    e_ref, their ratio, the two signed parts, ``skipped`` by the 1e-3 rule.  ``dev`` may be None (the oracle-only check)."""
    rows = []
    for kind, key, order in (("act", "acts", f32["order"]), ("grad", "grads", f32["gorder"])):
        norms = {n_: float(f32[key][n_].double().norm()) for n_ in order}
        top = max(norms.values())
        for n_ in order:
            row = dict(name=n_, kind=kind, norm=norms[n_], skipped=norms[n_] < SKIP_REL * top)
            row["e_ref"], row["bias_ref"], row["shrink_ref"], _ = rel_and_bias(bfr[key][n_], f32[key][n_])
            if dev is not None:
                if n_ not in dev[key]:
                    row["missing"] = True
                else:
                    row["e_dev"], row["bias_dev"], row["shrink_dev"], row["finite"] = rel_and_bias(dev[key][n_], f32[key][n_])
                    row["ratio"] = row["e_dev"] / max(row["e_ref"], 1e-30)
            rows.append(row)
    return rows


def _measure_against(t, ref64, absref64, k=D1_K):
    """A bf16 tensor against the f64 result of the same operation: the norm error, the round-to-nearest tensor's, the
    accumulation-order allowance ``k |abs|``; the same three for the signed mean (relative to mean|f64|); and the shrink of
    the tensor, of the f64 result rounded to nearest and of the f64 result truncated."""
    d = t.double() - ref64
    rn = ref64.to(torch.bfloat16).double() - ref64
    tr = truncate_to_bf16(ref64).double() - ref64
    scale = float(ref64.abs().mean())
    return dict(err=float(d.norm()), e_rn=float(rn.norm()), allow=k * float(absref64.norm()), ref_norm=float(ref64.norm()),
                bias=float(d.mean()) / scale, bias_rn=float(rn.mean()) / scale, bias_allow=k * float(absref64.mean()) / scale,
                shrink=shrink_of(d, ref64), shrink_rn=shrink_of(rn, ref64), shrink_trunc=shrink_of(tr, ref64),
                cos=float((d * ref64).sum() / (d.norm() * ref64.norm() + 1e-300)), finite=bool(torch.isfinite(t).all()))


def transplant_ok(m, factor):
    """The transplant bound: |dev - f64| <= factor |rn - f64| + 1e-4 | |x| (*) |w| |, and the same for the signed mean."""
    return (m["finite"] and m["err"] <= factor * m["e_rn"] + m["allow"]
            and abs(m["bias"]) <= factor * abs(m["bias_rn"]) + m["bias_allow"])


def transplant_excess(m):
    """What ``factor`` a measurement needs: (norm, bias), each (value - allowance) / round-to-nearest's."""
    return ((m["err"] - m["allow"]) / max(m["e_rn"], 1e-300),
            (abs(m["bias"]) - m["bias_allow"]) / max(abs(m["bias_rn"]), 1e-300))


def conv_reference(c, with_aten=True):
    """f64 forward and data gradient of one convolution from the recorded operands (MIOpen off, ATen's native path), the
    same on absolute values, and ATen's native bf16 results (the bf16-autocast oracle's path)."""
    prev = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        x, w, b, st, pd = c["x"], c["w"], c["b"], c["stride"], c["padding"]
        x64, w64 = x.double().contiguous(), w.double().contiguous()
        b64 = None if b is None else b.double()
        out = dict(y64=F.conv2d(x64, w64, b64, st, pd),
                   yabs=F.conv2d(x64.abs(), w64.abs(), None if b64 is None else b64.abs(), st, pd))
        if with_aten:
            out["y_aten"] = F.conv2d(x, w, b, st, pd)
        if c.get("go") is not None and c.get("gi") is not None:
            go64 = c["go"].double().contiguous()
            out["gi64"] = torch.nn.grad.conv2d_input(x.shape, w64, go64, st, pd)
            out["giabs"] = torch.nn.grad.conv2d_input(x.shape, w64.abs(), go64.abs(), st, pd)
            if with_aten:
                out["gi_aten"] = torch.nn.grad.conv2d_input(x.shape, w, c["go"], st, pd)
        return out
    finally:
        torch.backends.cudnn.enabled = prev


def geometry(c):
    return "x%s w%s s%d" % ("x".join(map(str, c["x"].shape)), "x".join(map(str, c["w"].shape)), c["stride"][0])


def transplant_rows(convs, with_aten=True):
    rows = []
    for name, c in convs.items():
        r = conv_reference(c, with_aten)
        row = dict(name=name, geometry=geometry(c), node=c["node"], x_strides=list(c["x"].stride()),
                   fwd=_measure_against(c["y"], r["y64"], r["yabs"]))
        if with_aten:
            row["fwd_aten"] = _measure_against(r["y_aten"], r["y64"], r["yabs"])
        if "gi64" in r:
            row["bwd"] = _measure_against(c["gi"], r["gi64"], r["giabs"])
            if with_aten:
                row["bwd_aten"] = _measure_against(r["gi_aten"], r["gi64"], r["giabs"])
        rows.append(row)
        del r
    return rows


# ----------------------------------------------------------------------------- the runs
def inputs(dev=DEV, B=4, hw=64, ctx=768):
    """The inputs of the r3 fixture ``sd15_reference_step`` (seed 123, batch 4), bf16-representable, as f32 on ``dev``."""
    g = torch.Generator().manual_seed(123)
    lat = torch.randn(B, 4, hw, hw, generator=g) * 0.18215
    ehs = torch.randn(B, 77, ctx, generator=g)
    noise = torch.randn(B, 4, hw, hw, generator=g)
    ts = torch.randint(0, 1000, (B,), generator=g)
    lat, ehs, noise = (v.to(torch.bfloat16).float().to(dev) for v in (lat, ehs, noise))
    return dict(lat=lat, ehs=ehs, noise=noise, ts=ts.to(dev))


def oracle_runs(ref, ref_params, inp):
    """The f32 and the bf16-autocast run of the oracle twin, recorded (as f32 / as computed); -> (f32, bf16 ref)."""
    from tests import helpers as H

    runs = []
    with H.oracle_on_device():
        for autocast in (False, True):
            rec = Recorder(ref)
            with rec:
                _, loss, _ = H.oracle_step_on_device(ref, ref_params, inp["lat"], inp["noise"], inp["ts"], inp["ehs"], autocast)
            r = rec.take()
            r["loss"] = loss
            runs.append(r)
    return runs


def device_step(unet, inp, fmt=torch.channels_last):
    """The `bench` configuration's step on ``unet`` (the caller has set LORA_AMD_HEAD_PAD / GROUP_QKV / fused._ENABLED):
    channels-last, merged weights; -> (fwd_bwd, st, lat, ehs)."""
    from lora_amd import trainer as T
    from lora_amd.standin import DDPMScheduler

    dev = inp["lat"].device
    unet.to(memory_format=fmt)
    st = T.FlatLoraState([{"params": T.lora_params(unet), "lr": 1e-4, "weight_decay": 1e-2}], max_grad_norm=1.0, device=dev)
    st.attach_direct_grads(unet)
    merged = st.enable_merged_weights(unet)
    sched = DDPMScheduler()
    lat = inp["lat"].to(torch.bfloat16).contiguous(memory_format=fmt)
    noise = inp["noise"].to(torch.bfloat16).contiguous(memory_format=fmt)
    ehs, ts = inp["ehs"].to(torch.bfloat16), inp["ts"]

    def fwd_bwd(l_, c_):
        return T.forward_backward(unet, sched, l_, c_, T.StepConfig(), noise=noise, timesteps=ts, merged=merged)

    return fwd_bwd, st, lat, ehs


def conv_kernels(step_fn):
    """One eager step under torch.profiler: convolution geometry (forward ``fwd x.. w..`` / backward ``bwd x.. w..``) -> the
    device kernels launched inside that convolution call."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], record_shapes=True) as prof:
        step_fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.events():
        kernels = getattr(ev, "kernels", None)
        if not kernels or "conv" not in ev.name.lower():
            continue
        top, e = None, ev
        while e is not None:
            if e.name in ("aten::convolution_backward", "aten::_convolution", "aten::convolution"):
                top = e
                break
            e = getattr(e, "cpu_parent", None)
        if top is None:
            continue
        shapes = [s for s in (top.input_shapes or []) if isinstance(s, (list, tuple)) and len(s) == 4]
        bwd = top.name == "aten::convolution_backward"
        if len(shapes) < (3 if bwd else 2):
            continue
        concrete = list(getattr(top, "concrete_inputs", None) or [])
        stride = concrete[4 if bwd else 3] if len(concrete) > 4 else None    # (grad, x, w, bias sizes, stride | x, w, b, stride
        stride = " s%d" % stride[0] if isinstance(stride, (list, tuple)) and stride else ""
        x_, w_ = shapes[1 if bwd else 0], shapes[2 if bwd else 1]
        key = "%s x%s w%s%s" % ("bwd" if bwd else "fwd", "x".join(map(str, x_)), "x".join(map(str, w_)), stride)
        names = out.setdefault(key, [])
        for k in kernels:
            if k.name[:160] not in names:
                names.append(k.name[:160])
    return out


def measure(seeded=False, with_aten=True, keep=None):
    """Both ladders (eager, replay), the transplant rows on the replayed step's operands and the kernels per geometry.
    The caller has put the process into the `bench` configuration's environment.  ``keep``: a convolution whose recorded
    operands are returned too (``_keep``: tensors, for the negative test)."""
    from lora_amd import trainer as T
    from tests import helpers as H

    ref, ref_params, unet = H.sd15_twins()
    inp = inputs()
    f32, bfr = oracle_runs(ref, ref_params, inp)
    del ref, ref_params
    torch.cuda.empty_cache()
    oracle_rows = ladder_rows(f32, bfr, None)
    fwd_bwd, st, lat, ehs = device_step(unet, inp)
    try:
        for _ in range(2):      # attention choices are timed on first use; the padded layout applies from the second call
            fwd_bwd(lat, ehs)
            st.zero_grad()
        rec = Recorder(unet, operands=True)
        with rec:
            loss_e = float(fwd_bwd(lat, ehs))
            st.reduce_pending()
            torch.cuda.synchronize()
            eager = rec.take()
            st.zero_grad()
        rows_eager = ladder_rows(f32, bfr, eager)
        del eager

        def one():
            fwd_bwd(lat, ehs)
            st.reduce_pending()

        kernels = conv_kernels(one)
        st.zero_grad()
        with rec:
            graphed = T.GraphedForwardBackward(fwd_bwd, lat, ehs, st)
            st.zero_grad()
            loss_r = float(graphed(lat, ehs))
            torch.cuda.synchronize()
        replay = rec.take()
        rows_replay = ladder_rows(f32, bfr, replay)
        trows = transplant_rows(replay["convs"], with_aten)
        kept = replay["convs"].get(keep)
        for row in trows:
            g = row["geometry"]
            row["kernels_fwd"] = kernels.get("fwd " + g) or kernels.get("fwd " + g.rsplit(" s", 1)[0], [])
            row["kernels_bwd"] = kernels.get("bwd " + g) or kernels.get("bwd " + g.rsplit(" s", 1)[0], [])
    finally:
        for m in unet.modules():
            m.__dict__.pop("_grad_sink", None)
            m.__dict__.pop("_merged", None)
    return dict(seeded_db=bool(seeded and os.environ.get("MIOPEN_USER_DB_PATH")), loss_f32=f32["loss"], loss_ref=bfr["loss"],
                loss_eager=loss_e, loss_replay=loss_r, oracle=oracle_rows, eager=rows_eager, replay=rows_replay,
                transplant=trows, kernels=kernels, **({"_keep": kept} if kept is not None else {}))


# ----------------------------------------------------------------------------- bounds
# The ladder's c: the worst ratio e_dev / e_ref measured in the EMPTY-database session (two runs, eager and replayed) + 10 %.
#   activations: 1.575 at conv_in (next: 1.307 down_blocks.0.resnets.0.conv1, 1.111 up_blocks.3.resnets.2.conv_shortcut; every
#   other boundary <= 1.11, median 0.96).  The three that stand out are direct outputs of the truncating forward kernels of
#   FINDINGS (2 x the rounding error of the reference's convolution); the GroupNorm behind each removes the common shrink.
#   gradients: 0.997 / 1.002 / 1.000 / 0.999 (median 0.99).
LADDER_C_ACT = 1.73         # measured 1.575, + 10 %
LADDER_C_GRAD = 1.10        # measured 1.002, + 10 %
# The floor of the signed part, |bias_dev| <= c |bias_ref| + floor: the worst measured excess |bias_dev| - c |bias_ref| in the
# empty-database session, 4.6e-4 / 6.5e-4 / 7.1e-4 / 7.7e-4 (activations, always conv_out: 65 K elements) and 4.1e-4 .. 5.5e-4
# (gradients, conv_out), + 10 %.
LADDER_BIAS_FLOOR = 8.5e-4  # measured 7.7e-4, + 10 %
# The transplant factor: the issue's starting point 2.  Checked against the reference's own bf16 convolution (ATen's native
# path, MIOpen off) on the step's operands: it needs 0.77 (forward) and 1.18 (data gradient: col2im sums nine taps in bf16,
# |err| = 1.43 |rn err| before the allowance) of the factor, so 2 stands
# (test_reference_convolution_meets_the_transplant_bound).
TRANSPLANT_FACTOR = 2.0

FINDINGS = """
Measured on an MI355X (profiles/ladder.json; three runs; the full account is DESIGN.md section 6, "Known issue, located"):

* Which convolutions round is a property of the KERNEL.  The assembly implicit-GEMM NHWC kernels
  `igemm_{fwd,bwd}_gtcx35_nhwc_bf16_*` WITHOUT the `_gkgs` suffix (ConvAsmImplicitGemmGTCDynamic{Fwd,Bwd}XdlopsNHWC) store their
  f32 accumulators to bf16 truncated: |dev - f64| = 2.00 x |rn(f64) - f64|, shrink -2.8e-3, on every one.  The `_gkgs` variants
  and the composable-kernel solvers round to nearest (1.00 x, shrink 1e-6).  No exception either way.
* The issue's transplant bound cannot see this (its allowance is 0.2-4.7 x the rounding error at these K, so a truncating
  store needs 1.76 of the factor 2); the shrink can.
* Benchmark's picks: every forward convolution rounds, 29-31 of the 63 data gradients truncate.  The gradient's shrink grows
  by 2.8e-3 per truncating convolution on the path, to -4.5e-2 at down_blocks.0; e_dev / e_ref goes 0.95 at conv_out, leaves
  c = 1.10 at up_blocks.3.attentions.0 (1.11), 2.15-2.28 at mid_block.  Activations: every ratio <= 1.00.
* Empty database: 15-19 forward convolutions and 13-14 data gradients truncate; the GroupNorm behind a truncated forward output
  enlarges the gradient by what the truncated data gradient takes away, and every gradient ratio stays within 0.97-1.00.
* Picks moved between runs in both sessions, so the tests key on the kernel that ran, never on a list of geometries.
"""
ASM_FAMILY = "ConvAsmImplicitGemmGTCDynamic{Fwd,Bwd}XdlopsNHWC (kernels igemm_*_gtcx35_nhwc_bf16_* without the _gkgs split)"


def ran_on_truncating_family(kernels):
    return any(k.startswith("igemm_") and "_nhwc_bf16_" in k and not k.endswith("_gkgs") for k in kernels)


def rounds_to_nearest(m):
    """Computed from the reference alone: the tensor's shrink lies nearer to that of the f64 result rounded to nearest than
    to that of the f64 result truncated toward zero (the two are three decades apart, 1e-6 against 2.8e-3)."""
    return m["finite"] and abs(m["shrink"] - m["shrink_rn"]) < abs(m["shrink"] - m["shrink_trunc"])


def ladder_failures(rows, kinds=("act", "grad")):
    """Boundaries in execution order (forward, then backward) that leave the ladder's bounds; -> [(name, kind, what)]."""
    bad = []
    for r in rows:
        if r["kind"] not in kinds or r["skipped"]:
            continue
        c = LADDER_C_ACT if r["kind"] == "act" else LADDER_C_GRAD
        if r.get("missing") or not r["finite"]:
            bad.append((r["name"], r["kind"], "missing" if r.get("missing") else "not finite"))
        elif r["e_dev"] > c * r["e_ref"]:
            bad.append((r["name"], r["kind"], "e_dev %.3e = %.3f x e_ref (c = %.2f)" % (r["e_dev"], r["ratio"], c)))
        elif abs(r["bias_dev"]) > c * abs(r["bias_ref"]) + LADDER_BIAS_FLOOR:
            bad.append((r["name"], r["kind"], "bias %.3e against the reference's %.3e" % (r["bias_dev"], r["bias_ref"])))
    return bad


def transplant_failures(trows, keys=("fwd", "bwd")):
    return [(r["name"], k, r["geometry"], transplant_excess(r[k])) for r in trows for k in keys
            if k in r and not transplant_ok(r[k], TRANSPLANT_FACTOR)]


def table_json(empty, picks):
    """Both sessions' measurements as the compact table kept under profiles/: one row per boundary (replayed step; the
    reference's columns once, they are the same in both sessions) and per convolution, three significant digits."""
    def g(v):
        return float("%.3g" % v)

    both = (empty, picks)
    names = sorted({k for r in both for x in r["transplant"] for d in ("fwd", "bwd") for k in x["kernels_" + d]})
    rows = []
    for x, y in zip(empty["replay"], picks["replay"]):
        assert (x["name"], x["kind"]) == (y["name"], y["kind"])
        rows.append([x["name"], x["kind"], g(x["e_ref"]), g(x["bias_ref"]), g(x["shrink_ref"])]
                    + [g(z[k]) for z in (x, y) for k in ("ratio", "bias_dev", "shrink_dev")])
    convs = []
    for x, y in zip(empty["transplant"], picks["transplant"]):
        row = [x["name"], x["geometry"]]
        for d in ("fwd", "bwd"):
            for z in (x, y):
                m = z.get(d)
                row += [None, None] if m is None else [g(m["err"] / m["e_rn"]), [names.index(k) for k in z["kernels_" + d]]]
        convs.append(row)
    head = dict(losses={k: [r[k] for r in both] for k in ("loss_f32", "loss_ref", "loss_eager", "loss_replay")},
                boundary_columns="name kind e_ref bias_ref shrink_ref ratio_empty bias_dev_empty shrink_dev_empty ratio_picks "
                                 "bias_dev_picks shrink_dev_picks".split(),
                convolution_columns="name geometry fwd_err_over_rn_empty fwd_kernels_empty fwd_err_over_rn_picks "
                                    "fwd_kernels_picks bwd_err_over_rn_empty bwd_kernels_empty bwd_err_over_rn_picks "
                                    "bwd_kernels_picks".split())
    parts = [json.dumps(head)[1:-1]]
    for key, items in (("boundaries", rows), ("convolutions", convs), ("kernels", names)):
        parts.append('"%s": [\n%s\n]' % (key, ",\n".join(json.dumps(i) for i in items)))
    return "{" + ",\n".join(parts) + "}\n"


def _child(*flags):
    """The measurement in a fresh child process (never exec) without MIOPEN_USER_DB_PATH; -> its JSON line, parsed."""
    env = {k: v for k, v in os.environ.items() if k != "MIOPEN_USER_DB_PATH"}
    p = subprocess.run([sys.executable, os.path.abspath(__file__), *flags], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])


# ----------------------------------------------------------------------------- sessions
def _bench_configuration():
    os.environ["LORA_AMD_HEAD_PAD"] = "1"
    os.environ["LORA_AMD_GROUP_QKV"] = "1"
    from lora_amd.standin import fused
    fused._ENABLED = True


def _main(argv):
    if "--table" in argv:       # both sessions, each in a child of its own, as one table
        with open(argv[argv.index("--table") + 1], "w") as f:
            f.write(table_json(_child("--no-aten"), _child("--seeded-db", "--no-aten")))
        return
    seeded = "--seeded-db" in argv
    if seeded:      # what bench.py sets around its step, before the first convolution
        import bench
        bench.private_miopen_db()
        torch.backends.cudnn.benchmark = True
        for k in ("FWD", "BWD", "WRW"):
            os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_" + k, "0")
    _bench_configuration()
    print(json.dumps(measure(seeded, with_aten="--no-aten" not in argv)), flush=True)


# ----------------------------------------------------------------------------- tests
NEGATIVE_CONV = "down_blocks.2.resnets.1.conv2"     # 1280 -> 1280, 3x3 at 16^2: rounds to nearest in both sessions


@pytest.fixture(scope="module")
def empty_session():
    """The measurement in the pytest process: MIOpen in immediate mode on whatever database the session has (empty in the
    suite's runs)."""
    from lora_amd.standin import fused

    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("LORA_AMD_HEAD_PAD", "1")
        mp.setenv("LORA_AMD_GROUP_QKV", "1")
        mp.setattr(fused, "_ENABLED", True)
        r = measure(False, keep=NEGATIVE_CONV)
    yield r
    r.pop("_keep", None)
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def seeded_session():
    """The same measurement in a child process (never exec) on the benchmark's picks: MIOPEN_USER_DB_PATH removed, the
    child calls bench.private_miopen_db() and sets what bench.py sets before its first convolution."""
    return _child("--seeded-db", "--no-aten")


def _summary(r, label):
    for mode in ("eager", "replay"):
        for kind in ("act", "grad"):
            rows = [x for x in r[mode] if x["kind"] == kind and not x["skipped"] and "ratio" in x]
            w = max(rows, key=lambda x: x["ratio"])
            c = LADDER_C_ACT if kind == "act" else LADDER_C_GRAD
            print(f"[ladder {label} {mode} {kind}] worst ratio {w['ratio']:.3f} at {w['name']}; worst |shrink| "
                  f"{max(abs(x['shrink_dev']) for x in rows):.2e} (reference {max(abs(x['shrink_ref']) for x in rows):.2e}); "
                  f"worst bias excess {max(abs(x['bias_dev']) - c * abs(x['bias_ref']) for x in rows):.2e}")
    for k in ("fwd", "bwd", "fwd_aten", "bwd_aten"):
        xs = [transplant_excess(x[k]) for x in r["transplant"] if k in x]
        if xs:
            print(f"[transplant {label} {k}] needs {max(a for a, _ in xs):.3f} of the factor (norm), "
                  f"{sum(not rounds_to_nearest(x[k]) for x in r['transplant'] if k in x)} of {len(xs)} truncate")


@pytest.mark.gpu
def test_oracle_boundaries_are_measurable(empty_session):
    """On the oracle alone: at most 5 % of the boundaries are numerically nothing (below 1e-3 of the largest norm of their
    kind) at these inputs; all 105 activations and 101 gradients are there."""
    rows = empty_session["oracle"]
    assert sum(x["kind"] == "act" for x in rows) == 105 and sum(x["kind"] == "grad" for x in rows) == 101
    assert sum(x["skipped"] for x in rows) <= MAX_SKIPPED * len(rows), [x["name"] for x in rows if x["skipped"]]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["eager", "replay"])
def test_ladder_on_the_empty_database(empty_session, mode):
    """Every boundary, activation and gradient: finite, e_dev <= c e_ref, |bias_dev| <= c |bias_ref| + floor."""
    _summary(empty_session, "empty db")
    assert not ladder_failures(empty_session[mode]), ladder_failures(empty_session[mode])[:6]


@pytest.mark.gpu
@pytest.mark.parametrize("session", ["empty", "seeded"])
def test_transplant_bound_on_the_steps_operands(empty_session, seeded_session, session):
    """The issue's bound, every convolution, forward and data gradient, on the replayed step's own operands:
    |dev - f64| <= 2 |rn - f64| + 1e-4 | |x| (*) |w| |, and the signed mean likewise."""
    r = empty_session if session == "empty" else seeded_session
    assert len(r["transplant"]) == 66 and sum("bwd" in x for x in r["transplant"]) == 63
    assert all(x["node"] in (None, "ConvolutionBackward0") for x in r["transplant"])
    assert not transplant_failures(r["transplant"]), transplant_failures(r["transplant"])[:6]


@pytest.mark.gpu
def test_reference_convolution_meets_the_transplant_bound(empty_session):
    """What sizes TRANSPLANT_FACTOR: ATen's native bf16 convolution (MIOpen off), the path of the bf16-autocast oracle, on the
    same operands meets the bound with the factor 2, and rounds to nearest by the shrink rule."""
    t = empty_session["transplant"]
    assert not transplant_failures(t, ("fwd_aten", "bwd_aten")), transplant_failures(t, ("fwd_aten", "bwd_aten"))[:6]
    assert all(rounds_to_nearest(x[k]) for x in t for k in ("fwd_aten", "bwd_aten") if k in x)


@pytest.mark.gpu
@pytest.mark.parametrize("session", ["empty", "seeded"])
def test_every_convolution_off_the_truncating_kernels_rounds_to_nearest(empty_session, seeded_session, session):
    """Keyed by the kernel that ran (one eager step under torch.profiler): every convolution, forward and data gradient, that
    did not run on the assembly implicit-GEMM NHWC kernels of FINDINGS rounds its output to nearest."""
    r = empty_session if session == "empty" else seeded_session
    checked = 0
    for x in r["transplant"]:
        for k in ("fwd", "bwd"):
            if k in x:
                assert x["kernels_" + k], (x["name"], k, "no kernel recorded")
                if not ran_on_truncating_family(x["kernels_" + k]):
                    checked += 1
                    assert rounds_to_nearest(x[k]), (x["name"], k, x["geometry"], x["kernels_" + k], x[k])
    assert checked >= 60, checked       # measured: 96-101 (empty), 98-100 (seeded) of 129
    for k in (("fwd", "bwd") if session == "empty" else ("bwd",)):      # the expected failure's cases below are not vacuous
        assert any(ran_on_truncating_family(x["kernels_" + k]) for x in r["transplant"] if k in x), k


@pytest.mark.gpu
@pytest.mark.parametrize("session,direction", [("empty", "fwd"), ("empty", "bwd"), ("seeded", "bwd")])
@pytest.mark.xfail(strict=True, raises=AssertionError,
                   reason="library solver " + ASM_FAMILY + " stores its f32 accumulators to bf16 truncated toward zero (|err| "
                   "= 2.00 x round-to-nearest's, shrink -2.8e-3).  Measured geometries (x, w, stride): empty database fwd "
                   "4->320, "
                   "320->320, 640->640, 960->320 (3x3, 1x1), 640->320 (3x3, 1x1) at 64^2; empty database bwd 320->320 s1/s2, "
                   "640->640, 640->320 (3x3, 1x1), 320->4 at 64^2, 640->640 s2 at 32^2; benchmark's picks bwd: those and "
                   "960->320 (3x3, 1x1) at 64^2, 1920/1280/960->640 (3x3, 1x1) at 32^2, the 1x1 shortcuts 320->640, 640->1280, "
                   "2560->1280, 1920->1280")
def test_convolutions_on_the_assembly_implicit_gemm_kernels_round_to_nearest(empty_session, seeded_session, session,
                                                                             direction):
    """Turns red (XPASS, strict) the day the library's kernels round: then drop this mark and the family exception above."""
    r = empty_session if session == "empty" else seeded_session
    on_family = [x for x in r["transplant"] if direction in x and ran_on_truncating_family(x["kernels_" + direction])]
    assert all(rounds_to_nearest(x[direction]) for x in on_family)    # (that the family ran at all: the test above)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["eager", "replay"])
def test_ladder_activations_on_the_benchmarks_picks(seeded_session, mode):
    """The forward side of the timed configuration holds the empty-database bounds (every ratio <= 1.00 measured)."""
    _summary(seeded_session, "bench picks")
    assert seeded_session["seeded_db"], "the child did not run on the seeded database"
    assert not ladder_failures(seeded_session[mode], ("act",)), ladder_failures(seeded_session[mode], ("act",))[:6]
    assert all(x["finite"] and not x.get("missing") for x in seeded_session[mode])


@pytest.mark.gpu
@pytest.mark.xfail(strict=True, raises=AssertionError,
                   reason="benchmark's picks: the data gradients of " + ASM_FAMILY + " are truncated; the gradient ladder "
                   "leaves c = 1.10 at up_blocks.3.attentions.0 / up_blocks.3.resnets.0 (1.11, shrink -1.1e-2; first truncated:"
                   " "
                   "up_blocks.3.resnets.2's conv2 / conv_shortcut, igemm_bwd_gtcx35_nhwc_bf16_*_bt64x128x32_*_mh and "
                   "*_ex0_bt128x128x32_*) and grows to 2.15-2.28 at mid_block (shrink -4.1e-2)")
def test_ladder_gradients_on_the_benchmarks_picks(seeded_session):
    bad = ladder_failures(seeded_session["replay"], ("grad",))
    assert not bad, bad[:3]


@pytest.mark.gpu
def test_where_the_error_enters_on_the_benchmarks_picks(seeded_session):
    """The named location, asserted as far as it is stable: no activation leaves the bounds; the first gradient boundary that
    does lies in up_blocks.3 or up_blocks.2 (backward order: the first blocks behind conv_out), downstream of at least one
    convolution whose data gradient ran on the truncating family; from there the gradient's shrink is negative and at
    mid_block beyond ten times the reference's."""
    r = seeded_session
    bad = ladder_failures(r["replay"])
    assert bad and bad[0][1] == "grad", bad[:3]
    first = bad[0][0]
    print("[ladder bench picks] first boundary outside the bounds:", bad[0])
    assert first.startswith(("up_blocks.3", "up_blocks.2")), bad[0]
    order = [x["name"] for x in r["replay"] if x["kind"] == "grad"]
    upstream = set(order[:order.index(first) + 1])
    trunc = [x["name"] for x in r["transplant"] if "bwd" in x and not rounds_to_nearest(x["bwd"])]
    assert any(n_ in upstream or n_.rsplit(".", 1)[0] in upstream for n_ in trunc), (first, trunc[:4])
    assert all(ran_on_truncating_family(x["kernels_bwd"]) for x in r["transplant"] if x["name"] in trunc)
    mid = next(x for x in r["replay"] if x["kind"] == "grad" and x["name"] == "mid_block")
    assert mid["shrink_dev"] < 0 and abs(mid["shrink_dev"]) > 10 * abs(mid["shrink_ref"]), mid


@pytest.mark.gpu
def test_the_child_ran_on_the_benchmarks_picks(empty_session, seeded_session):
    """Beyond the environment variable: the picks put the 3x3 forward convolutions at 64^2 on composable-kernel solvers
    (`kernel_grouped_conv_fwd_*`), which immediate mode on an empty database never chose; the two sessions' kernels differ."""
    assert seeded_session["seeded_db"] and not empty_session["seeded_db"]
    key = "fwd x4x320x64x64 w320x320x3x3 s1"
    assert any("grouped_conv_fwd" in k for k in seeded_session["kernels"][key]), seeded_session["kernels"][key]
    differ = [g for g, ks in seeded_session["kernels"].items() if set(ks) != set(empty_session["kernels"].get(g, []))]
    assert len(differ) >= 10, differ


@pytest.mark.gpu
def test_negative_a_truncated_or_k_short_output_fails_the_comparisons(empty_session):
    """Arithmetic on one convolution's recorded tensors; no kernel is changed.  The device's untouched output passes the
    transplant bound and the shrink rule.  The f64 result TRUNCATED to bf16 fails the shrink rule (and measures 2.00 x the
    rounding error; the issue's bound admits it because of the allowance: FINDINGS).  The f64 result with the LAST K-SLICE
    dropped (the last 32 of 1280 input channels), rounded to nearest, fails the transplant bound."""
    c = empty_session["_keep"]
    ref = conv_reference(c, with_aten=False)
    own = _measure_against(c["y"], ref["y64"], ref["yabs"])
    assert transplant_ok(own, TRANSPLANT_FACTOR) and rounds_to_nearest(own), own
    trunc = _measure_against(truncate_to_bf16(ref["y64"]), ref["y64"], ref["yabs"])
    assert not rounds_to_nearest(trunc), trunc
    assert 1.9 < trunc["err"] / trunc["e_rn"] < 2.1, trunc
    short = dict(c, x=c["x"].clone())
    short["x"][:, -32:] = 0
    y_short = conv_reference(short, with_aten=False)["y64"].to(torch.bfloat16)
    m = _measure_against(y_short, ref["y64"], ref["yabs"])
    assert not transplant_ok(m, TRANSPLANT_FACTOR), m
    # the same for the data gradient: untouched passes, truncated fails the shrink rule
    own_g = _measure_against(c["gi"], ref["gi64"], ref["giabs"])
    assert transplant_ok(own_g, TRANSPLANT_FACTOR) and rounds_to_nearest(own_g), own_g
    assert not rounds_to_nearest(_measure_against(truncate_to_bf16(ref["gi64"]), ref["gi64"], ref["giabs"]))


if __name__ == "__main__":
    _main(sys.argv[1:])
