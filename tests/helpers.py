"""Shared test helpers: module trees from JSON specs, reference loader, dtype helpers."""
from __future__ import annotations

import importlib.util
import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
REFERENCE_LORA = "/root/reference/lora_diffusion/lora.py"
if REPO not in sys.path:
    sys.path.insert(0, REPO)

_class_cache = {}


_LAP = [None]


def lap(label: str) -> None:
    """Phase timing of the long whole-step tests (``LORA_AMD_TEST_LAPS=1 pytest -s``): device-synchronised seconds since
    the previous lap, to stderr.  Off by default: no synchronisation is added to a normal run."""
    if os.environ.get("LORA_AMD_TEST_LAPS") != "1":
        return
    import time
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    now = time.perf_counter()
    if _LAP[0] is not None:
        print(f"[lap] {label}: {now - _LAP[0]:.2f} s", file=sys.stderr, flush=True)
    _LAP[0] = now


def named_class(name: str):
    """An nn.Module subclass whose __name__ is ``name`` (the finder matches class-name strings)."""
    if name not in _class_cache:
        _class_cache[name] = type(name, (nn.Module,), {})
    return _class_cache[name]


def build_tree(spec, adapter_linear=None, adapter_conv=None, dim=8):
    """spec = {"cls": str, "kind": "other|linear|conv|lora_linear|lora_conv", "children": [[name, spec], ...]}"""
    kind = spec.get("kind", "other")
    if kind == "linear":
        return nn.Linear(dim, dim, bias=spec.get("bias", True))
    if kind == "conv":
        k = spec.get("k", 3)
        return nn.Conv2d(dim, dim, k, padding=k // 2, bias=spec.get("bias", True))
    if kind == "lora_linear":
        return adapter_linear(dim, dim, spec.get("bias", True), r=spec.get("r", 2))
    if kind == "lora_conv":
        k = spec.get("k", 3)
        return adapter_conv(dim, dim, k, 1, k // 2, r=spec.get("r", 2))
    m = named_class(spec["cls"])()
    for name, child in spec.get("children", []):
        m.add_module(name, build_tree(child, adapter_linear, adapter_conv, dim))
    return m


_LORA_CHILDREN = {
    "lora_linear": [["linear", {"cls": "Linear", "kind": "linear"}], ["lora_down", {"cls": "Linear", "kind": "linear"}],
                    ["dropout", {"cls": "Dropout"}], ["lora_up", {"cls": "Linear", "kind": "linear"}],
                    ["selector", {"cls": "Identity"}]],
    "lora_conv": [["conv", {"cls": "Conv2d", "kind": "conv"}], ["lora_down", {"cls": "Conv2d", "kind": "conv"}],
                  ["dropout", {"cls": "Dropout"}], ["lora_up", {"cls": "Conv2d", "kind": "conv"}],
                  ["selector", {"cls": "Identity"}]],
}


def oracle_spec(spec):
    """Expand adapter nodes into their registered children so oracle.Node sees what named_modules() sees."""
    kind = spec.get("kind", "other")
    if kind in _LORA_CHILDREN:
        return {"cls": "LoraInjectedLinear" if kind == "lora_linear" else "LoraInjectedConv2d", "kind": kind,
                "children": _LORA_CHILDREN[kind]}
    out = {"cls": spec["cls"], "kind": kind}
    out["children"] = [[n, oracle_spec(c)] for n, c in spec.get("children", [])]
    return out


def random_tree_specs(n: int, seed: int = 0):
    """``n`` random module trees (Linear / 1x1 Conv2d leaves under target and non-target classes, depth <= 3) from one
    seeded stream: the trees of the differential test against the reference (scripts/make_golden.py::differential_cases)."""
    rng = np.random.default_rng(seed)

    def rand_spec(depth):
        kids = []
        for i in range(int(rng.integers(1, 4))):
            roll = rng.random()
            if depth >= 3 or roll < 0.35:
                kids.append([f"l{i}", {"cls": "Linear", "kind": "linear"}])
            elif roll < 0.45:
                kids.append([f"c{i}", {"cls": "Conv2d", "kind": "conv", "k": 1}])
            else:
                cls = ["CrossAttention", "GEGLU", "Attention", "ResnetBlock2D", "Other", "ModuleList"][int(rng.integers(0, 6))]
                kids.append([f"m{i}", {"cls": cls, "children": rand_spec(depth + 1)["children"]}])
        return {"cls": "Root", "children": kids}

    return [rand_spec(0) for _ in range(n)]


def reference_available() -> bool:
    return os.path.exists(REFERENCE_LORA)


def load_reference():
    """The real reference module, loaded by file path (its package __init__ needs torchvision/diffusers)."""
    spec = importlib.util.spec_from_file_location("ref_lora", REFERENCE_LORA)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def module_paths(root: nn.Module):
    return {id(m): n for n, m in root.named_modules()}


def t2n(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.float32).cpu().numpy()


TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


# ---- SD-like toy trees used by several tests -------------------------------------------------
def _lin():
    return {"cls": "Linear", "kind": "linear"}


def attn_spec(cls="CrossAttention"):
    return {"cls": cls, "children": [["to_q", _lin()], ["to_k", _lin()], ["to_v", _lin()],
                                     ["to_out", {"cls": "ModuleList", "children": [["0", _lin()], ["1", {"cls": "Dropout"}]]}]]}


def ff_spec():
    return {"cls": "FeedForward", "children": [["net", {"cls": "ModuleList", "children": [
        ["0", {"cls": "GEGLU", "children": [["proj", _lin()]]}], ["1", {"cls": "Dropout"}], ["2", _lin()]]}]]}


def block_spec():
    return {"cls": "BasicTransformerBlock", "children": [["attn1", attn_spec()], ["ff", ff_spec()],
                                                         ["attn2", attn_spec()], ["norm1", {"cls": "LayerNorm"}]]}


def resnet_spec(shortcut=True):
    ch = [["norm1", {"cls": "GroupNorm"}], ["conv1", {"cls": "Conv2d", "kind": "conv"}],
          ["time_emb_proj", _lin()], ["norm2", {"cls": "GroupNorm"}], ["conv2", {"cls": "Conv2d", "kind": "conv"}]]
    if shortcut:
        ch.append(["conv_shortcut", {"cls": "Conv2d", "kind": "conv", "k": 1}])
    return {"cls": "ResnetBlock2D", "children": ch}


def toy_unet_spec():
    return {"cls": "ToyUNet", "children": [
        ["conv_in", {"cls": "Conv2d", "kind": "conv"}],
        ["down_blocks", {"cls": "ModuleList", "children": [
            ["0", {"cls": "CrossAttnDownBlock2D", "children": [
                ["attentions", {"cls": "ModuleList", "children": [["0", {"cls": "Transformer2DModel", "children": [
                    ["proj_in", _lin()], ["transformer_blocks", {"cls": "ModuleList", "children": [["0", block_spec()]]}]]}]]}],
                ["resnets", {"cls": "ModuleList", "children": [["0", resnet_spec()], ["1", resnet_spec(False)]]}]]}]]}],
        ["up_blocks", {"cls": "ModuleList", "children": [["0", {"cls": "UpBlock2D", "children": [
            ["resnets", {"cls": "ModuleList", "children": [["0", resnet_spec()]]}]]}]]}],
        ["mid_block", {"cls": "UNetMidBlock2DCrossAttn", "children": [
            ["attentions", {"cls": "ModuleList", "children": [["0", {"cls": "Transformer2DModel", "children": [
                ["transformer_blocks", {"cls": "ModuleList", "children": [["0", block_spec()]]}]]}]]}],
            ["resnets", {"cls": "ModuleList", "children": [["0", resnet_spec(False)]]}]]}],
    ]}


def toy_clip_spec():
    layer = {"cls": "CLIPEncoderLayer", "children": [
        ["self_attn", {"cls": "CLIPAttention", "children": [["k_proj", _lin()], ["v_proj", _lin()], ["q_proj", _lin()],
                                                             ["out_proj", _lin()]]}],
        ["mlp", {"cls": "CLIPMLP", "children": [["fc1", _lin()], ["fc2", _lin()]]}]]}
    return {"cls": "ToyCLIP", "children": [["encoder", {"cls": "CLIPEncoder", "children": [
        ["layers", {"cls": "ModuleList", "children": [["0", layer], ["1", layer]]}]]}]]}


def nested_spec():
    """Ancestors nested in ancestors + pre-existing adapters: stresses de-duplication quirks."""
    return {"cls": "Root", "children": [
        ["a", {"cls": "GEGLU", "children": [["proj", _lin()], ["inner", attn_spec("Attention")]]}],
        ["b", {"cls": "CrossAttention", "children": [["to_q", {"cls": "LoraInjectedLinear", "kind": "lora_linear"}],
                                                    ["to_k", _lin()],
                                                    ["c", {"cls": "LoraInjectedConv2d", "kind": "lora_conv"}]]}],
        ["plain", _lin()],
    ]}


# ---- toy models with the call contract of cli_lora_pti.loss_step (scripts/make_golden.py::pti_loss_cases)
class PtiToyUNet(nn.Module):
    """A few-parameter stand-in with the call contract loss_step uses: ``unet(x, t, ehs).sample`` and ``.device``."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(4, 4, 3, padding=1)
        self.temb = nn.Linear(1, 4)
        self.ctx = nn.Linear(12, 4)

    @property
    def device(self):
        return self.conv.weight.device

    @property
    def dtype(self):
        return self.conv.weight.dtype

    def forward(self, x, t, ehs):
        import types

        h = self.conv(x) + self.temb(t.to(x.dtype).view(-1, 1) / 1000.0).view(-1, 4, 1, 1) \
            + self.ctx(ehs.mean(1)).view(-1, 4, 1, 1)
        return types.SimpleNamespace(sample=torch.tanh(h))


class PtiToyText(nn.Module):
    def __init__(self):
        super().__init__()
        self.emb = nn.Embedding(20, 12)

    @property
    def device(self):
        return self.emb.weight.device

    def forward(self, ids):
        return (self.emb(ids),)


# ----------------------------------------------------------------------------- the kernels' dropout stream, restated
def philox_dropout_mask(numel: int, p: float, seed: int, offset: int, device="cpu") -> torch.Tensor:
    """The multiplier (0 or 1/(1-p)) csrc/common.hpp's ``dropout_mult8`` gives element ``e`` of a dense tensor in memory
    order: Philox4x32-10 keyed by ``seed``, counter (e >> 3, offset), eight 16-bit uniforms per call, keep <=>
    u16 >= round(p * 65536).  A restatement for tests (int64 tensor arithmetic), independent of the HIP code."""
    assert numel % 8 == 0
    M32 = 0xFFFFFFFF
    idx = torch.arange(numel // 8, dtype=torch.int64, device=device)
    c0, c1 = idx & M32, (idx >> 32) & M32
    c2 = torch.full_like(idx, offset & M32)
    c3 = torch.full_like(idx, (offset >> 32) & M32)
    k0, k1 = seed & M32, (seed >> 32) & M32

    def mulhilo(a: int, b: torch.Tensor):
        # 32x32 -> 64 without overflowing int64: split b into 16-bit halves
        lo16, hi16 = b & 0xFFFF, b >> 16
        p_lo = a * lo16                      # < 2^48
        p_hi = a * hi16                      # < 2^48
        full_lo = (p_lo + ((p_hi & 0xFFFF) << 16))
        lo = full_lo & M32
        hi = ((p_hi >> 16) + (full_lo >> 32)) & M32
        return hi, lo

    for _ in range(10):
        h0, l0 = mulhilo(0xD2511F53, c0)
        h1, l1 = mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = (h1 ^ c1 ^ k0) & M32, l1, (h0 ^ c3 ^ k1) & M32, l0
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    thr = int(p * 65536.0 + 0.5)
    keep = 1.0 / (1.0 - p)
    words = torch.stack([c0, c1, c2, c3], dim=1)                          # [n/8, 4]
    u16 = torch.stack([words & 0xFFFF, words >> 16], dim=2).reshape(-1)   # element 2i = low half, 2i+1 = high half
    return (u16 >= thr).to(torch.float32) * keep


@contextlib.contextmanager
def oracle_on_device():
    """Evaluate the oracle's plain-torch op sequence (oracle/torch_ref.py) ON the GPU in f32 instead of on the host: the
    SD1.5-size whole steps take the host a minute each and the GPU suite has a time limit.  Inside this context the stand-in
    host model runs library kernels only — the fused host passes of csrc/hostops.hip, head padding and grouped projections are
    switched off — so the oracle stays independent of every hand-written kernel; f32 GEMMs / convolutions on ROCm are true f32
    (no TF32 on gfx950).  Convolutions take ATen's native im2col + rocBLAS path (MIOpen off): exact f32, and no run-time
    compilation of MIOpen kernels for the oracle's odd shapes (3x3 convs onto 16 channels: a minute of JIT on a fresh box).
    Kernel-level parity tests keep the host (numpy / f64) oracle."""
    from lora_amd.standin import fused

    prev = fused._ENABLED
    prev_cudnn = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    env = {k: os.environ.get(k) for k in ("LORA_AMD_HEAD_PAD", "LORA_AMD_GROUP_QKV")}
    fused._ENABLED = False
    os.environ["LORA_AMD_HEAD_PAD"] = os.environ["LORA_AMD_GROUP_QKV"] = "0"
    try:
        yield
    finally:
        fused._ENABLED = prev
        torch.backends.cudnn.enabled = prev_cudnn
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v



# ----------------------------------------------------------------------------- the SD1.5-size twins (whole-step parity)
def sd15_twins(r=4, ref_device="cuda:0", dev="cuda:0"):
    """SD1.5-size UNet twice: bf16 on the device exactly as bench.py builds it, and the f32 oracle twin with the same
    (bf16-representable) frozen values and the reference-algorithm adapters; same factor values (up != 0).  The oracle twin
    lives on ``ref_device``: the GPU by default (its steps are then evaluated inside ``H.oracle_on_device()``: library
    kernels only, f32 — the host needs a minute per SD1.5-size step)."""
    from bench import build_unet
    import lora_amd as L
    from lora_amd import trainer as T
    from lora_amd.standin import sd15_unet
    from oracle import torch_ref as TR

    dev_unet = build_unet(torch.device(dev), torch.bfloat16, seed=0)
    with torch.device("meta"):
        ref = sd15_unet()
    ref.to_empty(device=ref_device)
    ref.load_state_dict({k: v.float().to(ref_device) for k, v in dev_unet.state_dict().items()})
    ref.requires_grad_(False)
    ref_params = TR.inject(ref, L.UNET_DEFAULT_TARGET_REPLACE, r=r)
    g = torch.Generator().manual_seed(11)
    for s_ in TR.sites_of(ref):
        s_.up.data.copy_((torch.randn(s_.up.shape, generator=g) * 0.02).to(ref_device))
        s_.down.data.copy_((torch.randn(s_.down.shape, generator=g) / r).to(ref_device))
    L.inject_trainable_lora(dev_unet, r=r)
    T.promote_lora_to_fp32(dev_unet)
    ours = [m for m in dev_unet.modules() if isinstance(m, L.LoraInjectedLinear)]
    theirs = TR.sites_of(ref)
    assert len(ours) == len(theirs) == 144
    for a, b in zip(ours, theirs):
        a.lora_up.weight.data.copy_(b.up.data.to(dev))
        a.lora_down.weight.data.copy_(b.down.data.to(dev))
    ref.train(), dev_unet.train()
    return ref, ref_params, dev_unet


# ----------------------------------------------------------------------------- the bracket rule (whole-step parity)
def oracle_step_on_device(ref, ref_params, lat, noise, ts, ehs, autocast: bool):
    """One step of oracle/torch_ref.dreambooth_step (plain ATen ops) on the GPU: f32, or under torch.autocast(bf16) — the
    arithmetic the reference itself runs (accelerate mixed_precision="bf16", ref train_lora_dreambooth.py:489-494, 744-770).
    Returns (UNet output, loss, [gradient per LoRA tensor])."""
    import torch

    from lora_amd.standin import DDPMScheduler
    from oracle import torch_ref as TR

    out = {}

    def unet_fn(x, tt, c):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            y = ref(x, tt, c).sample
        out["pred"] = y.detach().float()
        return y

    grads = {}
    hooks = [p.register_hook(lambda gr, i=i: grads.__setitem__(i, gr.detach().clone())) for i, p in enumerate(ref_params)]
    opt = torch.optim.SGD(ref_params, lr=0.0)
    loss = TR.dreambooth_step(unet_fn, ref_params, opt, lat, noise, ts, ehs, DDPMScheduler().alphas_cumprod.to(lat.device),
                              max_grad_norm=1e30)
    for h in hooks:
        h.remove()
    return out["pred"], float(loss), [grads[i].reshape(-1).float() for i in range(len(ref_params))]


def bracket(g32, gbf, gdev, label=""):
    """The bracket rule: a device step may be as far from the f32 result as the reference's OWN bf16 arithmetic is.
    ``g32`` / ``gbf``: per-tensor LoRA gradients of the oracle's op sequence in f32 / under torch.autocast(bf16);
    ``gdev``: the device step's flat gradient.  Returns dict(aggregate, median, p90, rows) with rows =
    (ratio, tensor index, device relative error, bf16-reference relative error, elements) sorted by ratio, over the tensors
    whose f32 gradient is not numerically nothing (>= 1e-3 of the largest norm)."""
    pos, rows = 0, []
    gmax = max(float(x.norm()) for x in g32)
    tot_dev = tot_bf = 0.0
    for i, (a32, abf) in enumerate(zip(g32, gbf)):
        gd = gdev[pos:pos + a32.numel()]
        pos += a32.numel()
        ed, eb = float((gd - a32).norm()), float((abf - a32).norm())
        tot_dev += ed * ed
        tot_bf += eb * eb
        if float(a32.norm()) < 1e-3 * gmax:
            continue
        rows.append((ed / max(eb, 1e-30), i, ed / float(a32.norm()), eb / float(a32.norm()), a32.numel()))
    assert pos == gdev.numel()
    rows.sort(reverse=True)
    ratios = [r_[0] for r_ in rows]
    rep = dict(aggregate=(tot_dev / tot_bf) ** 0.5, median=ratios[len(ratios) // 2], p90=ratios[len(ratios) // 10],
               max=ratios[0], worst_rel_err=max(r_[2] for r_ in rows), rows=rows)
    print(f"[bracket {label}] LoRA gradients: aggregate ratio {rep['aggregate']:.3f}; per tensor median {rep['median']:.3f}, "
          f"90th pct {rep['p90']:.3f}, max {rep['max']:.3f}, worst relative error {rep['worst_rel_err']:.4f}, {len(ratios)} tensors")
    for r_ in rows[:6]:
        print("   tensor %d (%s of site %d, %d elements): ratio %.2f, rel err dev %.3e, bf16 ref %.3e"
              % (r_[1], "down" if r_[1] % 2 else "up", r_[1] // 2, r_[4], r_[0], r_[2], r_[3]))
    return rep


# the bracket's bounds: what five boxes measured in round 5 and round 6 (aggregate 1.27-1.41, median 1.20-1.30, worst tensor
# 2.5-4.2 x at 0.6-2 % relative error), + 10 %
BRACKET_AGGREGATE, BRACKET_MEDIAN = 1.55, 1.43


def assert_bracket(rep, aggregate=BRACKET_AGGREGATE, median=BRACKET_MEDIAN):
    assert rep["aggregate"] <= aggregate, rep["aggregate"]
    assert rep["median"] <= median, rep["median"]
    bad = [r_ for r_ in rep["rows"] if r_[0] > 4.0 and r_[2] > 0.03]   # no tensor BOTH 4 x the reference's error and 3 % off
    assert not bad, bad[:4]
    assert rep["worst_rel_err"] <= 0.05, max(rep["rows"], key=lambda r_: r_[2])
