"""Training step of the DreamBooth/PTI LoRA loop, MI355X-first.

What the reference does per step (training_scripts/train_lora_dreambooth.py:816-888) and what
this module does instead:

* ``accelerator.backward`` -> DDP bucketed NCCL all-reduce of every trainable grad
    -> ONE ``all_reduce`` (RCCL over xGMI) of ONE flat f32 buffer that already holds every
       LoRA gradient: the adapters' backward kernels accumulate straight into it.
* ``clip_grad_norm_`` over *all* UNet parameters (860 M frozen elements scanned), ``AdamW.step``,
  ``zero_grad``  -> two launches over the flat buffers (``sumsq`` + ``clip_adamw``), no host sync.
* per-step Python -> the forward/backward can be captured once into a hipGraph and replayed.

CPU tensors take a plain-torch path with the same maths (config 0 and the gloo tests).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import _C, ops
from .lora import LoraInjectedConv2d, LoraInjectedLinear


class FlatLoraState:
    """Every trainable LoRA tensor (of one or more models) as views of ONE flat f32 buffer, with flat
    gradient / Adam-moment twins.  ``groups``: ``[{"params": [...], "lr": float, "weight_decay": float}]``
    (the reference's two param groups: UNet lr / text-encoder lr, ref :659-676)."""

    def __init__(self, groups: Sequence[dict], betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: float = 1.0,
                 device: Optional[torch.device] = None):
        params: List[torch.nn.Parameter] = []
        self.group_ranges, self.lrs, self.wds = [], [], []
        pos = 0
        self.slices = {}
        for g in groups:
            begin = pos
            for p in g["params"]:
                if id(p) in self.slices:
                    continue
                self.slices[id(p)] = (pos, pos + p.numel())
                params.append(p)
                pos += p.numel()
            self.group_ranges.append((begin, pos))
            self.lrs.append(float(g["lr"]))
            self.wds.append(float(g.get("weight_decay", 1e-2)))
        if pos == 0:
            raise ValueError("FlatLoraState: no parameters")
        self.params = params
        self.n = pos
        self.device = torch.device(device) if device is not None else params[0].device
        self.betas, self.eps, self.max_grad_norm = betas, float(eps), float(max_grad_norm)
        self.flat_p = torch.empty(self.n, dtype=torch.float32, device=self.device)
        self.flat_g = torch.zeros_like(self.flat_p)
        self.exp_avg = torch.zeros_like(self.flat_p)
        self.exp_avg_sq = torch.zeros_like(self.flat_p)
        for p in params:
            a, b = self.slices[id(p)]
            self.flat_p[a:b].copy_(p.data.reshape(-1))
            p.data = self.flat_p[a:b].view(p.shape)  # fp32 master, aliasing the flat buffer
            p.grad = self.flat_g[a:b].view(p.shape)
        self.step_count = 0
        self._sinks: List[ops.GradSink] = []
        self._reduce_table, self._reduce_sig = None, None
        self.on_device = self.device.type == "cuda"
        if self.on_device:
            _C.require()
            self._sumsq = torch.zeros(1, dtype=torch.float32, device=self.device)
            self._ws = torch.empty(1024, dtype=torch.float32, device=self.device)
            self._groups_dev = _C.make_adamw_groups(self._group_rows(), self.device)
            self._step_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
            self._dev_steps: Optional[int] = 0  # host's knowledge of _step_dev, see _sync_step_counter()
        self.scaler: Optional[torch.Tensor] = None  # fp16 loss-scaling state, see enable_loss_scaling()
        self._scaler_cfg = (2.0, 0.5, 2000)
        # DDP broadcasts the parameters of rank 0 when it wraps the model (the reference's accelerator.prepare,
        # train_lora_dreambooth.py:744-757): replicas must not depend on every process having drawn the same
        # random numbers before injection
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.broadcast(self.flat_p, 0)

    def enable_loss_scaling(self, init_scale: float = 65536.0, growth_factor: float = 2.0,
                            backoff_factor: float = 0.5, growth_interval: int = 2000) -> torch.Tensor:
        """Dynamic loss scaling for fp16 compute (torch.cuda.amp.GradScaler's defaults; accelerate wraps the
        reference's step in one when mixed_precision="fp16", ref :489-494).  Returns the 4-float state tensor
        ``[scale, finite steps, 1/scale of the step being applied, finite flag]``; the step multiplies the loss by
        ``state[0]`` (``forward_backward(..., loss_scale=state.loss_scale)``), the optimiser un-scales, skips
        non-finite steps and adapts the scale — all on the device, no host sync, hipGraph-replayable."""
        self.scaler = torch.tensor([init_scale, 0.0, 1.0 / init_scale, 1.0], dtype=torch.float32, device=self.device)
        self._scaler_cfg = (float(growth_factor), float(backoff_factor), int(growth_interval))
        return self.scaler

    @property
    def loss_scale(self) -> Optional[torch.Tensor]:
        """0-d view of the current loss scale (None when loss scaling is off)."""
        return self.scaler[0] if self.scaler is not None else None

    def _group_rows(self):
        return [(a, b, lr, wd) for (a, b), lr, wd in zip(self.group_ranges, self.lrs, self.wds)]

    @property
    def payload_bytes(self) -> int:
        return self.n * 4

    def set_lrs(self, lrs: Sequence[float]) -> None:
        self.lrs = [float(x) for x in lrs]
        if self.on_device:  # same device tensor: captured graphs keep pointing at it
            self._groups_dev.copy_(_C.make_adamw_groups(self._group_rows(), "cpu"), non_blocking=True)

    def grad_view(self, p: torch.nn.Parameter) -> torch.Tensor:
        a, b = self.slices[id(p)]
        return self.flat_g[a:b].view(p.shape)

    def attach_direct_grads(self, *models: torch.nn.Module) -> int:
        """Let the adapters' backward kernels accumulate dA/dB directly into ``flat_g`` (no autograd
        AccumulateGrad launch per tensor).  Returns the number of adapters wired."""
        n = 0
        for model in models:
            for m in model.modules():
                if isinstance(m, (LoraInjectedLinear, LoraInjectedConv2d)) and id(m.lora_down.weight) in self.slices \
                        and id(m.lora_up.weight) in self.slices:
                    sink = ops.GradSink(self.grad_view(m.lora_down.weight), self.grad_view(m.lora_up.weight), self)
                    m.__dict__["_grad_sink"] = sink
                    self._sinks.append(sink)
                    n += 1
        return n

    def enable_merged_weights(self, *models: torch.nn.Module) -> "ops.MergedWeights":
        """Route every Linear adapter of ``models`` whose low-rank branch is maskless (dropout not in effect, no
        selector) through the step's merged weight: ONE ``lora_amd_merge_batched`` launch per step writes
        ``W + scale up down`` for all of them (``ops.MergedWeights``), forward and input gradient become the frozen
        dense GEMM on it, both factor gradients one launch.  Returns the object whose ``refresh()`` must open every
        step (``forward_backward(..., merged=...)`` calls it)."""
        mw = ops.MergedWeights(self)
        for model in models:
            for m in model.modules():
                if isinstance(m, LoraInjectedLinear) and id(m.lora_down.weight) in self.slices:
                    m.__dict__["_merged"] = mw
        self.merged = mw
        return mw

    def reduce_pending(self) -> None:
        """Sum every site's backward partials into the flat gradient buffer: ONE launch for all sites (after the one
        launch that produces the partials of the merged-weight sites, when those were deferred)."""
        mw = getattr(self, "merged", None)
        if mw is not None:
            mw.flush_factors()
        live = [s for s in self._sinks if s.pending is not None]
        if not live:
            return
        sig = tuple((id(s), s.pending) for s in live)
        if self._reduce_table is None or self._reduce_sig != sig:
            rows = []
            for s in live:
                rows += s.reduce_rows(s.pending)
            self._reduce_table = _C.make_reduce_table(rows, self.device)
            self._reduce_sig = sig
        table, n, total = self._reduce_table
        _C.reduce_batched(table, n, total)
        for s in live:
            s.pending = None

    def zero_grad(self) -> None:
        if getattr(self, "merged", None) is not None:
            self.merged._owed.clear()
        for s in self._sinks:
            s.pending = None
        self.flat_g.zero_()

    def all_reduce(self) -> float:
        """SUM all-reduce of the flat gradient; returns the scale (1/world) the optimiser applies."""
        self.reduce_pending()
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.flat_g, op=dist.ReduceOp.SUM)
            return 1.0 / dist.get_world_size()
        return 1.0

    def _sync_step_counter(self, graph_safe: bool) -> None:
        """Keep the host's ``step_count`` and the device counter of the ``graph_safe`` form telling the same number of
        applied steps (no loss scaling; see ``step``).  ``_dev_steps``: what the device counter holds as far as the host
        knows, None once a captured graph owns it.  Costs the ``graph_safe=False`` path one comparison."""
        if not graph_safe:
            if self._dev_steps is None:
                raise RuntimeError("FlatLoraState.step: a graph_safe step was captured into a graph, whose replays advance "
                                   "the device step counter only; the host step count is stale, so step with "
                                   "graph_safe=True from here on")
            return
        if torch.cuda.is_current_stream_capturing():
            if self._dev_steps is not None and self._dev_steps != self.step_count:
                raise RuntimeError(f"FlatLoraState.step: capturing a graph_safe step after {self.step_count} applied steps "
                                   f"while the device step counter holds {self._dev_steps}; run one step with "
                                   "graph_safe=True outside capture (the warm-up) first")
            self._dev_steps = None
        elif self._dev_steps is not None:
            if self._dev_steps != self.step_count:  # graph_safe=False steps went by: they never touch the device counter
                self._step_dev.fill_(self.step_count)
            self._dev_steps = self.step_count + 1

    def step(self, grad_scale: float = 1.0, graph_safe: bool = False) -> None:
        """clip_grad_norm_(max_grad_norm) -> AdamW -> zero_grad over the flat buffers (ref :878-888).

        Where the step number of the bias correction comes from (device tensors):

        * ``graph_safe=False`` without loss scaling: the host's ``step_count``, passed by value.  No launch and no
          synchronisation beyond ``sumsq`` + ``clip_adamw``.
        * ``graph_safe=True``: a device counter that one extra launch advances, so that the launches are the same from
          step to step and the call can be captured into a hipGraph and replayed.  Issued outside capture after
          ``graph_safe=False`` steps, the call first seeds the counter with the number of steps applied so far: the two
          forms may be mixed freely as long as nothing was captured.
        * Capturing a ``graph_safe=True`` step hands the counter to the graph: replays advance it where the host cannot
          see it without a synchronisation.  The counter must hold the applied steps at that point, which is so for a
          fresh state and after a ``graph_safe=True`` warm-up step; otherwise the capture raises ``RuntimeError``.
          From then on every step must be ``graph_safe=True`` (a replay or an eager call, both read the device
          counter); a ``graph_safe=False`` step raises ``RuntimeError`` instead of stepping with a stale host count.
        * With loss scaling (``enable_loss_scaling``) the device counter is used in every form, since only the device
          knows whether a step was applied; the forms mix freely.
        """
        self.reduce_pending()
        b1, b2 = self.betas
        if self.on_device:
            clip = self.max_grad_norm if self.max_grad_norm and self.max_grad_norm > 0 else 0.0
            scaling = self.scaler is not None
            if not scaling:
                self._sync_step_counter(graph_safe)
            self.step_count += 1
            if clip > 0 or scaling:
                _C.sumsq(self.flat_g, self._sumsq, self._ws)
            if scaling:  # finite check, un-scale factor, scale adaptation; the step counter advances only if applied
                if not graph_safe and self.step_count == 1:
                    self._step_dev.zero_()
                _C.loss_scale_update(self.scaler, self._sumsq, self._step_dev, *self._scaler_cfg)
                step = self._step_dev
            elif graph_safe:
                _C.step_advance(self._step_dev)
                step = self._step_dev
            else:
                step = self.step_count
            _C.clip_adamw(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self._groups_dev,
                          len(self.group_ranges), self._sumsq if (clip > 0 or scaling) else None, grad_scale, clip,
                          b1, b2, self.eps, step, True, scaler=self.scaler)
            return
        # CPU plumbing path (same maths as csrc/optim.hip)
        self.step_count += 1
        if self.scaler is not None:
            growth, backoff, interval = self._scaler_cfg
            scale = float(self.scaler[0])
            finite = bool(torch.isfinite(self.flat_g).all())
            self.scaler[2], self.scaler[3] = 1.0 / scale, float(finite)
            if not finite:
                self.scaler[0], self.scaler[1] = max(scale * backoff, 1.0), 0.0
                self.step_count -= 1
                self.flat_g.zero_()
                return
            good = float(self.scaler[1]) + 1.0
            if good >= interval:
                self.scaler[0], self.scaler[1] = scale * growth, 0.0
            else:
                self.scaler[1] = good
            grad_scale = grad_scale / scale
        g = self.flat_g * grad_scale
        if self.max_grad_norm and self.max_grad_norm > 0:
            total = g.norm(2)
            g = g * torch.clamp(self.max_grad_norm / (total + 1e-6), max=1.0)
        bc1 = 1 - b1 ** self.step_count
        bc2 = 1 - b2 ** self.step_count
        for (a, b), lr, wd in zip(self.group_ranges, self.lrs, self.wds):
            p, gg, m, v = self.flat_p[a:b], g[a:b], self.exp_avg[a:b], self.exp_avg_sq[a:b]
            p.mul_(1 - lr * wd)
            m.lerp_(gg, 1 - b1)
            v.mul_(b2).addcmul_(gg, gg, value=1 - b2)
            p.addcdiv_(m, (v.sqrt() / math.sqrt(bc2)).add_(self.eps), value=-lr / bc1)
        self.flat_g.zero_()

    def grad_norm(self) -> torch.Tensor:
        self.reduce_pending()
        return self.flat_g.norm(2)


def lora_params(model: torch.nn.Module) -> List[torch.nn.Parameter]:
    """[up, down, up, down, ...] of every adapter in registration order (the order the reference's
    ``itertools.chain(*unet_lora_params)`` produces, ref :661, lora.py:298-299)."""
    out = []
    for m in model.modules():
        if isinstance(m, (LoraInjectedLinear, LoraInjectedConv2d)):
            out += [m.lora_up.weight, m.lora_down.weight]
    return out


def promote_lora_to_fp32(model: torch.nn.Module) -> None:
    """Injection casts the new factors to the frozen weight's dtype (lora.py:295); with bf16-resident
    frozen weights the trainable masters must go back to f32 (what autocast training keeps them at)."""
    for p in lora_params(model):
        if p.dtype != torch.float32:
            p.data = p.data.float()


@dataclass
class StepConfig:
    with_prior_preservation: bool = False
    prior_loss_weight: float = 1.0
    num_train_timesteps: int = 1000
    t_multiplier: float = 1.0  # cli_lora_pti.py:300 (0.8 in perform_tuning)
    prediction_type: str = "epsilon"
    autocast_dtype: Optional[torch.dtype] = None  # reference-style mixed precision; None = model dtype
    # the noisy latents as diffusers forms them: scheduler.add_noise in the latents' OWN dtype (ref
    # train_lora_dreambooth.py:837); False = formed in f32 and rounded once (see forward_backward)
    reference_add_noise: bool = False


def dreambooth_loss(model_pred: torch.Tensor, target: torch.Tensor, cfg: StepConfig) -> torch.Tensor:
    """ref: train_lora_dreambooth.py:855-875."""
    if cfg.with_prior_preservation:
        pred, pred_prior = torch.chunk(model_pred, 2, dim=0)
        tgt, tgt_prior = torch.chunk(target, 2, dim=0)
        loss = F.mse_loss(pred.float(), tgt.float(), reduction="none").mean([1, 2, 3]).mean()
        return loss + cfg.prior_loss_weight * F.mse_loss(pred_prior.float(), tgt_prior.float(), reduction="mean")
    return F.mse_loss(model_pred.float(), target.float(), reduction="mean")


_CKPT_CAND = {}


def _ckpt_candidates(model):
    """The modules of ``model`` that carry a ``gradient_checkpointing`` switch (walked once per model)."""
    c = _CKPT_CAND.get(id(model))
    if c is None:
        c = _CKPT_CAND[id(model)] = [m for m in model.modules()
                                     if hasattr(m, "gradient_checkpointing") or hasattr(m, "_grad_ckpt")]
    return c


def _dropout_pool(unet, text_encoder, device):
    """One RNG launch per step for all dropout masks of the adapters (ops.dropout_pool) — unless the step recomputes
    activations (checkpointing re-runs the forward and must regenerate the SAME masks: per-site draws do, a pool does not)."""
    import contextlib

    if device.type != "cuda":
        return contextlib.nullcontext()
    ckpt = any((getattr(m, "gradient_checkpointing", False) or getattr(m, "_grad_ckpt", False)) and m.training
               for mod in (unet, text_encoder) if mod is not None for m in _ckpt_candidates(mod))
    if ckpt:
        return contextlib.nullcontext()
    return ops.dropout_pool(device)


def forward_backward(unet, scheduler, latents: torch.Tensor, cond, cfg: StepConfig,
                     text_encoder=None, noise: Optional[torch.Tensor] = None,
                     timesteps: Optional[torch.Tensor] = None, loss_scale: Optional[torch.Tensor] = None,
                     merged: Optional["ops.MergedWeights"] = None) -> torch.Tensor:
    """noise -> add_noise -> (text encoder) -> UNet -> loss -> backward (ref :823-877).
    ``merged``: the state's ``enable_merged_weights`` object — its one-launch refresh of ``W + scale up down`` opens the step.
    ``cond``: token ids [B, 77] when ``text_encoder`` is given, else encoder hidden states [B, 77, C].
    ``loss_scale``: 0-d tensor the loss is multiplied by before the backward (fp16: ``FlatLoraState.loss_scale``);
    the returned loss is the un-scaled one."""
    if merged is not None:
        merged.refresh()
    for reg in ops.conv_pack_registries(unet, text_encoder):   # conv adapters: ONE fragment-pack launch per step
        reg.refresh()
    if noise is None:
        noise = torch.randn_like(latents)
    if timesteps is None:
        timesteps = torch.randint(0, int(cfg.num_train_timesteps * cfg.t_multiplier), (latents.shape[0],),
                                  device=latents.device).long()
    # the noisy latents are formed in f32 and rounded ONCE to the compute dtype.  diffusers' DDPMScheduler.add_noise (ref
    # train_lora_dreambooth.py:837) works in the latents' dtype: under mixed precision it rounds alpha_bar_t itself to 16 bits
    # first — bf16(0.99915) = 1, so a t = 0 sample gets NO noise and small t a badly quantised one — and then rounds three more
    # times.  Measured on a batch holding t = 0 (profiles/r06_bracket_t0.log): the step's LoRA gradients sit 6.4 x as far from
    # the f32 step as the bf16-autocast reference's; formed in f32: 1.29 x.  16 K elements per sample: free.
    # StepConfig.reference_add_noise asks for the reference's arithmetic as it is.
    if latents.dtype in (torch.bfloat16, torch.float16) and not cfg.reference_add_noise:
        noisy = scheduler.add_noise(latents.float(), noise.float(), timesteps).to(latents.dtype)
    else:
        noisy = scheduler.add_noise(latents, noise, timesteps)
    ctx = torch.autocast(latents.device.type, dtype=cfg.autocast_dtype) if cfg.autocast_dtype is not None \
        else torch.autocast(latents.device.type, enabled=False)
    with ctx, _dropout_pool(unet, text_encoder, latents.device):
        ehs = text_encoder(cond)[0] if text_encoder is not None else cond
        pred = unet(noisy, timesteps, ehs).sample
    if cfg.prediction_type == "epsilon":
        target = noise
    elif cfg.prediction_type == "v_prediction":
        target = scheduler.get_velocity(latents.float(), noise.float(), timesteps)
    else:
        raise ValueError(f"Unknown prediction type {cfg.prediction_type}")
    loss = dreambooth_loss(pred, target, cfg)
    (loss * loss_scale if loss_scale is not None else loss).backward()
    return loss.detach()


class GraphedForwardBackward:
    """The forward+backward of one step captured into a hipGraph and replayed: removes the per-kernel
    host launch cost (thousands of launches per step) that bounds eager execution.

    Inputs are copied into static buffers; noise and timesteps are drawn inside the graph from torch's
    graph-safe Philox generator, so every replay sees fresh randomness.  Gradients land in the
    FlatLoraState's flat buffer (static address), the loss in ``self.loss``."""

    def __init__(self, fn: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], latents: torch.Tensor,
                 cond: torch.Tensor, state: FlatLoraState, warmup: int = 2):
        self.latents, self.cond = latents.clone(), cond.clone()
        self.state = state
        def body():
            loss = fn(self.latents, self.cond)
            state.reduce_pending()  # the batched partial reduction is part of the captured work
            return loss

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):  # also builds every lazily-allocated workspace / descriptor table
                body()
                state.zero_grad()
            # the merged-weight site table is built by the first refresh() AFTER the last new site / layout appeared, and
            # layouts keep appearing while the host model settles (the head-padded projections exist from the second
            # forward on): warm up until a step adds nothing, or the capture would find no table and the caller would fall
            # back to eager execution (round 3's configs[2] line ran 23 % slow for exactly this reason)
            mw = getattr(state, "merged", None)
            for _ in range(4):
                if mw is None or (mw._plans is not None and len(mw.entries) == getattr(self, "_n_entries", -1)):
                    break
                self._n_entries = len(mw.entries)
                body()
                state.zero_grad()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = body()

    def __call__(self, latents: torch.Tensor, cond: torch.Tensor) -> torch.Tensor:
        self.latents.copy_(latents, non_blocking=True)
        self.cond.copy_(cond, non_blocking=True)
        self.graph.replay()
        return self.loss


def get_lr_lambda(name: str, num_warmup_steps: int, num_training_steps: int,
                  lr_init: float = 1.0) -> Callable[[int], float]:
    """Multipliers of diffusers.optimization.get_scheduler (un-vendored; ref :737-742).  ``lr_init`` (the optimiser's
    base learning rate) only matters for "polynomial", whose floor is the absolute ``lr_end = 1e-7``."""
    w, T = max(0, num_warmup_steps), max(1, num_training_steps)

    def warm(s):
        return float(s) / float(max(1, w)) if s < w else None

    if name == "constant":
        return lambda s: 1.0
    if name == "constant_with_warmup":
        return lambda s: warm(s) if warm(s) is not None else 1.0
    if name == "linear":
        return lambda s: warm(s) if warm(s) is not None else max(0.0, float(T - s) / float(max(1, T - w)))
    if name in ("cosine", "cosine_with_restarts"):
        cycles = 0.5 if name == "cosine" else 1.0

        def f(s):
            if warm(s) is not None:
                return warm(s)
            prog = float(s - w) / float(max(1, T - w))
            if name == "cosine":
                return max(0.0, 0.5 * (1.0 + math.cos(math.pi * cycles * 2.0 * prog)))
            return 0.0 if prog >= 1.0 else max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((cycles * prog) % 1.0))))
        return f
    if name == "polynomial":
        def f(s, lr_end_ratio=1e-7 / float(lr_init), power=1.0):
            if warm(s) is not None:
                return warm(s)
            if s > T:
                return lr_end_ratio
            return (1 - lr_end_ratio) * (1 - (s - w) / (T - w)) ** power + lr_end_ratio
        return f
    raise ValueError(f"unknown lr scheduler {name!r}")


def init_distributed(device_type: str = "cuda"):
    """One process per GPU; RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* from the launcher's environment.
    backend "nccl" on ROCm is RCCL (xGMI within the node); gloo for CPU runs."""
    import os

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if device_type == "cuda":
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
    return rank, local, world
