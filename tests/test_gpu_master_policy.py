"""The reference's precision policy as a mode on the device: f32-resident frozen weights under 16-bit autocast, the step's
merged weights read from the f32 MASTERS (``ops.MASTER_MERGE``, csrc/merge_step.hip ``src_f32``), through the trainer, the
hipGraph runner and both CLIs."""
import os
import sys

import pytest
import torch

import lora_amd as L
from lora_amd import _C, ops
from lora_amd import trainer as T
from lora_amd.standin import DDPMScheduler
from oracle import torch_ref as TR
from tests import helpers as H
from tests.test_gpu_master_merge import CAP, round16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
sys.path.insert(0, os.path.join(H.REPO, "training_scripts"))
import train_lora_dreambooth as cli  # noqa: E402

# The bracket under the reference's policy (aggregate / median ratio of the device step's LoRA-gradient error to the
# bf16-autocast reference's own error, H.bracket): the values measured on one MI355X + 10 %, the project's convention for
# bracket bounds.  Measured (profiles/master_policy_bracket.log):
#   master merge           aggregate 1.138, median 1.089
#   MASTER_MERGE=0 shadow  aggregate 1.191, median 1.091
BOUNDS = {"master": (1.252, 1.198), "shadow": (1.310, 1.200)}


@pytest.fixture(scope="module")
def twins():
    """tests/helpers.sd15_twins with the device UNet f32-resident, and a sub-ulp residue (below half a bf16 ulp, so that
    bf16(W) is unchanged) on the frozen weight of every adapted Linear of BOTH twins: master != shadow."""
    ref, ref_params, unet = H.sd15_twins()
    unet.float()
    T.promote_lora_to_fp32(unet)
    ours = [m for m in unet.modules() if isinstance(m, L.LoraInjectedLinear)]
    g = torch.Generator(device=DEV).manual_seed(123)
    for a, b in zip(ours, TR.sites_of(ref)):
        w = a.linear.weight.data
        w16 = w.to(torch.bfloat16)
        w.mul_(1.0 + (torch.rand(w.shape, generator=g, device=DEV) * 2 - 1) * 2.0 ** -10)
        assert torch.equal(w.to(torch.bfloat16), w16) and not torch.equal(w, w16.float())
        b.frozen.weight.data.copy_(w)
    L.invalidate_caches(unet)
    yield ref, ref_params, unet
    del ref, unet
    torch.cuda.empty_cache()


def _unwire(*models):
    for model in models:
        for m in model.modules():
            m.__dict__.pop("_grad_sink", None)
            m.__dict__.pop("_merged", None)


def _batch(B=4, seed=77):
    g = torch.Generator().manual_seed(seed)
    lat = (torch.randn(B, 4, 64, 64, generator=g) * 0.18215).to(torch.bfloat16).float().to(DEV)
    ehs = torch.randn(B, 77, 768, generator=g).to(torch.bfloat16).float().to(DEV)
    noise = torch.randn(B, 4, 64, 64, generator=g).to(torch.bfloat16).float().to(DEV)
    ts = torch.randint(0, 1000, (B,), generator=g).to(DEV)
    return lat, ehs, noise, ts


def _state(unet):
    st = T.FlatLoraState([{"params": T.lora_params(unet), "lr": 1e-4, "weight_decay": 1e-2}], max_grad_norm=1.0,
                         device=torch.device(DEV))
    st.attach_direct_grads(unet)
    return st, st.enable_merged_weights(unet)


def test_merged_weights_run_on_the_masters_and_round_once(twins, monkeypatch):
    """Under ``StepConfig(autocast_dtype=bf16)`` all 144 adapters of the f32-resident UNet are master sites, none builds a
    16-bit shadow of its weight (the bias keeps its), and after ``refresh()`` every site's W_eff is the f64 value of its OWN
    master + scale up down rounded once: at most 1e-3 of the elements differ."""
    _, _, unet = twins
    monkeypatch.setattr(ops, "MERGE_ROUNDING", _C.ROUND_ONCE)
    monkeypatch.setenv("LORA_AMD_HEAD_PAD", "0")   # dense layouts: every site's W_eff has its master's shape
    L.invalidate_caches(unet)
    st, mw = _state(unet)
    lat, ehs, noise, ts = _batch(2)
    try:
        for _ in range(2):
            T.forward_backward(unet, DDPMScheduler(), lat, ehs, T.StepConfig(autocast_dtype=torch.bfloat16), noise=noise,
                               timesteps=ts, merged=mw)
            st.reduce_pending()
            assert float(st.flat_g.abs().max()) > 0 and bool(torch.isfinite(st.flat_g).all())
            st.zero_grad()
        assert mw.n_master_sites == 144
        ours = [m for m in unet.modules() if isinstance(m, L.LoraInjectedLinear)]
        assert not any("w" in m.__dict__.get("_shadow_cache", {}) for m in ours)
        assert any("b" in m.__dict__.get("_shadow_cache", {}) for m in ours)
        mw.refresh()
        assert all(p[0].src_f32 for p in mw._plans) and len(mw._plans) == 1
        assert mw.bytes_algorithmic >= sum(m.linear.weight.numel() for m in ours) * 6
        worst, seen = 0.0, set()
        for e in mw.entries.values():
            m = e["module"]
            assert e["src_f32"] and e["w_eff"].dtype == torch.bfloat16 and e["w"].dtype == torch.float32
            if tuple(e["w_eff"].shape) != tuple(m.linear.weight.shape):
                continue   # head-padded layouts: the kernel tests cover the mapping
            want = round16(m.linear.weight.double() + float(m.scale) * (m.lora_up.weight.double() @ m.lora_down.weight.double()),
                           torch.bfloat16)
            share = float((e["w_eff"] != want).double().mean())
            worst = max(worst, share)
            assert share <= CAP, (share, tuple(want.shape))
            if e["w_eff_t"] is not None:
                assert torch.equal(e["w_eff_t"], e["w_eff"].t())
            seen.add(id(m))
        print(f"\n[master policy] {len(seen)} dense sites checked, worst differing share {worst:.3e}")
        assert len(seen) == 144
    finally:
        _unwire(unet)


def test_bracket_under_the_policy_with_master_and_with_shadow_merge(twins, monkeypatch):
    """The bracket rule (tests/helpers.bracket: distance from the f32 oracle step in units of the bf16-autocast oracle's
    own distance) for the merged step under the policy, reading the masters and — ``MASTER_MERGE=0`` — 16-bit shadows of
    them, in one run.  Which of the two is closer is not asserted: nobody has measured that."""
    ref, ref_params, unet = twins
    lat, ehs, noise, ts = _batch(4)
    with H.oracle_on_device():
        _, l32, g32 = H.oracle_step_on_device(ref, ref_params, lat, noise, ts, ehs, False)
        _, lbf, gbf = H.oracle_step_on_device(ref, ref_params, lat, noise, ts, ehs, True)
    sched, reps = DDPMScheduler(), {}
    for label, master in (("master", True), ("shadow", False)):
        monkeypatch.setattr(ops, "MASTER_MERGE", master)
        L.invalidate_caches(unet)
        st, mw = _state(unet)
        try:
            for _ in range(2):
                loss = T.forward_backward(unet, sched, lat, ehs, T.StepConfig(autocast_dtype=torch.bfloat16), noise=noise,
                                          timesteps=ts, merged=mw)
                st.reduce_pending()
                gdev = st.flat_g.clone()
                st.zero_grad()
            assert mw.n_master_sites == (144 if master else 0)
        finally:
            _unwire(unet)
        reps[label] = dict(H.bracket(g32, gbf, gdev, f"reference policy, {label} merge"), loss=float(loss))
        reps[label].pop("rows")
    print("\n[master policy bracket] loss f32 %.6f, bf16 reference %.6f" % (l32, lbf))
    for k_, v in reps.items():
        print("[master policy bracket] %-7s aggregate %.3f median %.3f p90 %.3f max %.2f worst rel err %.4f loss %.6f"
              % (k_, v["aggregate"], v["median"], v["p90"], v["max"], v["worst_rel_err"], v["loss"]))
    for k_, v in reps.items():
        agg, med = BOUNDS[k_]
        assert v["aggregate"] <= agg and v["median"] <= med, (k_, v)


def _slices(unet):
    """(begin, end) of every LoRA tensor in the flat gradient (the order of T.lora_params, as FlatLoraState lays them out)."""
    out, pos = [], 0
    for p in T.lora_params(unet):
        out.append((pos, pos + p.numel()))
        pos += p.numel()
    return out


def test_graph_replay_and_eager_step_agree_under_autocast(twins):
    """``StepConfig.autocast_dtype`` inside ``GraphedForwardBackward``: the autocast context is entered inside the captured
    body.  One eager step and one replay of the same ``forward_backward`` (fixed noise and timesteps): loss within 1 %, the
    WORST per-tensor cosine of the LoRA gradients >= 0.99 — the tolerances of test_gpu_parity_r4's consecutive-steps test, which holds graph and eager
    to them (the host model's forward is two-valued from call to call, so bits are not compared)."""
    _, _, unet = twins
    L.invalidate_caches(unet)
    st, mw = _state(unet)
    lat, ehs, noise, ts = _batch(2, seed=5)
    sched, cfg = DDPMScheduler(), T.StepConfig(autocast_dtype=torch.bfloat16)

    def fwd_bwd(l_, c_):
        return T.forward_backward(unet, sched, l_, c_, cfg, noise=noise, timesteps=ts, merged=mw)

    try:
        for _ in range(2):
            fwd_bwd(lat, ehs)
            st.zero_grad()
        loss_e = float(fwd_bwd(lat, ehs))
        st.reduce_pending()
        g_e = st.flat_g.clone()
        st.zero_grad()
        runner = T.GraphedForwardBackward(fwd_bwd, lat, ehs, st)
        st.zero_grad()
        loss_g = float(runner(lat, ehs))
        g_g = st.flat_g.clone()
        assert mw.n_master_sites == 144
    finally:
        _unwire(unet)
    # the WORST cosine over the LoRA gradient tensors above 1e-4 of the largest norm (test_gpu_parity_r4._grad_cos)
    pos, cos, gmax = 0, 2.0, max(float(g_e[a:b].norm()) for a, b in _slices(unet))
    for a, b in _slices(unet):
        te, tg = g_e[a:b], g_g[a:b]
        if float(te.norm()) >= 1e-4 * gmax:
            cos = min(cos, float(torch.dot(te, tg) / (te.norm() * tg.norm() + 1e-30)))
        pos = b
    assert pos == g_e.numel()
    print(f"\n[master policy graph] loss eager {loss_e:.6f} graph {loss_g:.6f}; worst per-tensor gradient cosine {cos:.6f}, "
          f"max |diff| {float((g_e - g_g).abs().max()):.3e} of {float(g_e.abs().max()):.3e}")
    assert float(g_e.abs().max()) > 0 and bool(torch.isfinite(g_g).all())
    assert abs(loss_g - loss_e) <= 0.01 * loss_e
    assert cos >= 0.99


BASE = ["--pretrained_model_name_or_path", "standin", "--standin", "tiny", "--instance_data_dir", "synthetic:4",
        "--instance_prompt", "a photo of sks dog", "--resolution", "128", "--train_batch_size", "2", "--learning_rate",
        "1e-3", "--lr_warmup_steps", "0", "--device", "cuda", "--seed", "3", "--train_text_encoder", "--lora_rank", "8",
        "--output_format", "safe", "--frozen_dtype", "fp32"]


@pytest.mark.parametrize("precision,graph", [("bf16", 0), ("bf16", 1), ("fp16", 0)])
def test_dreambooth_cli_under_the_policy(tmp_path, capsys, precision, graph):
    """tests/test_cli_gpu.py's toy run with ``--frozen_dtype fp32``: f32 UNet and trained text encoder under autocast, eager
    and hipGraph-replayed, bf16 and (with loss scaling) fp16 — 4 steps, trained finite factors in both models, and the merged
    weights read from f32 masters."""
    out = str(tmp_path / f"{precision}{graph}")
    steps = cli.main(cli.parse_args(BASE + ["--output_dir", out, "--max_train_steps", "4", "--hip_graph", str(graph),
                                            "--mixed_precision", precision, "--reference_add_noise"]))
    assert steps == 4
    said = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("merged weights:")]
    assert len(said) == 1 and int(said[0].split(",")[1].split()[0]) > 0, said
    loras = L.load_safeloras(os.path.join(out, "lora_weight.safetensors"))
    assert set(loras) == {"unet", "text_encoder"}
    for name in ("unet", "text_encoder"):
        ups = loras[name][0][0::2]
        assert all(torch.isfinite(u).all() for u in ups) and max(float(u.abs().max()) for u in ups) > 0, name


def test_pti_cli_under_the_policy(tmp_path):
    """cli_lora_pti with ``frozen_dtype="fp32"``, extended LoRA at rank 16 (tests/test_cli_gpu.py's toy geometry): phase 2
    keeps the models f32 under autocast; conv and Linear adapters are trained and saved."""
    from lora_amd import cli_lora_pti as pti

    out = str(tmp_path / "pti")
    pti.train(instance_data_dir="synthetic:4", pretrained_model_name_or_path="standin", output_dir=out, standin="tiny",
              placeholder_tokens="<s1>", use_template="object", resolution=256, train_batch_size=2,
              max_train_steps_ti=2, max_train_steps_tuning=4, save_steps=4, gradient_accumulation_steps=1,
              lora_rank=16, use_extended_lora=True, device="cuda:0", out_name="final", frozen_dtype="fp32")
    loras, embeds = L.load_safeloras_both(os.path.join(out, "final.safetensors"))
    ups = loras["unet"][0][0::2]
    assert all(torch.isfinite(u).all() for u in ups) and set(embeds) == {"<s1>"}
    conv_ups, lin_ups = [u for u in ups if u.dim() == 4], [u for u in ups if u.dim() == 2]
    assert conv_ups and lin_ups
    assert max(float(u.abs().max()) for u in conv_ups) > 0 and max(float(u.abs().max()) for u in lin_ups) > 0
