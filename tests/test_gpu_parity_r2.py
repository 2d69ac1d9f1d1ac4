"""Round-2 device parity: the §8 rows that only had CPU evidence (a5, a8, f2), the training step against the oracle's
own restatement, hipGraph replay against eager, real-size configs[3]/[4] geometries, the SVD clamp, the RCCL code
path, and the dropout / loss-scaling / cache fixes.  Everything runs through the C-ABI (``lora_amd/_C.py``).

Tolerances: as in tests/test_gpu_kernels.py (f32 sums: 2e-5 x sum|terms|; bf16/f16: one rounding of the result);
file bytes bit-exact."""
import copy
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lora_amd as L
from lora_amd import _C, ops
from lora_amd import trainer as T
from lora_amd.standin import DDPMScheduler, tiny_unet
from oracle import lora_numpy as O
from oracle import torch_ref as TR
from tests import helpers as H
from tests.test_gpu_kernels import DT, close, n, rnd

pytestmark = pytest.mark.gpu
G = H.GOLDEN
DEV = "cuda:0"


def _npz(name):
    return dict(np.load(os.path.join(G, name)))


def quiet(fn, *a, **k):
    with redirect_stdout(io.StringIO()):
        return fn(*a, **k)


# ----------------------------------------------------------------------------- a5: extract / realize / save from device adapters
def test_extract_and_safetensors_bytes_from_device_adapters(tmp_path):
    """ref lora.py:400-421, 451-483: adapters living on the GPU -> extract_lora_as_tensor (scale folded into up, fp16)
    -> save_safeloras_with_embeds: file equal, tensor for tensor and byte for byte, to the one the reference wrote."""
    from safetensors import safe_open

    info = json.load(open(os.path.join(G, "mini_ref_info.json")))
    st = _npz("mini_ref_state.npz")
    torch.manual_seed(7)
    unet, clip = H.build_tree(H.toy_unet_spec()), H.build_tree(H.toy_clip_spec())
    L.inject_trainable_lora(unet, r=2, scale=0.7)
    L.inject_trainable_lora(clip, target_replace_module={"CLIPAttention"}, r=3)
    unet.to(DEV), clip.to(DEV)
    for tag, model, tgt in (("unet", unet, L.DEFAULT_TARGET_REPLACE), ("text_encoder", clip, {"CLIPAttention"})):
        for i, (up, down) in enumerate(L.extract_lora_ups_down(model, tgt)):
            up.weight.data = torch.from_numpy(st[f"{tag}_{i}_up"]).to(DEV)
            down.weight.data = torch.from_numpy(st[f"{tag}_{i}_down"]).to(DEV)
    pairs = L.extract_lora_as_tensor(unet)
    assert all(u.is_cuda and u.dtype == torch.float16 and d.dtype == torch.float16 for u, d in pairs)
    want_up, _ = O.realize_as_lora(st["unet_0_up"], st["unet_0_down"], info["scale_unet"])
    assert np.array_equal(n(pairs[0][0]), want_up.astype(np.float16).astype(np.float32))
    f32 = L.extract_lora_as_tensor(unet, as_fp16=False)
    assert f32[0][0].dtype == torch.float32 and np.array_equal(n(f32[0][0]), want_up)
    out = str(tmp_path / "dev.safetensors")
    quiet(L.save_safeloras_with_embeds, {"unet": (unet, L.DEFAULT_TARGET_REPLACE), "text_encoder": (clip, {"CLIPAttention"})},
          {"<s1>": torch.from_numpy(st["embed_s1"]).to(DEV), "<s2>": torch.from_numpy(st["embed_s2"]).to(DEV)}, out)
    a, b = safe_open(out, framework="pt"), safe_open(os.path.join(G, "mini_ref.safetensors"), framework="pt")
    assert list(a.keys()) == list(b.keys())
    for k in a.keys():
        ta, tb = a.get_tensor(k), b.get_tensor(k)
        assert ta.dtype == tb.dtype and ta.shape == tb.shape and ta.numpy().tobytes() == tb.numpy().tobytes(), k
    ma, mb = a.metadata(), b.metadata()
    assert {k: v for k, v in ma.items() if k not in ("unet", "text_encoder")} == \
        {k: v for k, v in mb.items() if k not in ("unet", "text_encoder")}
    # .pt form from device adapters: fp16 CPU list, scale NOT folded (ref :424-436)
    quiet(L.save_lora_weight, unet, str(tmp_path / "dev.pt"))
    mine, ref = torch.load(str(tmp_path / "dev.pt")), torch.load(os.path.join(G, "mini_ref.pt"))
    assert len(mine) == len(ref) and all(torch.equal(x, y) and not x.is_cuda for x, y in zip(mine, ref))
    # and back: patch a device model from the reference's file, adapters run on the HIP kernels
    pipe = type("P", (), {})()
    torch.manual_seed(7)
    pipe.unet, pipe.text_encoder = H.build_tree(H.toy_unet_spec()).to(DEV), H.build_tree(H.toy_clip_spec()).to(DEV)
    quiet(L.monkeypatch_or_replace_safeloras, pipe, safe_open(os.path.join(G, "mini_ref.safetensors"), framework="pt"))
    src = unet.mid_block.attentions._modules["0"].transformer_blocks._modules["0"].attn2.to_v
    dst = pipe.unet.mid_block.attentions._modules["0"].transformer_blocks._modules["0"].attn2.to_v
    assert dst.lora_up.weight.is_cuda and dst.scale == 1.0
    x = torch.randn(5, 8, device=DEV)
    src.eval(), dst.eval()
    np.testing.assert_allclose(n(dst(x)), n(src(x)), rtol=2e-3, atol=2e-3)  # fp16 storage of up*scale, down


# ----------------------------------------------------------------------------- a8: monkeypatch_add_lora on device
def test_add_lora_blend_on_device_matches_reference_vectors():
    """ref lora.py:850-874 with every tensor on the GPU (vectors produced by the reference)."""
    d = _npz("add_lora_case.npz")
    m = H.build_tree(H.attn_spec())
    L.inject_trainable_lora(m, r=2)
    m.to(DEV)
    for i, (up, down) in enumerate(L.extract_lora_ups_down(m)):
        up.weight.data = torch.from_numpy(d[f"cur{2 * i}"]).to(DEV)
        down.weight.data = torch.from_numpy(d[f"cur{2 * i + 1}"]).to(DEV)
    L.monkeypatch_add_lora(m, [torch.from_numpy(d[f"new{i}"]) for i in range(8)], alpha=0.3, beta=0.9)  # CPU list, as loaded
    for i, (up, down) in enumerate(L.extract_lora_ups_down(m)):
        assert up.weight.is_cuda and down.weight.is_cuda
        np.testing.assert_allclose(n(up.weight), d[f"after{2 * i}"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(n(down.weight), d[f"after{2 * i + 1}"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(n(up.weight), O.add_lora_blend(d[f"cur{2 * i}"], d[f"new{2 * i}"], 0.3, 0.9), rtol=1e-6,
                                   atol=1e-7)
    # the blended adapters run on the HIP kernels
    x = torch.randn(6, 8, device=DEV)
    a = m.to_q
    a.eval()
    want = F.linear(x, a.linear.weight, a.linear.bias) + (x @ a.lora_down.weight.t()) @ a.lora_up.weight.t()
    np.testing.assert_allclose(n(a(x)), n(want), rtol=1e-4, atol=1e-5)


# ----------------------------------------------------------------------------- f2: lora_add upl on device
def test_upl_on_device_equals_oracle_collapse(tmp_path):
    """ref cli_lora_add.py:96-131: model + LoRA -> model.  The device path merges every site of a model in ONE launch of
    lora_amd_merge_batched; each merged weight must equal the oracle's collapse (ref lora.py:646-655) of the base
    weight with the factors stored in the file."""
    from lora_amd import cli_lora_add as A

    lp = str(tmp_path / "l.safetensors")
    torch.manual_seed(4)
    unet = tiny_unet()
    L.inject_trainable_lora(unet, r=2)
    for up, _ in L.extract_lora_ups_down(unet):
        up.weight.data.normal_(0, 0.05)
    quiet(L.save_safeloras, {"unet": (unet, L.UNET_DEFAULT_TARGET_REPLACE)}, lp)
    out = str(tmp_path / "merged")
    quiet(A.add, "standin:7", lp, out, alpha_1=0.8, mode="upl", device=DEV)
    sd = torch.load(os.path.join(out, "unet.pt"), map_location="cpu")
    assert not any("lora" in k for k in sd)
    torch.manual_seed(7)
    base = tiny_unet()
    factors = L.load_safeloras(lp)["unet"][0]
    sites = [(name, m) for name, m in base.named_modules() if isinstance(m, torch.nn.Linear)]
    order = [m for _, _, m in L._find_modules(base, L.UNET_DEFAULT_TARGET_REPLACE, search_class=[torch.nn.Linear])]
    path = {id(m): nm for nm, m in sites}
    checked = 0
    for i, m in enumerate(order):
        up, down = factors[2 * i].data.float().numpy(), factors[2 * i + 1].data.float().numpy()  # fp16 values of the file
        want = O.collapse(m.weight.data.numpy(), up, down, 0.8)
        got = sd[path[id(m)] + ".weight"].numpy()
        # the file stores fp16 factors; patch_pipe casts them to the f32 weight dtype -> f32 merge, reference rounding
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-7 + 1e-6 * np.abs(want).max())
        checked += 1
    assert checked == len(factors) // 2 and checked > 8
    untouched = [k for k in sd if k.endswith("weight") and k[:-7] not in {path[id(m)] for m in order}]
    assert untouched and all(torch.equal(sd[k], base.state_dict()[k]) for k in untouched)


# ----------------------------------------------------------------------------- a7: step vs the oracle's restatement; graph == eager
def _twin_models(extended=False, r=4, dropout=0.0):
    """tiny UNet twice: reference-algorithm adapters (oracle/torch_ref.py) on the CPU, ours on the device, same
    frozen weights and same factor values."""
    torch.manual_seed(0)
    base = tiny_unet()
    base.requires_grad_(False)
    ref = copy.deepcopy(base)
    targets = L.UNET_EXTENDED_TARGET_REPLACE if extended else L.UNET_DEFAULT_TARGET_REPLACE
    torch.manual_seed(5)
    ref_params = TR.inject(ref, targets, r=r, dropout_p=dropout, conv=extended)
    for s in TR.sites_of(ref):
        s.up.data.normal_(0, 0.05)
    dev = base
    (L.inject_trainable_lora_extended(dev, r=r) if extended else L.inject_trainable_lora(dev, r=r))
    ours = [m for m in dev.modules() if isinstance(m, (L.LoraInjectedLinear, L.LoraInjectedConv2d))]
    theirs = TR.sites_of(ref)
    assert len(ours) == len(theirs)
    for a, b in zip(ours, theirs):
        a.dropout.p = dropout
        a.lora_up.weight.data = b.up.data.clone()
        a.lora_down.weight.data = b.down.data.clone()
    dev.to(DEV)
    ref.train(), dev.train()
    return ref, ref_params, dev


@pytest.mark.parametrize("extended", [False, True])
def test_device_training_steps_match_oracle_dreambooth_step(extended):
    """ref train_lora_dreambooth.py:824-888 restated in oracle/torch_ref.dreambooth_step (stock ATen ops, torch AdamW,
    clip_grad_norm_) vs forward_backward + FlatLoraState on the HIP kernels.  Per step: loss, every LoRA gradient, and
    the parameter update; the device parameters are then synchronised to the oracle's so that step k+1 again compares
    one step (AdamW turns a ~0 gradient into +-lr, which would otherwise compound)."""
    ref, ref_params, dev = _twin_models(extended)
    opt = torch.optim.AdamW(ref_params, lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    st = T.FlatLoraState([{"params": T.lora_params(dev), "lr": 1e-3, "weight_decay": 1e-2}], max_grad_norm=1.0,
                         device=torch.device(DEV))
    st.attach_direct_grads(dev)
    assert [tuple(p.shape) for p in st.params] == [tuple(p.shape) for p in ref_params]  # [up0, down0, up1, ...]
    sched = DDPMScheduler()
    hw = 32 if extended else 16
    for it in range(3):
        g = torch.Generator().manual_seed(100 + it)
        lat, ehs = torch.randn(2, 4, hw, hw, generator=g), torch.randn(2, 7, 32, generator=g)
        noise, t = torch.randn(2, 4, hw, hw, generator=g), torch.randint(0, 1000, (2,), generator=g)
        before = torch.cat([p.detach().reshape(-1) for p in ref_params]).clone()
        # oracle gradients (captured before its optimiser consumes them)
        grads = {}
        hooks = [p.register_hook(lambda gr, i=i: grads.__setitem__(i, gr.clone())) for i, p in enumerate(ref_params)]
        lo = TR.dreambooth_step(lambda x, tt, c: ref(x, tt, c).sample, ref_params, opt, lat, noise, t, ehs,
                                sched.alphas_cumprod)
        for h in hooks:
            h.remove()
        g_ref = torch.cat([grads[i].reshape(-1) for i in range(len(ref_params))]).numpy()
        after = torch.cat([p.detach().reshape(-1) for p in ref_params]).numpy()
        ld = T.forward_backward(dev, sched, lat.to(DEV), ehs.to(DEV), T.StepConfig(), noise=noise.to(DEV),
                                timesteps=t.to(DEV))
        assert abs(lo.item() - ld.item()) <= 1e-4 * max(1.0, abs(lo.item())), (it, lo.item(), ld.item())
        st.reduce_pending()
        g_dev = n(st.flat_g)
        gmax = np.abs(g_ref).max()
        np.testing.assert_allclose(g_dev, g_ref, rtol=2e-3, atol=2e-5 * gmax, err_msg=f"step {it} gradients")
        st.step(st.all_reduce())
        upd_ref, upd_dev = after - before.numpy(), n(st.flat_p) - before.numpy()
        # elements whose gradient stands clear of the summation noise allowed above (2e-5 gmax = 0.2 % of them): the
        # update (<= lr = 1e-3 in magnitude) must agree to 1 % of lr
        solid = np.abs(g_ref) > 1e-2 * gmax
        assert solid.sum() > 100
        np.testing.assert_allclose(upd_dev[solid], upd_ref[solid], rtol=0, atol=1e-5, err_msg=f"step {it} update")
        assert np.abs(upd_dev - upd_ref).max() <= 2.1e-3  # nothing anywhere exceeds the +-lr flip bound
        st.flat_p.copy_(torch.from_numpy(after).to(DEV))
        # Adam moments follow the device gradients; align them too so the next step starts equal
        m_ref = torch.cat([opt.state[p]["exp_avg"].reshape(-1) for p in ref_params])
        v_ref = torch.cat([opt.state[p]["exp_avg_sq"].reshape(-1) for p in ref_params])
        np.testing.assert_allclose(n(st.exp_avg), m_ref.numpy(), rtol=2e-3, atol=2e-6 * gmax)
        st.exp_avg.copy_(m_ref.to(DEV)), st.exp_avg_sq.copy_(v_ref.to(DEV))


def test_graph_replayed_step_equals_eager_step():
    """trainer.GraphedForwardBackward: the captured forward+backward (+ batched partial reduce) must leave the same loss
    and the same flat gradient as the eager call on the same inputs, replay after replay."""
    _, _, dev = _twin_models(False)
    st = T.FlatLoraState([{"params": T.lora_params(dev), "lr": 1e-3}], max_grad_norm=1.0, device=torch.device(DEV))
    st.attach_direct_grads(dev)
    sched = DDPMScheduler()
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(2, 4, 16, 16, generator=g).to(DEV)
    tsteps = torch.randint(0, 1000, (2,), generator=g).to(DEV)

    def fwd_bwd(lat, cond):  # fixed noise / timesteps: replay and eager see identical inputs
        return T.forward_backward(dev, sched, lat, cond, T.StepConfig(), noise=noise, timesteps=tsteps)

    lat0, ehs0 = torch.randn(2, 4, 16, 16, generator=g).to(DEV), torch.randn(2, 7, 32, generator=g).to(DEV)
    graphed = T.GraphedForwardBackward(fwd_bwd, lat0, ehs0, st)
    st.zero_grad()
    for k in range(3):
        lat, ehs = torch.randn(2, 4, 16, 16, generator=g).to(DEV), torch.randn(2, 7, 32, generator=g).to(DEV)
        loss_g = graphed(lat, ehs).clone()
        grad_g = st.flat_g.clone()
        st.zero_grad()
        loss_e = fwd_bwd(lat, ehs)
        st.reduce_pending()
        grad_e = st.flat_g.clone()
        st.zero_grad()
        assert float(grad_e.abs().max()) > 0
        # same kernels and launch geometry, deterministic reductions in ours; the frozen f32 GEMMs are library calls whose
        # split may differ under capture (measured: 1.2e-6 of the largest gradient) -> f32 summation-order bound
        assert abs(loss_g.item() - loss_e.item()) <= 1e-6 * abs(loss_e.item()), (k, loss_g.item(), loss_e.item())
        assert (grad_g - grad_e).abs().max().item() <= 2e-5 * grad_e.abs().max().item(), k
    p0 = st.flat_p.clone()
    graphed(lat, ehs)
    st.step(1.0, graph_safe=True)
    p_graph = st.flat_p.clone()
    assert not torch.equal(p_graph, p0)


def test_dropout_masks_fresh_per_graph_replay_and_stable_under_checkpoint():
    """ADVICE r1 (ops.py dropout stream): (1) hipGraph replays must not reuse one baked mask; (2) with activation
    checkpointing the recomputed forward must regenerate the forward's mask (else the saved T / regenerated mask
    pair is inconsistent and the gradients are wrong)."""
    torch.manual_seed(11)
    m = L.LoraInjectedLinear(320, 640, False, r=4, dropout_p=0.5, scale=1.0).to(DEV)
    m.linear.weight.data.zero_()
    m.lora_up.weight.data.normal_(0, 0.1)
    m.train()
    x = torch.randn(64, 320, device=DEV)
    # (1) capture one forward, replay twice: the zero pattern of the branch output must change
    static_x = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        m(static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        y_static = m(static_x)
    outs = []
    for _ in range(3):
        graph.replay()
        outs.append((y_static != 0).clone())
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    keep = float(outs[0].float().mean())
    assert abs(keep - 0.5) < 0.02, keep
    # (2) checkpointed recompute == plain forward/backward under the same torch seed
    from torch.utils.checkpoint import checkpoint

    def run(use_ckpt):
        torch.manual_seed(123)
        for p_ in (m.lora_up.weight, m.lora_down.weight):
            p_.grad = None
        xin = x.clone().requires_grad_(True)
        y = checkpoint(m, xin, use_reentrant=False) if use_ckpt else m(xin)
        (y * y).sum().backward()
        return y.detach().clone(), xin.grad.clone(), m.lora_up.weight.grad.clone(), m.lora_down.weight.grad.clone()

    plain, ckpt = run(False), run(True)
    for a, b, name in zip(plain, ckpt, ("y", "dx", "dup", "ddown")):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), name
    # sanity of the consistency argument: gradient of sum(y^2) through the dropped-out branch vs autograd on the mask
    y, dx, dup, _ = plain
    mask = (y != 0).float() * 2.0  # 1/(1-p)
    t = x @ m.lora_down.weight.t()
    want_dup = ((2 * y) * mask).t() @ t
    np.testing.assert_allclose(n(dup), n(want_dup), rtol=2e-4, atol=2e-4 * float(want_dup.abs().max()))


def test_loss_scaling_on_device_matches_cpu_semantics():
    """lora_amd_loss_scale_update + the scaler operand of lora_amd_clip_adamw vs the CPU restatement in
    FlatLoraState.step (GradScaler semantics: unscale, skip on inf/nan, backoff / growth)."""
    def make(device):
        p = torch.nn.Parameter(torch.linspace(-1, 1, 4096, device=device))
        st = T.FlatLoraState([{"params": [p], "lr": 1e-2, "weight_decay": 1e-2}], max_grad_norm=1.0,
                             device=torch.device(device))
        st.enable_loss_scaling(init_scale=1024.0, growth_interval=2)
        return st

    sc, sd = make("cpu"), make(DEV)
    gen = torch.Generator().manual_seed(0)
    for it in range(6):
        g = torch.randn(4096, generator=gen) * (0.01 if it != 3 else 1.0)
        for st in (sc, sd):
            st.flat_g.copy_((g * float(st.scaler[0])).to(st.device))
            if it == 2:
                st.flat_g[17] = float("nan")
            st.step(1.0)
        assert sc.scaler.tolist() == sd.scaler.cpu().tolist(), (it, sc.scaler, sd.scaler)
        np.testing.assert_allclose(n(sd.flat_p), sc.flat_p.numpy(), rtol=2e-6, atol=2e-7, err_msg=f"it {it}")
        assert float(sd.flat_g.abs().sum()) == 0.0
    assert int(sd._step_dev.item()) == sc.step_count == 5  # the skipped step did not count


def test_weight_t_cache_survives_free_and_reallocation():
    """ADVICE r1 (_C.weight_t): an address-keyed cache must not hand site A's transpose to site B after A was freed."""
    _C.invalidate_weight_caches()
    a = torch.randn(320, 640, device=DEV).to(torch.bfloat16)
    wa = _C.weight_t(a)
    assert torch.equal(wa, a.t()) and _C.weight_t(a) is wa
    ptr = a.data_ptr()
    del a
    hit = False
    for _ in range(8):  # the caching allocator would hand the freed block to the next same-size request
        b = torch.randn(320, 640, device=DEV).to(torch.bfloat16)
        hit |= b.data_ptr() == ptr
        assert torch.equal(_C.weight_t(b), b.t())
        del b
    assert not hit  # the cache entry keeps the source alive, so its address cannot be reused while cached
    _C.invalidate_weight_caches()


# ----------------------------------------------------------------------------- e: the RCCL code path executes
def test_rccl_world1_allreduce_of_the_flat_gradient():
    """backend "nccl" on ROCm is RCCL: init a 1-rank group and run FlatLoraState.all_reduce through it (the N-rank
    semantics are covered by the gloo tests; this proves the RCCL path loads and launches on this box)."""
    import torch.distributed as dist

    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29531")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        assert dist.get_backend() == "nccl"
        p = torch.nn.Parameter(torch.randn(1000, device=DEV))
        st = T.FlatLoraState([{"params": [p], "lr": 1e-3}], device=torch.device(DEV))
        st.flat_g.normal_()
        before = st.flat_g.clone()
        t = torch.ones(4, device=DEV)
        dist.all_reduce(t)
        assert t.tolist() == [1.0] * 4
        scale = st.all_reduce()  # world 1: no-op by construction, scale 1
        assert scale == 1.0 and torch.equal(st.flat_g, before)
        buf = st.flat_g.clone()
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)  # the collective the N-rank step issues, on the real payload
        torch.cuda.synchronize()
        assert torch.equal(buf, before)
        dist.broadcast(st.flat_p, 0)
        dist.barrier()
    finally:
        dist.destroy_process_group()


# ----------------------------------------------------------------------------- a3 at the real configs[3] sites (r = 16, 768^2)
REAL_CONV_SITES = [
    # B, C_in, C_out, H, W, ks  — ResnetBlock2D convs of SD1.5 at 768x768; B = 1 (configs[3] batch)
    (1, 320, 320, 96, 96, 3), (1, 640, 640, 48, 48, 3), (1, 320, 640, 48, 48, 1), (1, 1280, 1280, 24, 24, 3),
    (1, 2560, 1280, 24, 24, 3), (1, 1920, 640, 48, 48, 3), (1, 960, 320, 96, 96, 1), (1, 2560, 1280, 12, 12, 1),
]


@pytest.mark.parametrize("B,Ci,Co,Hh,Ww,ks", REAL_CONV_SITES)
def test_conv_kernels_real_size_sites_rank16(B, Ci, Co, Hh, Ww, ks):
    """The K4 entry points at the true channel counts / maps of configs[3], bf16 activations, rank 16, vs the numpy
    oracle's low-rank terms (frozen conv excluded: W = None)."""
    r, dt, scale = 16, "bf16", 0.9
    plan = _C.conv_plan(B, Ci, Co, Hh, Ww, ks, r)
    assert plan.native == 1
    pad, HW = (ks - 1) // 2, Hh * Ww
    x, g = rnd((B, Ci, Hh, Ww), dt, seed=1), rnd((B, Co, Hh, Ww), dt, seed=2)
    down, up = rnd((r, Ci, ks, ks), "f32", 0.05, seed=3), rnd((Co, r, 1, 1), "f32", 0.1, seed=4)
    bufs = ops.conv_buffers(plan, B, r, HW, DEV)
    t_part, gt_part, gt, up_part, down_part = bufs
    t = torch.empty((B, r, Hh, Ww), dtype=torch.float32, device=DEV)
    _C.conv_down_fwd(x, down, None, t_part, t, ks)
    y0 = rnd((B, Co, Hh, Ww), dt, seed=6)
    y = y0.clone()
    _C.conv_up_fwd_(y, t, up, scale, 0.0, 0, 0)
    yo, t_o = O.lora_conv2d_forward(n(x), None, None, n(down), n(up), scale, (1, 1), (pad, pad), (1, 1))
    # sum over C_in*ks*ks terms: bound of the reduction = max|x| * sum|down|
    close(n(t), t_o, np.abs(n(x)).max() * np.abs(n(down)).sum(axis=(1, 2, 3)).max(), "f32", msg="T")
    absy = np.abs(t_o).max() * np.abs(n(up)).sum(axis=1).max() * scale
    close(n(y), yo + n(y0), absy + np.abs(n(y0)), dt, msg="Y")
    dx0 = rnd((B, Ci, Hh, Ww), dt, seed=8)
    dx = dx0.clone()
    _C.conv_bwd_g(g, t, up, None, gt_part, gt, up_part, scale, 0.0, 0, 0)
    _C.conv_bwd_x(x, dx, gt, down, down_part, ks)
    d_up, d_down = torch.empty((Co, r, 1, 1), device=DEV), torch.empty((r, Ci, ks, ks), device=DEV)
    table, nn_, total = _C.make_reduce_table(ops.conv_reduce_rows(bufs, plan, Ci, Co, ks, r, d_up, d_down, 0.0), DEV)
    _C.reduce_batched(table, nn_, total)
    dxo, ddo, duo = O.lora_conv2d_backward(n(g), n(x), None, n(down), n(up), scale, (1, 1), (pad, pad), (1, 1))
    kk = 2e-4  # f32 sums over B*H*W (up to 9216) terms in a different order than numpy
    np.testing.assert_allclose(n(d_up), duo, rtol=kk * 10, atol=kk * np.abs(duo).max() + 1e-6, err_msg="dUp")
    np.testing.assert_allclose(n(d_down), ddo, rtol=kk * 10, atol=kk * np.abs(ddo).max() + 1e-6, err_msg="dDown")
    close(n(dx), dxo + n(dx0), np.abs(dxo).max() + np.abs(n(dx0)), dt, k=1e-4, msg="dX")


def test_conv_module_12x12_site_rank16_against_reference_ops():
    """The 12x12 maps of the mid block at 768^2 (3x3: rows of 12 pixels are not 16-byte chunks): whatever path the
    module takes there must match the reference's op sequence (oracle/torch_ref.conv_adapter_forward, f32 on CPU)."""
    torch.manual_seed(0)
    B, Ci, Co, Hh, r = 1, 1280, 1280, 12, 16
    m = L.LoraInjectedConv2d(Ci, Co, 3, 1, 1, r=r, dropout_p=0.0, scale=0.8)
    m.conv.weight.data.mul_(0.5)
    m.lora_up.weight.data.normal_(0, 0.05)
    x_c = torch.randn(B, Ci, Hh, Hh)
    gy_c = torch.randn(B, Co, Hh, Hh)
    xr = x_c.clone().requires_grad_(True)
    dn, upw = m.lora_down.weight.detach().clone().requires_grad_(True), m.lora_up.weight.detach().clone().requires_grad_(True)
    yr = TR.conv_adapter_forward(xr, m.conv.weight.detach(), m.conv.bias.detach(), dn, upw, 0.8, 1, 1, 1, 1)
    (yr * gy_c).sum().backward()
    m.to(DEV)
    x = x_c.to(DEV).requires_grad_(True)
    y = m(x)
    (y * gy_c.to(DEV)).sum().backward()
    for name, got, want in (("y", y, yr), ("dx", x.grad, xr.grad), ("ddown", m.lora_down.weight.grad, dn.grad),
                            ("dup", m.lora_up.weight.grad, upw.grad)):
        np.testing.assert_allclose(n(got), want.detach().numpy(), rtol=2e-3, atol=2e-3 * float(want.abs().max()),
                                   err_msg=name)


def test_clip_text_encoder_site_rank8_bf16():
    """configs[2]: CLIP attention projections (308 = 4x77 rows, 768 -> 768), rank 8, bf16, vs the numpy oracle."""
    M, K, N, r, s = 308, 768, 768, 8, 1.0
    x, w, b = rnd((M, K), "bf16", seed=1), rnd((N, K), "bf16", 0.03, seed=2), rnd((N,), "bf16", seed=3)
    down, up, g = rnd((r, K), "f32", 0.125, seed=4), rnd((N, r), "f32", 0.05, seed=5), rnd((M, N), "bf16", seed=6)
    m = L.LoraInjectedLinear(K, N, True, r=r, dropout_p=0.0, scale=s).to(DEV)
    m.linear.weight.data, m.linear.bias.data = w.clone(), b.clone()
    m.lora_down.weight.data, m.lora_up.weight.data = down.clone(), up.clone()
    xin = x.clone().requires_grad_(True)
    y = m(xin)
    y.backward(g)
    yo, _ = O.lora_linear_forward(n(x), n(w), n(b), n(down), n(up), s)
    dxo, ddo, duo, _, _ = O.lora_linear_backward(n(g), n(x), n(w), n(down), n(up), s)
    e = 2.0 ** -8
    assert np.abs(n(y) - yo).max() <= 2 * e * np.abs(yo).max()
    assert np.abs(n(xin.grad) - dxo).max() <= 2 * e * np.abs(dxo).max()
    np.testing.assert_allclose(n(m.lora_up.weight.grad), duo, rtol=5e-3, atol=5e-3 * np.abs(duo).max())
    np.testing.assert_allclose(n(m.lora_down.weight.grad), ddo, rtol=5e-3, atol=5e-3 * np.abs(ddo).max())


# ----------------------------------------------------------------------------- f1: distillation incl. the clamp, largest site
def _reference_recipe(res: torch.Tensor, rank: int, q: float):
    """ref cli_svd.py:30-47 on the CPU (exact LAPACK SVD, signed joint quantile, clamp); thin SVD: the reference's
    full_matrices=True only adds columns of U beyond the ones it keeps."""
    U, S, Vh = torch.linalg.svd(res.float(), full_matrices=False)
    U = U[:, :rank] @ torch.diag(S[:rank])
    Vh = Vh[:rank, :]
    hi = torch.quantile(torch.cat([U.flatten(), Vh.flatten()]), q)
    return U.clamp(-hi, hi), Vh.clamp(-hi, hi), float(hi), U, Vh


@pytest.mark.parametrize("N,K,r", [(10240, 1280, 8), (1280, 2880, 8)])
def test_distill_pair_on_device_vs_reference_recipe_including_clamp(N, K, r):
    """configs[4] at the largest Linear site (GEGLU proj 10240 x 1280) and a flattened 3x3 conv (320 x 2880... here
    1280 x 2880): ``distill_pair`` on the device vs the reference's recipe executed on the CPU.

    The sign of a singular-vector pair is arbitrary (LAPACK's included), and the reference's clamp threshold is a
    quantile of SIGNED entries, so (up, down) are compared after aligning each of our pairs to the reference's sign;
    the threshold itself is compared for both our native signs and the aligned ones."""
    from lora_amd import cli_svd as S
    from tests.test_cli_svd import _planted

    tuned, base = _planted(N, K, r + 4, 2e-3 / (N ** 0.5 + K ** 0.5), 1, "cpu")
    res = (tuned - base).float()
    up_ref, down_ref, hi_ref, U_ref, Vh_ref = _reference_recipe(res, r, 0.99)
    gen = torch.Generator(device=DEV).manual_seed(0)
    up, down = S.distill_pair(tuned.to(DEV), base.to(DEV), r, 0.99, generator=gen)
    assert up.shape == (N, r) and down.shape == (r, K) and up.is_cuda
    # un-clamped factors, signs aligned to the reference's
    U, Sg, Vh = S.topr_svd(res.to(DEV), r, generator=torch.Generator(device=DEV).manual_seed(0))
    U, Vh = (U @ torch.diag(Sg)).cpu(), Vh.cpu()
    sgn = torch.sign((Vh * Vh_ref).sum(1))
    Ua, Vha = U * sgn[None, :], Vh * sgn[:, None]
    assert (Ua - U_ref).abs().max() <= 5e-3 * U_ref.abs().max()
    assert (Vha - Vh_ref).abs().max() <= 5e-3 * Vh_ref.abs().max()
    hi_aligned = float(torch.quantile(torch.cat([Ua.flatten(), Vha.flatten()]), 0.99))
    assert abs(hi_aligned - hi_ref) <= 5e-3 * hi_ref
    np.testing.assert_allclose(Ua.clamp(-hi_aligned, hi_aligned).numpy(), up_ref.numpy(), rtol=0,
                               atol=5e-3 * float(up_ref.abs().max()))
    np.testing.assert_allclose(Vha.clamp(-hi_aligned, hi_aligned).numpy(), down_ref.numpy(), rtol=0,
                               atol=5e-3 * float(down_ref.abs().max()))
    # what distill_pair returned (our deterministic sign rule): same clamp applied to sign-flipped columns; the
    # threshold moves only as far as the signed quantile depends on the signs (bounded here, documented in DESIGN)
    hi_native = float(torch.quantile(torch.cat([U.flatten(), Vh.flatten()]), 0.99))
    assert abs(hi_native - hi_ref) <= 0.1 * hi_ref
    assert float(up.abs().max()) <= hi_native * (1 + 1e-6) and float(down.abs().max()) <= hi_native * (1 + 1e-6)
    prod, prod_ref = (up @ down).cpu(), up_ref @ down_ref
    assert (prod - prod_ref).norm() <= 0.05 * prod_ref.norm()


# ----------------------------------------------------------------------------- K1/K2 weight-stationary kernel (gemm_ws.hip)
WS_SHAPES = [(16384, 320, 320, 4), (4096, 640, 640, 4), (1024, 1280, 1280, 8), (308, 768, 320, 4), (308, 768, 640, 16),
             (1000, 320, 2560, 16), (130, 768, 768, 1), (77, 1280, 20, 3), (200, 640, 1284, 5)]


def _ws_reference(X, W, Bv, A, U, s, dt):
    t_ref = X @ A.T
    U16 = O.round_to(s * U, dt)
    y_ref = X @ W.T + (Bv if Bv is not None else 0.0) + O.round_to(t_ref, dt) @ U16.T
    absref = np.abs(X) @ np.abs(W).T + (np.abs(Bv) if Bv is not None else 0.0) + np.abs(t_ref) @ np.abs(U16).T
    return t_ref, y_ref, absref


@pytest.mark.parametrize("M,K,N,r", WS_SHAPES)
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("rgs", [0, 8, 1])
def test_ws_gemm_matches_oracle(M, K, N, r, dt, rgs):
    """Y = X W^T + b + s (X down^T) up^T and T through lora_amd_linear_ws (packed weight, one site) vs the numpy oracle;
    asymmetric operands, ragged M / N tails, forced row-group counts (1 = one workgroup walks every tile of a panel:
    exercises the 3-slot input ring end to end)."""
    x, w = rnd((M, K), dt, 1.0, seed=1), rnd((N, K), dt, 0.05, seed=2)
    b = rnd((N,), dt, 0.5, seed=3)
    down, up = rnd((r, K), "f32", 0.2, seed=4), rnd((N, r), "f32", 0.3, seed=5)
    assert _C.ws_supported(x, K, N, r)
    y, t = _C.linear_ws_fwd(x, w, b, down, up, 0.7, rgs)
    t_ref, y_ref, absref = _ws_reference(n(x), n(w), n(b), n(down), n(up), 0.7, dt)
    close(n(t), t_ref, np.abs(n(x)) @ np.abs(n(down)).T, "f32", k=3e-5, msg="T")
    close(n(y), y_ref, absref, dt, k=2e-3 if dt == "bf16" else 3e-4, msg="Y")


def test_ws_pack_layout_and_strided_views():
    """lora_amd_ws_pack: fragment order as documented in include/lora_amd.h, from a strided weight view and in the
    transposed orientation (element (n, k) of the packed operand read at w[k, n])."""
    def reference(B, bn):  # B [n_out, Kc]
        n_out, Kc = B.shape
        panels = -(-n_out // bn)
        want = np.zeros(panels * bn * Kc, np.float32)
        cs, kf_n = bn // 64, Kc // 32
        idx = np.arange(want.size)
        e, lane, f = idx % 8, (idx // 8) % 64, idx // 512
        kf, j, wave, panel = f % kf_n, (f // kf_n) % cs, (f // (kf_n * cs)) % 4, f // (kf_n * cs * 4)
        rows = (panel * 4 + wave) * cs * 16 + j * 16 + (lane & 15)
        cols = kf * 32 + (lane >> 4) * 8 + e
        ok = rows < n_out
        want[ok] = B[rows[ok], cols[ok]]
        return want

    big = rnd((330, 320 + 64), "bf16", 1.0, seed=9)
    w = big[:, :320]                                   # [N = 330, K = 320], row stride 384
    assert np.array_equal(n(_C.ws_pack(w)), reference(n(w), 320))
    wt = rnd((640, 136), "bf16", 1.0, seed=10)         # [N' = 640, K' = 136]: packed as B[k'][n'] for dX (contraction 640)
    assert np.array_equal(n(_C.ws_pack(wt, True)), reference(n(wt).T, 128))
    with pytest.raises(ValueError):
        _C.ws_pack(rnd((64, 100), "bf16", 1.0, seed=11))  # contraction length without a kernel


@pytest.mark.parametrize("M,K,N,r", [(4096, 640, 640, 4), (1000, 2560, 320, 16), (308, 320, 768, 4), (130, 768, 768, 3),
                                     (16384, 320, 320, 4)])
def test_ws_input_gradient(M, K, N, r):
    """dX = G W + s (G up) down and Gt = s G up through the weight-stationary kernel on W packed in the transposed
    orientation (contraction over N), factors read in place."""
    dt, s = "bf16", 0.6
    g, w = rnd((M, N), dt, 1.0, seed=2), rnd((N, K), dt, 0.05, seed=3)
    down, up = rnd((r, K), "f32", 0.2, seed=4), rnd((N, r), "f32", 0.3, seed=5)
    assert _C.ws_supported(g, N, K, r)
    dx, gt = _C.linear_ws_dx(g, w, down, up, s)
    G, W, A, U = n(g), n(w), n(down), n(up)
    gt_ref = s * (G @ U)
    close(n(gt), gt_ref, s * (np.abs(G) @ np.abs(U)), "f32", k=3e-5, msg="Gt")
    dx_ref = G @ W + O.round_to(G @ U, dt) @ O.round_to(s * A, dt)
    close(n(dx), dx_ref, np.abs(G) @ np.abs(W) + np.abs(gt_ref) @ np.abs(A), dt, k=2e-3, msg="dX")


def test_ws_three_sites_one_launch_equals_three_launches():
    """attn1's to_q / to_k / to_v read one tensor (lora.py:53-58 called three times on it): ONE launch with three sites
    must give exactly what three single-site launches give."""
    M, K, r, dt = 4096, 640, 4, "bf16"
    x = rnd((M, K), dt, 1.0, seed=1)
    sites, single = [], []
    for i, N in enumerate((640, 640, 320)):
        w, b = rnd((N, K), dt, 0.05, seed=10 + i), rnd((N,), dt, 0.5, seed=20 + i)
        down, up = rnd((r, K), "f32", 0.2, seed=30 + i), rnd((N, r), "f32", 0.3, seed=40 + i)
        sites.append(dict(wp=_C.ws_pack(w), N=N, bias=b if i != 1 else None, down=down, up=up, scale=0.5 + 0.1 * i))
        single.append(_C.linear_ws(x, [sites[-1]])[0])
    outs = _C.linear_ws(x, sites)
    for (y, t), (y1, t1) in zip(outs, single):
        assert torch.equal(y, y1) and torch.equal(t, t1)
    # writing into column slices of ONE [M, 3C] buffer (what the attention module does for q | k | v)
    buf = torch.zeros(M, 1600, dtype=DT[dt], device=DEV)
    col = 0
    for s_, N in zip(sites, (640, 640, 320)):
        s_["y"] = buf[:, col:col + N]
        col += N
    _C.linear_ws(x, sites)
    assert torch.equal(buf, torch.cat([y for y, _ in single], dim=1))


@pytest.mark.parametrize("K,Ns,M", [(640, (640, 640, 640), 4096), (768, (320, 320), 308), (320, (320, 320, 320), 1000)])
def test_linear_group_forward_backward_vs_oracle(K, Ns, M):
    """lora.lora_linear_group (q/k/v or k/v adapters on one tensor -> one weight-stationary launch, one autograd node
    with the input gradients summed in-kernel) vs the numpy oracle of lora.py:53-58 and its autograd, site by site."""
    dt, r = "bf16", 4
    torch.manual_seed(0)
    mods = []
    for i, N in enumerate(Ns):
        m = L.LoraInjectedLinear(K, N, i == 1, r=r, dropout_p=0.0, scale=0.5 + 0.25 * i)
        m.linear.weight.data.normal_(0, 0.05)
        m.lora_up.weight.data.normal_(0, 0.1)
        m.to(DEV).to(DT[dt])
        m.linear.requires_grad_(False)
        m.lora_up.weight.data = m.lora_up.weight.data.float()
        m.lora_down.weight.data = m.lora_down.weight.data.float()
        m.train()
        mods.append(m)
    x = rnd((2, M // 2, K), dt, 1.0, seed=1).requires_grad_(True)
    outs = L.lora_linear_group(mods, x)
    assert outs is not None and [tuple(o.shape) for o in outs] == [(2, M // 2, N) for N in Ns]
    gs = [rnd((2, M // 2, N), dt, 1.0, seed=10 + i) for i, N in enumerate(Ns)]
    torch.autograd.backward(outs, gs)
    X = n(x).reshape(M, K)
    dx_ref = np.zeros((M, K), np.float64)
    dx_abs = np.zeros((M, K), np.float64)
    for m, o, g in zip(mods, outs, gs):
        W, A, U = n(m.linear.weight), n(m.lora_down.weight), n(m.lora_up.weight)
        b = n(m.linear.bias) if m.linear.bias is not None else None
        t_ref, y_ref, absref = _ws_reference(X, W, b, A, U, m.scale, dt)
        close(n(o).reshape(M, -1), y_ref, absref, dt, k=2e-3, msg="Y")
        G = n(g).reshape(M, -1)
        dxo, ddo, duo, _, _ = O.lora_linear_backward(G, X, W, A, U, m.scale)
        dx_ref += dxo
        dx_abs += np.abs(G) @ np.abs(W) + m.scale * np.abs(G @ U) @ np.abs(A)
        np.testing.assert_allclose(n(m.lora_up.weight.grad), duo, rtol=5e-3, atol=5e-3 * np.abs(duo).max())
        np.testing.assert_allclose(n(m.lora_down.weight.grad), ddo, rtol=5e-3, atol=5e-3 * np.abs(ddo).max())
    # each site's contribution is rounded to bf16 when it is accumulated: len(Ns) roundings of the running sum
    got = n(x.grad).reshape(M, K)
    tol = 2e-3 * dx_abs + len(Ns) * 2.0 ** -8 * np.abs(dx_ref) + len(Ns) * 2.0 ** -8 * np.abs(dx_ref).max() * 0.05
    bad = np.abs(got - dx_ref) > tol
    assert not bad.any(), (bad.sum(), np.abs(got - dx_ref).max())
    # ineligible groups fall back (None): dropout in effect, mixed ranks, CPU tensors
    mods[0].dropout.p = 0.1
    assert L.lora_linear_group(mods, x.detach()) is None
    mods[0].dropout.p = 0.0
    assert L.lora_linear_group(mods, x.detach().cpu()) is None


# ----------------------------------------------------------------------------- f1: batched pieces of the SVD distillation
def test_batched_rowdot_colreduce_and_cholesky_qr():
    """lora_amd_rowdot_batched / colreduce_batched / chol_inverse_batched against torch on a stack of matrices, and the
    shifted CholeskyQR3 built from them (cli_svd._orth) on an ill-conditioned block."""
    from lora_amd import cli_svd as S

    g = torch.Generator().manual_seed(0)
    B, N, K, l = 3, 700, 328, 16
    x = torch.randn(B, N, K, generator=g).to(DEV)
    f = torch.randn(B, l, K, generator=g).to(DEV)
    t = _C.rowdot_batched(x, f, _C.FACTOR_RK, 0.5)
    want = 0.5 * torch.bmm(x, f.transpose(1, 2))
    assert (t - want).abs().max() <= 2e-5 * torch.bmm(x.abs(), f.abs().transpose(1, 2)).max()
    fk = f.transpose(1, 2).contiguous()
    assert torch.allclose(_C.rowdot_batched(x, fk, _C.FACTOR_KR, 0.5), t, rtol=1e-5, atol=1e-4)
    d = _C.colreduce_batched(x, t, _C.FACTOR_RK)
    wd = torch.bmm(t.transpose(1, 2), x)
    assert (d - wd).abs().max() <= 2e-5 * torch.bmm(t.abs().transpose(1, 2), x.abs()).max()
    dk = _C.colreduce_batched(x, t, _C.FACTOR_KR)
    assert torch.allclose(dk, d.transpose(1, 2), rtol=1e-5, atol=1e-3)
    for b in range(B):  # the batched launch equals the single-matrix entry points
        assert torch.equal(_C.rowdot(x[b], f[b], _C.FACTOR_RK, 0.5), t[b])
    # Cholesky inverse: L^{-1} (G + shift) L^{-T} = I
    y = torch.randn(B, N, l, generator=g).to(DEV)
    gram = torch.bmm(y.transpose(1, 2), y)
    linv = _C.chol_inverse_batched(gram.contiguous(), 0.0)
    eye = torch.bmm(torch.bmm(linv, gram), linv.transpose(1, 2))
    assert (eye - torch.eye(l, device=DEV)).abs().max() < 1e-4
    assert linv.triu(1).abs().max() == 0
    # CholeskyQR3 on columns spanning 3.5 orders of magnitude of singular values (cond^2 of the Gram ~ 1e7)
    u, _ = torch.linalg.qr(torch.randn(B, N, l, generator=g))
    v, _ = torch.linalg.qr(torch.randn(B, l, l, generator=g))
    sv = torch.logspace(0, -3.5, l)
    ill = (u * sv) @ v.transpose(1, 2)
    q = S._orth(ill.to(DEV).contiguous())
    qtq = torch.bmm(q.transpose(1, 2), q)
    assert (qtq - torch.eye(l, device=DEV)).abs().max() < 5e-5
    # same column space: projecting the input onto Q reproduces it
    proj = torch.bmm(q, torch.bmm(q.transpose(1, 2), ill.to(DEV)))
    assert (proj - ill.to(DEV)).norm() <= 1e-3 * ill.norm() * 10 ** -0.0


def test_distill_group_equals_per_site_recipe_on_device():
    """cli_svd.overwrite_base on a toy model pair: grouped batched device path vs the reference recipe per site (CPU,
    exact SVD), compared through the un-clamped rank-r product (sign-free) and the clamp threshold."""
    from lora_amd import cli_svd as S

    Holder = H.named_class("CrossAttention")

    def tree(seed):
        torch.manual_seed(seed)
        t = Holder()
        for nm in ("to_q", "to_k", "to_v"):
            t.add_module(nm, torch.nn.Linear(64, 48, bias=False))
        t.add_module("to_out", torch.nn.Linear(64, 96, bias=False))
        return t

    base = tree(0)
    tuned = copy.deepcopy(base)
    g = torch.Generator().manual_seed(1)
    for m in tuned.children():  # planted rank-5 update well above the f32 noise floor
        u, v = torch.randn(m.out_features, 5, generator=g), torch.randn(5, m.in_features, generator=g)
        m.weight.data += (u * torch.tensor([1.0, 0.5, 0.25, 0.12, 0.002])) @ v * 0.05
    ours_b, ours_t = copy.deepcopy(base).to(DEV), copy.deepcopy(tuned).to(DEV)
    quiet(L.inject_trainable_lora, ours_b, r=4), quiet(L.inject_trainable_lora, ours_t, r=4)
    # (1) the batched iteration itself, un-clamped, against the exact SVD (sign-free product, then aligned vectors)
    names = ("to_q", "to_k", "to_v")
    stack = torch.stack([(getattr(tuned, nm).weight.data - getattr(base, nm).weight.data).float() for nm in names]).to(DEV)
    U, Sg, Vh = S.topr_svd_batched(stack, 4, generator=torch.Generator(device=DEV).manual_seed(0))
    for i, nm in enumerate(names):
        _, _, _, U_ref, Vh_ref = _reference_recipe(stack[i].cpu(), 4, 0.99)
        prod, prod_ref = ((U[i] * Sg[i]) @ Vh[i]).cpu(), U_ref @ Vh_ref
        assert (prod - prod_ref).norm() <= 1e-4 * prod_ref.norm(), (nm, float((prod - prod_ref).norm() / prod_ref.norm()))
        sgn = torch.sign((Vh[i].cpu() * Vh_ref).sum(1))
        assert (Vh[i].cpu() * sgn[:, None] - Vh_ref).abs().max() <= 1e-3 * Vh_ref.abs().max(), nm
        assert ((U[i] * Sg[i]).cpu() * sgn[None, :] - U_ref).abs().max() <= 1e-3 * U_ref.abs().max(), nm
    # (2) overwrite_base (grouping by shape, clamp, write-back into the adapters) == distill_pair site by site
    quiet(S.overwrite_base, ours_b, ours_t, rank=4, clamp_quantile=0.99)
    for nm in ("to_q", "to_k", "to_v", "to_out"):
        m = getattr(ours_b, nm)
        up1, down1 = S.distill_pair(getattr(tuned, nm).weight.data.to(DEV), getattr(base, nm).weight.data.to(DEV), 4, 0.99,
                                    torch.Generator(device=DEV).manual_seed(7))
        assert m.lora_up.weight.shape == up1.shape and m.lora_down.weight.shape == down1.shape
        assert (m.lora_up.weight.data - up1).abs().max() <= 1e-4 * up1.abs().max(), nm
        assert (m.lora_down.weight.data - down1).abs().max() <= 1e-4 * down1.abs().max(), nm
        hi = float(torch.cat([up1.flatten(), down1.flatten()]).max())
        assert float(m.lora_down.weight.data.min()) >= -hi * (1 + 1e-6)  # clamped symmetrically (ref :42-47)


def test_rank_beyond_kernel_limit_is_chunked_not_refused():
    """the reference accepts any r <= min(in, out) and rank-joined files pass 64 quickly; on device the rank
    dimension is cut into chunks of <= LORA_AMD_MAX_RANK (forward, backward, selector) and collapse_lora takes the torch
    expression for such a site."""
    torch.manual_seed(0)
    K, N, r, M = 256, 192, 96, 70
    m = L.LoraInjectedLinear(K, N, True, r=r, dropout_p=0.0, scale=0.7).to(DEV)
    m.lora_up.weight.data.normal_(0, 0.05)
    diag = torch.linspace(0.2, 1.5, r)
    m.set_selector_from_diag(diag)
    x = torch.randn(M, K, device=DEV, requires_grad=True)
    y = m(x)
    g = torch.randn(M, N, device=DEV)
    y.backward(g)
    W, b, A, U = (t.detach().double().cpu() for t in (m.linear.weight, m.linear.bias, m.lora_down.weight, m.lora_up.weight))
    xd = x.detach().double().cpu().requires_grad_(True)
    A.requires_grad_(True), U.requires_grad_(True)
    yr = xd @ W.t() + b + 0.7 * (((xd @ A.t()) * diag.double()) @ U.t())
    yr.backward(g.double().cpu())
    for got, want, nm in ((y, yr, "y"), (x.grad, xd.grad, "dx"), (m.lora_down.weight.grad, A.grad, "ddown"),
                          (m.lora_up.weight.grad, U.grad, "dup")):
        # the frozen f32 GEMM may run on reduced-precision matrix cores (smoke() uses the same bound)
        assert (got.detach().double().cpu() - want.detach()).abs().max() <= 2e-3 * want.detach().abs().max(), nm
    holder = H.named_class("CrossAttention")()
    m.selector = torch.nn.Identity()
    holder.add_module("to_q", m)
    w0 = m.linear.weight.detach().clone()
    quiet(L.collapse_lora, holder, 0.5)
    want = w0 + 0.5 * (m.lora_up.weight.detach() @ m.lora_down.weight.detach())
    assert torch.allclose(m.linear.weight.detach(), want, rtol=1e-5, atol=1e-6)


# ----------------------------------------------------------------------------- nn.Dropout inside the fused MFMA kernels
@pytest.mark.parametrize("M,K,N,r,p", [(4096, 320, 320, 16, 0.1), (2048, 640, 640, 4, 0.25), (308, 768, 320, 8, 0.1),
                                       (1000, 320, 2560, 16, 0.1)])
def test_ws_kernel_dropout_forward_equals_two_launch_path(M, K, N, r, p):
    """lora.py:45, 56 on the weight-stationary kernel: same (seed, offset) -> the SAME mask as lora_amd_linear_fwd
    (Philox chunk = 8 consecutive columns of a row), so the fused output equals frozen GEMM + masked branch up to the
    one extra rounding of the two-launch path."""
    x, w, b = rnd((M, K), "bf16", seed=1), rnd((N, K), "bf16", 0.05, seed=2), rnd((N,), "bf16", seed=3)
    down, up = rnd((r, K), "f32", 0.2, seed=4), rnd((N, r), "f32", 0.5, seed=5)
    seed, s = 4321, 0.9
    off = torch.tensor([977], dtype=torch.int64, device=DEV)
    y_ws, t_ws = _C.linear_ws_fwd(x, w, b, down, up, s, 0, p, seed, off)
    y_ref = F.linear(x, w, b)
    base = y_ref.clone()
    t_ref = _C.linear_fwd_(x, y_ref, down, up, s, None, p, seed, off)
    branch = (y_ref.float() - base.float()).abs()
    assert float(branch.max()) > 0.5 and 0.5 * p < float((branch == 0).float().mean()) < 2 * p + 0.02  # a real mask
    e = 2.0 ** -8
    tol = 3 * e * (y_ref.float().abs() + branch) + 2 * e * branch.max()  # T is rounded to bf16 before the up-projection
    assert bool(((y_ws.float() - y_ref.float()).abs() <= tol).all()), float((y_ws.float() - y_ref.float()).abs().max())
    np.testing.assert_allclose(n(t_ws), n(t_ref), rtol=1e-4, atol=1e-4 * float(t_ref.abs().max()))
    # another offset -> another mask
    y_2, _ = _C.linear_ws_fwd(x, w, b, down, up, s, 0, p, seed, 12345)
    assert float((y_2.float() - y_ws.float()).abs().max()) > 0.5


@pytest.mark.parametrize("M,K,N,r,p", [(4096, 320, 320, 16, 0.1), (2048, 1280, 640, 4, 0.25), (576, 320, 1280, 16, 0.1)])
def test_ws_kernel_dropout_input_gradient_and_factor_partials(M, K, N, r, p):
    """Backward of the same site: Gt = s (mask*G) up and dX = G W + Gt down from the weight-stationary kernel, dUp
    from lora_amd_linear_bwd_factors with dropout — against the masked primitives (rowdot / colreduce) with the same
    (seed, offset)."""
    g, x = rnd((M, N), "bf16", seed=1), rnd((M, K), "bf16", seed=6)
    w = rnd((N, K), "bf16", 0.05, seed=2)
    down, up = rnd((r, K), "f32", 0.2, seed=4), rnd((N, r), "f32", 0.3, seed=5)
    t = rnd((M, r), "f32", 1.0, seed=7)
    seed, off, s = 99, 31337, 0.8
    dx, gt = _C.linear_ws_dx(g, w, down, up, s, 0, p, seed, off)
    gt_ref = _C.rowdot(g, up, _C.FACTOR_KR, s, None, False, p, seed, off)
    bound = s / (1 - p) * (n(g).__abs__() @ np.abs(n(up)))
    close(n(gt), n(gt_ref), bound, "f32", k=2e-5, msg="Gt")  # mask bits exact, bf16 G exact, f32-accurate factor (hi+lo)
    dx_ref = g.float() @ w.float() + gt_ref @ down
    e = 2.0 ** -8
    assert float((dx.float() - dx_ref).abs().max()) <= 4 * e * float(dx_ref.abs().max())
    plan = _C.linear_plan(M, K, N, r)
    up_part, down_part = (torch.empty(max(int(k), 1), device=DEV) for k in (plan.up_part_floats, plan.down_part_floats))
    _C.linear_bwd_factors(g, t, up_part, x, gt_ref, down_part, r, s, dropout=(p, seed, off))
    d_up, d_down = torch.empty((N, r), device=DEV), torch.empty((r, K), device=DEV)
    rows = [(up_part, d_up, plan.nparts_up, plan.rank_tile, N, r, _C.FACTOR_KR, 1.0, 0.0),
            (down_part, d_down, plan.nparts_down, plan.rank_tile, K, r, _C.FACTOR_RK, 1.0, 0.0)]
    table, nn_, total = _C.make_reduce_table(rows, DEV)
    _C.reduce_batched(table, nn_, total)
    d_up_ref = _C.colreduce(g, t, _C.FACTOR_KR, s, dropout_p=p, seed=seed, offset=off)
    d_down_ref = _C.colreduce(x, gt_ref, _C.FACTOR_RK, 1.0)
    np.testing.assert_allclose(n(d_up), n(d_up_ref), rtol=2e-3, atol=2e-4 * float(d_up_ref.abs().max()))
    np.testing.assert_allclose(n(d_down), n(d_down_ref), rtol=2e-3, atol=2e-4 * float(d_down_ref.abs().max()))


def test_module_with_dropout_takes_the_fused_kernels_and_matches_the_three_launch_path(monkeypatch):
    """LoraInjectedLinear in train mode with dropout 0.1 (what inject_trainable_lora_extended leaves on every site):
    the fused path (weight-stationary forward and input gradient) against LORA_AMD_GEMM=0 (library GEMM + streaming
    kernels) under the same torch seed, i.e. the same masks."""
    res = {}
    for mode in ("fused", "unfused"):
        if mode == "unfused":
            monkeypatch.setenv("LORA_AMD_GEMM", "0")
        torch.manual_seed(11)
        m = L.LoraInjectedLinear(320, 320, True, r=16, dropout_p=0.1, scale=1.0)
        m.lora_up.weight.data.normal_(0, 0.2)
        m.to(DEV)
        m.linear.to(torch.bfloat16)
        m.train()
        x = torch.randn(4096, 320, device=DEV).to(torch.bfloat16).requires_grad_(True)
        gy = torch.randn(4096, 320, device=DEV).to(torch.bfloat16)
        torch.manual_seed(5)
        y = m(x)
        y.backward(gy)
        res[mode] = [n(y), n(x.grad), n(m.lora_up.weight.grad), n(m.lora_down.weight.grad)]
    for a, b, tol in zip(res["fused"], res["unfused"], (2.0 ** -6, 2.0 ** -6, 3e-3, 3e-3)):
        assert np.abs(a - b).max() <= tol * np.abs(b).max() + 1e-6, np.abs(a - b).max() / np.abs(b).max()
