"""lora_amd.cli_svd: the reference's SVD-distillation recipe (CPU exact path vs the reference's own code; the device
randomized path vs the exact one)."""
import copy

import numpy as np
import pytest
import torch

import lora_amd as L
from lora_amd import cli_svd as S
from tests import helpers as H


def _planted(N, K, k, noise, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(N, K, generator=g) * 0.05
    u, v = torch.randn(N, k, generator=g), torch.randn(k, K, generator=g)
    sv = torch.tensor([3.0 * 0.6 ** i for i in range(k)])
    tuned = base + (u / u.norm(dim=0)) @ torch.diag(sv) @ (v / v.norm(dim=1, keepdim=True)) * 0.2 \
        + noise * torch.randn(N, K, generator=g)
    return tuned.to(device), base.to(device)


def test_cpu_path_equals_reference_recipe():
    """up @ down and the clamp threshold equal the reference's lines executed verbatim by torch (cli_svd.py:30-47)."""
    tuned, base = _planted(96, 64, 6, 1e-3, 0)
    up, down = S.distill_pair(tuned, base, rank=4, clamp_quantile=0.99)
    res = (tuned - base).float()
    U, Sg, Vh = torch.linalg.svd(res)
    U = U[:, :4] @ torch.diag(Sg[:4])
    Vh = Vh[:4]
    hi = torch.quantile(torch.cat([U.flatten(), Vh.flatten()]), 0.99)
    # sign convention differs per vector at most; the product does not
    assert torch.allclose((up @ down), (U.clamp(-hi, hi) @ Vh.clamp(-hi, hi)), atol=2e-4)
    assert up.shape == (96, 4) and down.shape == (4, 64)


def test_overwrite_base_matches_live_reference_on_cpu():
    """Whole-model pass on a toy tree: our overwrite_base vs the reference's (its cli_svd imports diffusers, so its
    loop is restated here: the reference's lines executed by torch.linalg.svd / torch.quantile)."""
    torch.manual_seed(0)
    Holder = H.named_class("CrossAttention")

    def tree():
        t = Holder()
        t.add_module("to_q", torch.nn.Linear(24, 16, bias=False))
        t.add_module("to_k", torch.nn.Linear(12, 16, bias=False))
        return t

    base, tuned = tree(), tree()
    ours_b, ours_t = copy.deepcopy(base), copy.deepcopy(tuned)
    L.inject_trainable_lora(ours_b, r=3), L.inject_trainable_lora(ours_t, r=3)
    S.overwrite_base(ours_b, ours_t, rank=3, clamp_quantile=0.99)
    for name in ("to_q", "to_k"):
        res = getattr(tuned, name).weight.data - getattr(base, name).weight.data
        U, Sg, Vh = torch.linalg.svd(res.float())
        U = U[:, :3] @ torch.diag(Sg[:3])
        Vh = Vh[:3]
        hi = torch.quantile(torch.cat([U.flatten(), Vh.flatten()]), 0.99)
        want = U.clamp(-hi, hi) @ Vh.clamp(-hi, hi)
        m = getattr(ours_b, name)
        assert torch.allclose(m.lora_up.weight.data @ m.lora_down.weight.data, want, atol=1e-5), name


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,r", [(640, 320, 4), (1280, 2880, 8), (10240, 1280, 8), (320, 768, 16), (77, 33, 3)])
def test_device_randomized_svd_matches_exact(N, K, r):
    # noise floor ~ noise*(sqrt(N)+sqrt(K)) = 2e-3, an order below the r-th planted singular value (spectral gap: the
    # regime distillation lives in; the randomized method's error scales with (s_{l+1}/s_r)^(2*n_iter+1))
    tuned, base = _planted(N, K, r + 4, 2e-3 / (N ** 0.5 + K ** 0.5), 1, "cuda:0")
    res = (tuned - base).float()
    U, Sg, Vh = S.topr_svd(res, r)
    Ue, Se, Vhe = torch.linalg.svd(res.cpu(), full_matrices=False)
    floor = 2e-3  # singular values of the noise term; below ~10x of it the "top-r" triplets are noise directions
    sig = Se[:r] > 10 * floor
    assert torch.allclose(Sg.cpu()[sig], Se[:r][sig], rtol=1e-3, atol=1e-6), (Sg.cpu(), Se[:r])
    assert torch.allclose(Sg.cpu(), Se[:r], rtol=0.1, atol=floor)
    approx = (U @ torch.diag(Sg) @ Vh).cpu()
    exact = Ue[:, :r] @ torch.diag(Se[:r]) @ Vhe[:r]
    assert (approx - exact).norm() <= 5e-3 * exact.norm()
    # orthonormal factors
    assert torch.allclose(U.t() @ U, torch.eye(r, device=U.device), atol=1e-4)
    assert torch.allclose(Vh @ Vh.t(), torch.eye(r, device=U.device), atol=1e-4)


@pytest.mark.gpu
def test_svd_distill_cli_on_device(tmp_path):
    out = str(tmp_path / "d.safetensors")
    S.svd_distill("standin:1", "standin:2", rank=4, device="cuda:0", save_path=out)
    loras = L.load_safeloras(out)
    assert set(loras) == {"unet", "text_encoder"}
    ups = loras["unet"][0][0::2]
    # reference quirk kept: svd_distill saves with save_all's DEFAULT unet targets (cli_svd.py:130-138), so the conv
    # adapters it distilled under ResnetBlock2D are not written
    assert all(u.dim() == 2 for u in ups) and all(torch.isfinite(u).all() for u in ups)
    assert max(float(u.abs().max()) for u in ups) > 0


def test_distill_model_on_cpu_is_distill_group_per_shape():
    """The model-level entry (one ragged device iteration for all shape groups) takes the per-group reference path for
    CPU tensors: same values as ``distill_group``, in the order of the groups."""
    gs = [([_planted(48, 64, 6, 1e-3, i)[0] for i in range(2)], [_planted(48, 64, 6, 1e-3, i)[1] for i in range(2)]),
          ([_planted(96, 64, 6, 1e-3, 5)[0]], [_planted(96, 64, 6, 1e-3, 5)[1]])]
    res = S.distill_model(gs, 4)
    assert len(res) == 2
    for (t, b), (up, down) in zip(gs, res):
        up1, down1 = S.distill_group(t, b, 4)
        assert torch.equal(up, up1) and torch.equal(down, down1)
