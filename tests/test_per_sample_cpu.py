"""Per-sample LoRA tables on the CPU path (the semantics every device route is held to) and the argument checks of the
new C entry points (the library loads without a GPU)."""
import ctypes as C
import os
import types

import pytest
import torch

import lora_amd as L
from lora_amd import _C
from lora_amd.lora_manager import LoRAManager
from lora_amd.standin import tiny_unet
from tests import helpers as H


def _unet(extended=True, r=4, seed=0):
    torch.manual_seed(seed)
    u = tiny_unet()
    (L.inject_trainable_lora_extended if extended else L.inject_trainable_lora)(u, r=r)
    for up, _ in L.extract_lora_ups_down(u, L.UNET_EXTENDED_TARGET_REPLACE if extended else
                                         L.UNET_DEFAULT_TARGET_REPLACE):
        up.weight.data.normal_(0, 0.05)
    return u.eval()


def _inputs(B, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 4, 16, 16, generator=g), torch.arange(B) * 37 + 5, torch.randn(B, 7, 32, generator=g))


@torch.no_grad()
def _run(u, x, t, e):
    return u(x, t, e).sample


@torch.no_grad()
def _per_row(u, x, t, e, n, setup):
    """Sample b alone after the per-module calls for row b % n."""
    out = []
    for b in range(x.shape[0]):
        setup(b % n)
        out.append(_run(u, x[b:b + 1], t[b:b + 1], e[b:b + 1]))
    return torch.cat(out)


@pytest.mark.parametrize("mult", [1, 2])
@pytest.mark.parametrize("kind", ["diag", "alpha", "both"])
def test_batched_per_sample_equals_per_row_calls(kind, mult):
    u = _unet()
    n, r = 3, 4
    diags = torch.tensor([[1.0, 0.0, 0.5, 2.0], [0.0, 1.0, 1.0, 0.0], [0.3, -0.7, 1.5, 1.0]])
    alphas = torch.tensor([0.0, 0.6, 1.7])
    x, t, e = _inputs(n * mult)
    if kind in ("diag", "both"):
        L.set_lora_diag_per_sample(u, diags)
    if kind in ("alpha", "both"):
        L.tune_lora_scale_per_sample(u, alphas)
    y = _run(u, x, t, e)
    L.clear_lora_per_sample(u)

    def setup(q):
        if kind in ("diag", "both"):
            L.set_lora_diag(u, diags[q])
        if kind in ("alpha", "both"):
            L.tune_lora_scale(u, float(alphas[q]))

    want = _per_row(u, x, t, e, n, setup)
    torch.testing.assert_close(y, want, rtol=1e-5, atol=1e-5)


def test_adapter_modules_per_sample_exact():
    """One Linear (3-D input: 5 rows per sample) and one Conv2d adapter: bit-equal to the per-row calls."""
    torch.manual_seed(0)
    lin = L.LoraInjectedLinear(16, 24, True, r=4, dropout_p=0.0, scale=0.7)
    conv = L.LoraInjectedConv2d(6, 10, 3, padding=1, r=4, dropout_p=0.0, scale=0.7)
    for m, x in ((lin, torch.randn(6, 5, 16)), (conv, torch.randn(6, 6, 8, 8))):
        m.lora_up.weight.data.normal_()
        holder = torch.nn.Sequential(m)
        d, a = torch.randn(3, 4), torch.tensor([0.25, 1.5, -2.0])
        L.set_lora_diag_per_sample(holder, d)
        L.tune_lora_scale_per_sample(holder, a)
        y = holder(x)
        L.clear_lora_per_sample(holder)
        for b in range(6):
            L.set_lora_diag(holder, d[b % 3])
            L.tune_lora_scale(holder, float(a[b % 3]))
            got = holder(x[b:b + 1])
            if isinstance(m, L.LoraInjectedLinear):  # row-wise ops: the same bits
                assert torch.equal(got, y[b:b + 1]), b
            else:  # the library conv may block a batch of 1 differently
                torch.testing.assert_close(got, y[b:b + 1], rtol=1e-5, atol=1e-5)


def test_clear_restores_bit_for_bit():
    u = _unet()
    x, t, e = _inputs(4)
    L.tune_lora_scale(u, 0.8)
    L.set_lora_diag(u, torch.tensor([1.0, 0.5, 0.0, 2.0]))
    y0 = _run(u, x, t, e)
    L.set_lora_diag_per_sample(u, torch.rand(2, 4))
    L.tune_lora_scale_per_sample(u, [0.1, 3.0])
    assert not torch.equal(_run(u, x, t, e), y0)
    L.clear_lora_per_sample(u)
    assert torch.equal(_run(u, x, t, e), y0)
    assert all("_ps_rows" not in m.__dict__ for m in u.modules())


def test_tables_do_not_touch_state_or_files(tmp_path):
    u = _unet(extended=False)
    keys0 = list(u.state_dict().keys())
    p0, p1 = str(tmp_path / "a.safetensors"), str(tmp_path / "b.safetensors")
    L.save_safeloras({"unet": (u, L.UNET_DEFAULT_TARGET_REPLACE)}, p0)
    ups0 = [(up.weight.clone(), down.weight.clone()) for up, down in L.extract_lora_ups_down(u)]
    L.set_lora_diag_per_sample(u, torch.rand(3, 4))
    L.tune_lora_scale_per_sample(u, [0.5, 1.0, 2.0])
    assert list(u.state_dict().keys()) == keys0
    assert not any("_ps" in k for k in u.state_dict())
    L.save_safeloras({"unet": (u, L.UNET_DEFAULT_TARGET_REPLACE)}, p1)
    # the file's header orders its metadata keys by a set (two saves of one model differ there already): compare what it
    # holds — the same metadata and byte-identical tensors under the same names
    from safetensors import safe_open

    f0, f1 = safe_open(p0, framework="pt"), safe_open(p1, framework="pt")
    assert f0.metadata() == f1.metadata() and sorted(f0.keys()) == sorted(f1.keys())
    for k in f0.keys():
        a, b = f0.get_tensor(k), f1.get_tensor(k)
        assert a.dtype == b.dtype and a.shape == b.shape and a.view(torch.uint8).equal(b.view(torch.uint8)), k
    assert all(torch.equal(a, up.weight) and torch.equal(b, down.weight)
               for (a, b), (up, down) in zip(ups0, L.extract_lora_ups_down(u)))
    L.clear_lora_per_sample(u)
    L.save_lora_weight(u, str(tmp_path / "c0.pt"))
    insp0 = L.inspect_lora(u)
    L.tune_lora_scale_per_sample(u, [0.5, 1.0, 2.0])
    L.save_lora_weight(u, str(tmp_path / "c1.pt"))
    w0, w1 = torch.load(str(tmp_path / "c0.pt")), torch.load(str(tmp_path / "c1.pt"))
    assert len(w0) == len(w1) and all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(w0, w1))
    assert L.inspect_lora(u) == insp0


def test_bad_shapes_raise():
    u = _unet(r=4)
    with pytest.raises(ValueError):
        L.set_lora_diag_per_sample(u, torch.rand(2, 3))  # wrong rank
    with pytest.raises(ValueError):
        L.set_lora_diag_per_sample(u, torch.rand(4))  # not [n, r]
    with pytest.raises(ValueError):
        L.tune_lora_scale_per_sample(u, torch.rand(2, 2))  # not [n]
    L.tune_lora_scale_per_sample(u, [1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        L.set_lora_diag_per_sample(u, torch.rand(2, 4))  # n differs from the alphas' n
    x, t, e = _inputs(4)
    with pytest.raises(ValueError):
        _run(u, x, t, e)  # batch 4 is not a multiple of 3
    assert all("_ps_diag" not in m.__dict__ for m in u.modules())  # a refused call changed nothing


def _toy_pipe():
    torch.manual_seed(7)
    unet = H.build_tree(H.toy_unet_spec())

    class Text(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.emb = torch.nn.Embedding(4, 8)

        def resize_token_embeddings(self, k):
            if k > self.emb.num_embeddings:
                new = torch.nn.Embedding(k, self.emb.embedding_dim)
                new.weight.data[: self.emb.num_embeddings] = self.emb.weight.data
                self.emb = new

        def get_input_embeddings(self):
            return self.emb

    from lora_amd.standin.io import StandinTokenizer

    return types.SimpleNamespace(unet=unet, text_encoder=Text(), tokenizer=StandinTokenizer(vocab_size=4))


def test_manager_tune_per_sample_one_hot_equals_tune(tmp_path, capsys):
    """The reference's mini LoRA file joined with a second one the test writes; one-hot rows = one member each."""
    second = H.build_tree(H.toy_unet_spec())
    L.inject_trainable_lora(second, target_replace_module=L.DEFAULT_TARGET_REPLACE.union({"GEGLU"}), r=3)
    torch.manual_seed(3)
    for up, _ in L.extract_lora_ups_down(second, L.DEFAULT_TARGET_REPLACE.union({"GEGLU"})):
        up.weight.data.normal_(0, 0.1)
    p2 = str(tmp_path / "second.safetensors")
    L.save_safeloras({"unet": (second, L.DEFAULT_TARGET_REPLACE.union({"GEGLU"}))}, p2)
    # the golden file carries UNet (rank 2) and text-encoder (rank 3) factors, and LoRAManager takes one rank per file:
    # its UNet half, as it stands, is the first member
    from safetensors import safe_open
    from safetensors.torch import save_file

    f = safe_open(os.path.join(H.GOLDEN, "mini_ref.safetensors"), framework="pt")
    p1 = str(tmp_path / "mini_unet.safetensors")
    save_file({k: f.get_tensor(k) for k in f.keys() if k.startswith("unet")}, p1,
              {k: v for k, v in f.metadata().items() if k.startswith("unet")})
    pipe = _toy_pipe()
    mgr = LoRAManager([p1, p2], pipe)
    assert mgr.ranklist == [2, 3]
    pipe.unet.eval()
    sites = [m for m in pipe.unet.modules() if isinstance(m, L.LoraInjectedLinear)]
    assert sites
    rows = [[1.0, 0.0], [0.0, 1.0], [0.4, 1.3]]
    torch.manual_seed(11)
    xs = [torch.randn(6, 5, m.linear.in_features) for m in sites]
    mgr.tune_per_sample(rows)
    with torch.no_grad():
        ys = [m(x) for m, x in zip(sites, xs)]
    L.clear_lora_per_sample(pipe.unet)
    for q, row in enumerate(rows):
        mgr.tune(row)
        with torch.no_grad():
            for m, x, y in zip(sites, xs, ys):
                torch.testing.assert_close(y[q::3], m(x[q::3]), rtol=1e-6, atol=1e-6)
    with pytest.raises(ValueError):
        mgr.tune_per_sample([[1.0, 0.0, 1.0]])


# ----------------------------------------------------------------------------- C entry points: argument checks
def _err(lib):
    return lib.lora_amd_last_error().decode()


def test_rowscale_entry_points_reject_bad_arguments():
    lib = _C.require()
    p = C.c_void_p(16)  # never dereferenced: every call below fails its argument checks first
    M, K, N, r = 256, 320, 320, 4
    g = lambda nsel, rps, rr: lib.lora_amd_linear_gemm_fwd_rowscale(p, K, p, K, None, p, N, p, p, None, M, K, N, rr,
                                                                   _C.BF16, 1.0, p, nsel, rps, 0, None)
    assert g(0, 1, r) == -1 and "nsel" in _err(lib)
    assert g(1, 0, r) == -1 and "rows_per_sample" in _err(lib)
    assert g(1, 1, 17) == -2 and "rank 17" in _err(lib)
    assert lib.lora_amd_linear_gemm_fwd_rowscale(p, K, p, K, None, p, N, p, p, None, M, K, N, r, _C.BF16, 1.0, None,
                                                 1, 1, 0, None) == -1
    u = lambda nsel, rps, rr: lib.lora_amd_rank_update_rowscale(p, N, p, p, M, N, rr, _C.BF16, _C.F32, _C.FACTOR_KR, 1.0,
                                                               p, nsel, rps, 0.0, 0, 0, None)
    assert u(0, 1, r) == -1 and "nsel" in _err(lib)
    assert u(1, 0, r) == -1 and "rows_per_sample" in _err(lib)
    assert u(1, 1, 65) == -2 and "rank 65" in _err(lib)
    c = lambda nsel, rps, rr: lib.lora_amd_conv_up_fwd_rowscale(p, p, p, 2, 320, 16, 16, rr, _C.BF16, _C.F32, 1.0, p,
                                                               nsel, rps, 0.0, 0, 0, None)
    assert c(0, 1, r) == -1 and "nsel" in _err(lib)
    assert c(1, 0, r) == -1 and "rows_per_sample" in _err(lib)
    assert c(1, 1, 17) == -2
