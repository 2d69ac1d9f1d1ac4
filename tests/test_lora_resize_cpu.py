"""The rank resize from the factors alone, as far as it goes without a GPU: the host plan and the launchers' argument checks
(host arithmetic on fake addresses), the exact route of ``cli_svd.resize_pairs`` against numpy f64, ``svd_resize`` on the
golden LoRA file and ``LoRAManager.compress``.  The kernels themselves: tests/test_gpu_lora_resize.py (imported here so that
its footprint case is registered when this file runs alone)."""
import copy
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import lora_amd as L
from lora_amd import _C, cli_svd
from lora_amd.lora_manager import DummySafeTensorObject, LoRAManager
from lora_amd.standin import tiny_unet
from tests import helpers as H
from tests import test_gpu_lora_resize as K   # noqa: F401  (registers the footprint case of the four launchers)
from tests.test_cli_add_manager import _lora_file

EINVAL, ERANK, EWORKSPACE = -1, -2, -4
GOLDEN = os.path.join(H.GOLDEN, "mini_ref.safetensors")


def test_plan_is_pure_host_arithmetic():
    lib = _C.require()
    assert lib.lora_amd_abi_version() == 8
    for (N, Kk, R, r), (bn, bk) in (((40, 72, 9, 4), (1, 1)), ((320, 2880, 64, 64), (2, 12)), ((1, 1, 1, 1), (1, 1))):
        pl = _C.resize_plan(N, Kk, R, r, up_ptr=4096, down_ptr=8192)
        assert pl.native == 1 and (pl.gram_blocks_n, pl.gram_blocks_k) == (bn, bk)
        assert (pl.apply_blocks_n, pl.apply_blocks_k) == (-(-N // 64), -(-Kk // 64))
        need = ((bn + bk) * R * R + 2 * R * r) * 8
        assert pl.workspace_bytes % 256 == 0 and need <= pl.workspace_bytes < need + 256
    for bad in ((40, 72, 65, 4), (40, 72, 9, 0), (40, 72, 9, 10)):
        pl = _C.ResizePlan()
        assert lib.lora_amd_resize_plan(*bad, _C.F32, 4096, 8192, C.byref(pl)) == ERANK and pl.native == 0
        with pytest.raises(ValueError):
            _C.resize_plan(*bad)
    assert b"target rank 10" in lib.lora_amd_last_error()
    # everything else the kernels do not take answers native = 0: 16-bit factors, a misaligned base, an empty side
    assert _C.resize_plan(40, 72, 9, 4, torch.bfloat16, 4096, 8192).native == 0
    assert _C.resize_plan(40, 72, 9, 4, up_ptr=4100, down_ptr=8192).native == 0
    assert _C.resize_plan(40, 72, 9, 4, up_ptr=4096, down_ptr=8200).native == 0
    assert _C.resize_plan(0, 72, 9, 4, up_ptr=4096, down_ptr=8192).native == 0


def _planned(shapes):
    lib = _C.require()
    arr = (_C.ResizeSite * len(shapes))()
    for q, (N, Kk, R, r) in zip(arr, shapes):
        q.up, q.down, q.up_out, q.down_out = 4096, 8192, 12288, 16384
        q.N, q.K, q.R, q.r = N, Kk, R, r
    geo = _C.ResizeGeometry()
    return lib, arr, geo, lib.lora_amd_resize_table_plan(arr, len(shapes), C.byref(geo))


def test_table_plan_and_launcher_argument_checks():
    shapes = [(40, 72, 9, 4), (320, 2880, 64, 64), (1, 1, 1, 1), (700, 33, 17, 5)]
    lib, arr, geo, rc = _planned(shapes)
    assert rc == 0 and geo.n_sites == 4
    off = 0
    for q, (N, Kk, R, r) in zip(arr, shapes):
        assert q.ws_offset == off
        off += _C.resize_plan(N, Kk, R, r).workspace_bytes
    assert geo.workspace_bytes == off
    assert geo.gram_grid == 2 + 12 and geo.apply_grid == 5 + 45 and geo.sign_grid == 64
    for bad in ((40, 72, 65, 4), (40, 72, 9, 0), (40, 72, 9, 10)):
        assert _planned([shapes[0], bad])[3] == ERANK
    assert _planned([(40, 0, 9, 4)])[3] == EINVAL
    arr[1].down = 8200   # a misaligned factor
    assert lib.lora_amd_resize_table_plan(arr, 4, C.byref(_C.ResizeGeometry())) == EINVAL
    assert b"site 1" in lib.lora_amd_last_error()
    # the launchers check their arguments before they launch: no GPU is touched by a refused call
    tab, ws, n, g = 1 << 20, 1 << 21, 4, C.byref(geo)
    short = geo.workspace_bytes - 1
    assert lib.lora_amd_resize_gram(tab, n, g, ws, short, None) == EWORKSPACE
    assert lib.lora_amd_resize_core(tab, n, g, ws, short, 1e-13, ws, ws, None) == EWORKSPACE
    assert lib.lora_amd_resize_apply(tab, n, g, ws, short, None) == EWORKSPACE
    assert b"workspace" in lib.lora_amd_last_error()
    for t in (tab + 8, tab + 4, 0):   # a table that is not 16-byte aligned, or null
        assert lib.lora_amd_resize_gram(t, n, g, ws, geo.workspace_bytes, None) == EINVAL
        assert lib.lora_amd_resize_core(t, n, g, ws, geo.workspace_bytes, 1e-13, ws, ws, None) == EINVAL
        assert lib.lora_amd_resize_apply(t, n, g, ws, geo.workspace_bytes, None) == EINVAL
        assert lib.lora_amd_resize_sign(t, n, g, None) == EINVAL
    assert lib.lora_amd_resize_gram(tab, 3, g, ws, geo.workspace_bytes, None) == EINVAL   # not the planned table
    assert lib.lora_amd_resize_core(tab, n, g, ws, geo.workspace_bytes, 1e-13, None, ws, None) == EINVAL
    assert lib.lora_amd_resize_gram(tab, n, g, None, geo.workspace_bytes, None) == EINVAL
    assert C.sizeof(_C.ResizeSite) == 64 and _C.ResizeSite.ws_offset.offset == 56


def _np_reference(up, down, scale=None):
    a = up.double().numpy() if scale is None else up.double().numpy() * np.asarray(scale, dtype=np.float64)[None, :]
    W = a @ down.double().numpy()
    return W, np.linalg.svd(W, compute_uv=False)


@pytest.mark.parametrize("N,Kk,R,r", [(40, 72, 9, 4), (33, 288, 17, 17), (24, 20, 64, 8), (7, 5, 2, 1), (1, 1, 1, 1)])
def test_exact_route_on_cpu_tensors_against_numpy_f64(N, Kk, R, r):
    g = torch.Generator().manual_seed(N + R)
    up, down = torch.randn(N, R, generator=g) * 1e-2, torch.randn(R, Kk, generator=g) * 0.3
    scale = torch.rand(R, generator=g) + 0.5
    before = dict(cli_svd.RESIZE_ROUTES)
    pairs, svals = cli_svd.resize_pairs([up, up.half()], [down, down.half()], r, scales=[scale, None], return_s=True)
    assert cli_svd.RESIZE_ROUTES["exact"] - before["exact"] == 2 and cli_svd.RESIZE_ROUTES["native"] == before["native"]
    for (uo, do), S, (u_in, d_in, sc) in zip(pairs, svals, ((up, down, scale), (up.half().float(), down.half().float(), None))):
        assert uo.dtype == do.dtype == torch.float32 and tuple(uo.shape) == (N, r) and tuple(do.shape) == (r, Kk)
        W, sigma = _np_reference(u_in, d_in, sc)
        m = min(N, Kk, R)
        # the optimum up to the one f32 rounding of each output factor
        err = np.linalg.norm(W - uo.double().numpy() @ do.double().numpy())
        opt = np.sqrt((sigma[r:] ** 2).sum())
        assert (err - opt) / np.linalg.norm(W) <= 2.0 ** -22
        # S: descending, the f64 singular values, zero past the product's rank
        S = S.numpy()
        assert S.shape == (R,) and (S[:-1] >= S[1:]).all()
        np.testing.assert_allclose(S[:m], sigma[:m], rtol=1e-12, atol=1e-13 * sigma[0])
        assert (S[m:] == 0).all()
        # convention: up' = U S (column norms are the singular values), down' = V^T (orthonormal rows), sign rule
        live = min(r, m)
        dd = do.double().numpy()[:live]
        np.testing.assert_allclose(dd @ dd.T, np.eye(live), atol=1e-6)
        np.testing.assert_allclose(np.linalg.norm(uo.double().numpy(), axis=0)[:live], sigma[:live], rtol=1e-6)
        assert (do[live:] == 0).all() and (uo[:, live:] == 0).all()
        assert (do.gather(1, do.abs().argmax(dim=1, keepdim=True)) >= 0).all()
    with pytest.raises(ValueError):
        cli_svd.resize_pairs([up], [torch.zeros(R + 1, Kk)], r)
    with pytest.raises(ValueError):
        cli_svd.resize_pairs([up], [down], r, scales=[scale[:-1]] if R > 1 else [torch.ones(3)])


def test_exact_route_conv_factors_clamp_and_deficient_products():
    g = torch.Generator().manual_seed(3)
    cu, cd = torch.randn(24, 12, 1, 1, generator=g), torch.randn(12, 8, 3, 3, generator=g) * 0.3
    (uo, do), = cli_svd.resize_pairs([cu], [cd], 5)
    assert tuple(uo.shape) == (24, 5, 1, 1) and tuple(do.shape) == (5, 8, 3, 3)
    W, sigma = _np_reference(cu.reshape(24, 12), cd.flatten(1))
    err = np.linalg.norm(W - uo.reshape(24, 5).double().numpy() @ do.flatten(1).double().numpy())
    assert (err - np.sqrt((sigma[5:] ** 2).sum())) / np.linalg.norm(W) <= 2.0 ** -22
    (uq, dq), = cli_svd.resize_pairs([cu], [cd], 5, clamp_quantile=0.9)
    hi = torch.quantile(torch.cat([uo.flatten(), do.flatten()]), 0.9)
    assert torch.equal(uq, uo.clamp(-hi, hi)) and torch.equal(dq, do.clamp(-hi, hi))
    # a rank above the site's: re-factored at its own rank, not padded
    (u9, d9), = cli_svd.resize_pairs([cu], [cd], 40)
    assert tuple(u9.shape) == (24, 12, 1, 1) and tuple(d9.shape) == (12, 8, 3, 3)
    # deficient products: finite, surplus rows and columns exactly zero
    up, down = torch.randn(40, 16, generator=g), torch.randn(16, 72, generator=g)
    (uz, dz), = cli_svd.resize_pairs([torch.zeros(40, 16)], [down], 4)
    assert (uz == 0).all() and (dz == 0).all()
    (ut, dt), = cli_svd.resize_pairs([torch.cat([up, up], 1)], [torch.cat([down, down], 0)], 24)
    assert torch.isfinite(ut).all() and torch.isfinite(dt).all() and (ut[:, 16:] == 0).all() and (dt[16:] == 0).all()
    assert (dt[:16].abs().amax(dim=1) > 0).all()
    np.testing.assert_allclose((ut.double() @ dt.double()).numpy(), 2 * (up.double() @ down.double()).numpy(), atol=1e-5)
    sc0 = torch.cat([torch.ones(16), torch.zeros(16)])
    (us, ds), = cli_svd.resize_pairs([torch.cat([up, up * 3], 1)], [torch.cat([down, down], 0)], 24, scales=[sc0])
    np.testing.assert_allclose((us.double() @ ds.double()).numpy(), (up.double() @ down.double()).numpy(), atol=1e-5)
    assert (ds[16:] == 0).all()


def test_svd_resize_of_the_golden_file(tmp_path):
    from safetensors import safe_open

    out = str(tmp_path / "small.safetensors")
    cli_svd.svd_resize(GOLDEN, 1, out, device="cpu")
    a, b = safe_open(GOLDEN, framework="pt"), safe_open(out, framework="pt")
    assert list(a.keys()) == list(b.keys())
    ma, mb = a.metadata(), b.metadata()
    assert set(ma) == set(mb)
    for key, value in ma.items():
        assert mb[key] == ("1" if key.endswith(":rank") else value)
    n_sites = 0
    for key in a.keys():
        ta, tb = a.get_tensor(key), b.get_tensor(key)
        if ma.get(key) == L.EMBED_FLAG:
            assert ta.dtype == tb.dtype and ta.numpy().tobytes() == tb.numpy().tobytes()
            continue
        assert tb.dtype == ta.dtype
        if key.endswith(":up"):
            n_sites += 1
            stem = key[:-3]
            up, down = b.get_tensor(stem + ":up"), b.get_tensor(stem + ":down")
            assert tuple(up.shape) == (ta.shape[0], 1) and tuple(down.shape) == (1,) + tuple(a.get_tensor(stem + ":down").shape[1:])
            W, sigma = _np_reference(ta.float(), a.get_tensor(stem + ":down").float())
            err = np.linalg.norm(W - up.double().numpy() @ down.double().numpy())
            # the file keeps its 16-bit storage: one f16 rounding of each factor on top of the optimum
            assert (err - np.sqrt((sigma[1:] ** 2).sum())) / np.linalg.norm(W) <= 2.0 ** -9
    assert n_sites == 18 + 8
    # the resized file loads like any other
    pipe = types.SimpleNamespace(unet=H.build_tree(H.toy_unet_spec()), text_encoder=H.build_tree(H.toy_clip_spec()))
    parsed = L.parse_safeloras(safe_open(out, framework="pt", device="cpu"))
    assert all(r == 1 for _, ranks, _ in parsed.values() for r in ranks)
    L.monkeypatch_or_replace_safeloras(pipe, safe_open(out, framework="pt", device="cpu"))
    adapters = [m for m in pipe.unet.modules() if isinstance(m, L.LoraInjectedLinear)]
    assert len(adapters) == 18 and all(m.r == 1 for m in adapters)
    # a rank at or above the file's: every site is copied
    same = str(tmp_path / "same.safetensors")
    cli_svd.svd_resize(GOLDEN, 3, same, device="cpu")
    c = safe_open(same, framework="pt")
    assert c.metadata() == ma and all(torch.equal(c.get_tensor(k), a.get_tensor(k)) for k in a.keys())


def test_manager_compress_at_the_joined_rank_is_lossless(tmp_path):
    p1, p2 = str(tmp_path / "a.safetensors"), str(tmp_path / "b.safetensors")
    _lora_file(p1, 2, 1), _lora_file(p2, 3, 2)
    torch.manual_seed(0)
    base = tiny_unet()
    pipe = types.SimpleNamespace(unet=copy.deepcopy(base), text_encoder=torch.nn.Identity(), tokenizer=None)
    mgr = LoRAManager([p1, p2], pipe)
    scales = [0.5, 2.0]
    mgr.tune(scales)
    pipe.unet.eval()
    x, t, ehs = torch.randn(2, 4, 16, 16), torch.tensor([10, 500]), torch.randn(2, 7, 32)
    with torch.no_grad():
        want = pipe.unet(x, t, ehs).sample
        plain = base.eval()(x, t, ehs).sample

    def patched(rank):
        tensors, metadata = mgr.compress(scales, rank)
        joined = mgr.total_safelora
        assert list(tensors) == list(joined.keys()) and set(metadata) == set(joined.metadata())
        assert all(v == str(rank) for k, v in metadata.items() if k.endswith(":rank"))
        assert all(t.dtype == torch.float32 for k, t in tensors.items() if k.startswith("unet"))
        one = types.SimpleNamespace(unet=copy.deepcopy(base), text_encoder=torch.nn.Identity())
        L.monkeypatch_or_replace_safeloras(one, DummySafeTensorObject(tensors, metadata))
        one.unet.eval()
        with torch.no_grad():
            return one.unet(x, t, ehs).sample

    got = patched(sum(mgr.ranklist))
    # f32 arithmetic: the same sums in another order through ~30 layers; 2^-23 per rounding, a few hundred of them deep
    tol = 2.0 ** -23 * 256 * float(want.abs().max())
    assert float((got - want).abs().max()) <= tol, (float((got - want).abs().max()), tol)
    assert float((want - plain).abs().max()) > 100 * tol, "the adapters must matter for this to show anything"
    # fewer ranks than the mix holds: the best approximation per site, so closer to the mix than the base model is
    low = patched(2)
    assert float((low - want).abs().max()) < float((plain - want).abs().max())
    with pytest.raises(AssertionError):
        mgr.compress([1.0], 2)
