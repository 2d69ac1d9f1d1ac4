"""SVD distillation to LoRA ranks 17..64 on the matrix-core subspace iteration (lora_amd/cli_svd.py ``WIDE``): the wide planes
product (csrc/rank16_mfma.hip rowdot16_planes_wide_kernel behind ``lora_amd_rowdot16_planes``, 17 <= r <= 80), the Cholesky
inverse up to l = 80 (csrc/linear.hip chol_inverse_wide_kernel behind ``lora_amd_chol_inverse_batched``), CholeskyQR3 at l = 80
and the distillation end to end.  Every tolerance is the one the project uses for the 16-wide form (named at each use)."""
import functools

import numpy as np
import pytest
import torch

import lora_amd as L
from lora_amd import _C
from lora_amd import cli_svd as S
from tests import memguard as MG
from tests.test_gpu_kernels import DEV, close, n

pytestmark = pytest.mark.gpu
PDT = {"bf16": torch.bfloat16, "f16": torch.float16}


# ----------------------------------------------------------------------------- the planes product
@functools.lru_cache(maxsize=None)
def _planes_case(B, M, C, scale):
    """Inputs of one (B, M, C) case at the full 80 columns and their float64 product, computed once: a narrower case takes the
    leading columns of the factor and of the reference."""
    g = torch.Generator().manual_seed(B * 1000 + M + C)
    x = torch.randn(B, M, C, generator=g) * scale
    f = torch.randn(B, C, 80, generator=g)
    xn, fn = x.numpy().astype(np.float64), f.numpy().astype(np.float64)
    return x, f, np.einsum("bmc,bcr->bmr", xn, fn), np.einsum("bmc,bcr->bmr", np.abs(xn), np.abs(fn))


def _run_planes(hi, lo, f, out, r):
    prog = _C.PlanesProgram(torch.device(DEV), r, plane_dtype=hi.dtype)
    h = prog.table([(hi, lo, f, out)])
    prog.upload()
    prog.run(h)


PLANES_CASES = [(B, M, C, r, "bf16") for (B, M, C) in [(2, 17, 64), (1, 77, 320), (3, 320, 320), (1, 1280, 2880)]
                for r in (32, 40, 64, 80)] + [(3, 320, 320, 40, "f16")]


@pytest.mark.parametrize("B,M,C,r,pdt", PLANES_CASES)
def test_wide_planes_product(B, M, C, r, pdt):
    """out[b] = X[b] F[b] for 17 <= r <= 80 columns in one launch: against float64 within the bound of
    tests/test_gpu_rank16.py::test_rowdot16_planes_vs_float64 (k = 3e-5 of |X| |F|: sums of the same length); bit-equal,
    column block by column block, to the 16-column launch on F[:, :, 16 s : 16 s + 16] (at r = 40 the last block is 8 wide);
    the same bits on a second call; and, under tests/memguard.py, nothing read past the planes or the factor enters the result
    and the output is written exactly at [B, M, r]."""
    # f16's five exponent bits: entries of order 1 keep the lo plane (2^-11 of the value) out of the subnormals
    x, f80, want, bound = _planes_case(B, M, C, 0.1 if pdt == "bf16" else 4.0)
    dt = PDT[pdt]
    xd = x.to(DEV)
    hi0, lo0 = torch.empty_like(xd, dtype=dt), torch.empty_like(xd, dtype=dt)
    _C.split16_ragged([xd.view(-1)], [hi0.view(-1)], [lo0.view(-1)])
    hi, lo = MG.poisoned(hi0), MG.poisoned(lo0)                      # poison (a NaN) before and behind the planes
    f = MG.poisoned(f80[:, :, :r].contiguous().to(DEV))
    out = MG.Guarded((B, M, r), torch.float32, DEV)                  # sentinel in the data and in both guards
    _run_planes(hi, lo, f, out.data, r)
    torch.cuda.synchronize()
    out.check(f"wide planes product {B}x{M}x{C} r{r}")
    MG.assert_written(out.data, "wide planes product")
    MG.assert_finite(out.data, what="wide planes product")
    got = out.data.clone()
    close(n(got), want[:, :, :r], bound[:, :, :r], k=3e-5, msg=f"wide planes product r{r} {pdt}")
    for s in range(-(-r // 16)):
        w = min(16, r - 16 * s)
        fs = f[:, :, 16 * s:16 * s + w].contiguous()
        o16 = torch.empty(B, M, w, device=DEV)
        _run_planes(hi, lo, fs, o16, w)
        assert torch.equal(got[:, :, 16 * s:16 * s + w], o16), f"column block {s} differs from the 16-column launch"
    again = torch.empty(B, M, r, device=DEV)
    _run_planes(hi, lo, f, again, r)
    assert torch.equal(again, got)


def test_planes_product_refuses_81_columns():
    hi = torch.zeros(1, 32, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(Exception):
        _run_planes(hi, hi.clone(), torch.zeros(1, 64, 81, device=DEV), torch.zeros(1, 32, 81, device=DEV), 81)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- Cholesky inverse and CholeskyQR3
@pytest.mark.parametrize("l", [33, 48, 64, 80])
def test_chol_inverse_up_to_80(l):
    """L^{-1} (G) L^{-T} = I for the Gram matrix of a random [700, l] block, batch 3, with the numbers of
    tests/test_gpu_parity_r2.py::test_batched_rowdot_colreduce_and_cholesky_qr (1e-4, strict upper triangle exactly zero); a
    rank-deficient Gram matrix gives zero rows and columns for the dropped pivots and nothing non-finite."""
    g = torch.Generator().manual_seed(l)
    y = torch.randn(3, 700, l, generator=g).to(DEV)
    gram = torch.bmm(y.transpose(1, 2), y).contiguous()
    out = MG.Guarded((3, l, l), torch.float32, DEV)
    linv = _C.chol_inverse_batched(gram, 0.0, out=out.data)
    torch.cuda.synchronize()
    out.check(f"chol_inverse l={l}")
    MG.assert_written(linv, "chol_inverse")
    eye = torch.bmm(torch.bmm(linv, gram), linv.transpose(1, 2))
    assert float((eye - torch.eye(l, device=DEV)).abs().max()) < 1e-4
    assert float(linv.triu(1).abs().max()) == 0
    # columns 5 and l - 2 repeat columns 0 and 1: their pivots vanish and are dropped
    yd = y[:1].clone()
    yd[:, :, 5], yd[:, :, l - 2] = yd[:, :, 0], yd[:, :, 1]
    gd = torch.bmm(yd.transpose(1, 2), yd).contiguous()
    ld = _C.chol_inverse_batched(gd, 0.0)
    assert bool(torch.isfinite(ld).all())
    for j in (5, l - 2):
        assert float(ld[0, j].abs().max()) == 0 and float(ld[0, :, j].abs().max()) == 0
    keep = [j for j in range(l) if j not in (5, l - 2)]
    eye = (ld[0] @ gd[0] @ ld[0].t())[keep][:, keep]
    assert float((eye - torch.eye(l - 2, device=DEV)).abs().max()) < 1e-4


def test_chol_inverse_up_to_32_keeps_the_one_wave_kernel_bits():
    """l = 16 and l = 32 run the one-wave kernel.  Pinned by construction inside the test: with no shift the factorisation of
    blockdiag(G16, G32) is the two factorisations side by side (every cross term is an exact x - 0 y), so the 48-wide launch,
    which runs the workgroup kernel, must reproduce the one-wave kernel's L^{-1} of either block bit for bit — and does so
    only while both kernels keep the same f64 arithmetic in the same order."""
    g = torch.Generator().manual_seed(5)
    y16, y32 = torch.randn(2, 700, 16, generator=g).to(DEV), torch.randn(2, 700, 32, generator=g).to(DEV)
    g16, g32 = torch.bmm(y16.transpose(1, 2), y16).contiguous(), torch.bmm(y32.transpose(1, 2), y32).contiguous()
    l16, l32 = _C.chol_inverse_batched(g16, 0.0), _C.chol_inverse_batched(g32, 0.0)
    for lin, gr, l in ((l16, g16, 16), (l32, g32, 32)):   # the one-wave kernel as the existing tests know it
        eye = torch.bmm(torch.bmm(lin, gr), lin.transpose(1, 2))
        assert float((eye - torch.eye(l, device=DEV)).abs().max()) < 1e-4
    g48 = torch.zeros(2, 48, 48, device=DEV)
    g48[:, :16, :16], g48[:, 16:, 16:] = g16, g32
    l48 = _C.chol_inverse_batched(g48, 0.0)
    assert torch.equal(l48[:, :16, :16], l16) and torch.equal(l48[:, 16:, 16:], l32)
    assert float(l48[:, 16:, :16].abs().max()) == 0 and float(l48[:, :16, 16:].abs().max()) == 0


def test_cholesky_qr3_at_80_columns():
    """The orthonormalisation of the wide path (Gram matrix, ``chol_inverse_batched``, Y L^{-T}; shifted first pass, two clean
    ones) on the ill-conditioned block of test_batched_rowdot_colreduce_and_cholesky_qr at [700, 80]: columns spanning 3.5
    orders of magnitude of singular values; its bounds (5e-5, 1e-3)."""
    g = torch.Generator().manual_seed(0)
    B, N, l = 3, 700, 80
    u, _ = torch.linalg.qr(torch.randn(B, N, l, generator=g))
    v, _ = torch.linalg.qr(torch.randn(B, l, l, generator=g))
    ill = ((u * torch.logspace(0, -3.5, l)) @ v.transpose(1, 2)).to(DEV).contiguous()
    q = S._orth(ill)
    qtq = torch.bmm(q.transpose(1, 2), q)
    assert float((qtq - torch.eye(l, device=DEV)).abs().max()) < 5e-5
    proj = torch.bmm(q, torch.bmm(q.transpose(1, 2), ill))
    assert float((proj - ill).norm()) <= 1e-3 * float(ill.norm())


# ----------------------------------------------------------------------------- end to end
def _planted(N, K, r, seed):
    """(tuned, base) on the CPU: residual of rank r + 4 with singular values 0.6 0.95^i plus noise of singular values ~1e-3."""
    g = torch.Generator().manual_seed(seed)
    k = r + 4
    u, _ = torch.linalg.qr(torch.randn(N, k, generator=g))
    v, _ = torch.linalg.qr(torch.randn(K, k, generator=g))
    sv = 0.6 * 0.95 ** torch.arange(k, dtype=torch.float32)
    base = torch.randn(N, K, generator=g) * 0.05
    res = (u * sv) @ v.t() + 1e-3 / (N ** 0.5 + K ** 0.5) * torch.randn(N, K, generator=g)
    return base + res, base


class _routes:
    """``cli_svd.ROUTES`` counted over the block, and every matrix ``torch.linalg.svd`` saw."""

    def __enter__(self):
        self.before = dict(S.ROUTES)
        self.seen = []
        self._svd = torch.linalg.svd

        def spy(a, *args, **kw):
            self.seen.append(tuple(a.shape))
            return self._svd(a, *args, **kw)
        torch.linalg.svd = spy
        return self

    def __exit__(self, *a):
        torch.linalg.svd = self._svd
        self.routes = {k: S.ROUTES[k] - v for k, v in self.before.items() if S.ROUTES[k] != v}


E2E = [(96, 128, 64), (320, 768, 17), (320, 768, 32), (640, 320, 48), (1280, 320, 64)]


@pytest.mark.parametrize("N,K,r", E2E)
def test_wide_distillation_matches_exact(N, K, r):
    """``topr_svd`` / ``distill_pair`` at ranks 17..64 with the assertions of
    tests/test_cli_svd.py::test_device_randomized_svd_matches_exact (singular values rtol 1e-3, product within 5e-3 of the exact
    truncation, both factors orthonormal to 1e-4), and the clamp against the reference recipe on the CPU with the bounds of
    tests/test_gpu_parity_r2.py::test_distill_pair_on_device_vs_reference_recipe_including_clamp (threshold of the sign-aligned
    factors and their clamped product within 5e-3, threshold under the device's own sign rule within 0.1).  Every site takes
    the wide route and no ``torch.linalg.svd`` call sees more than the l x l core."""
    tuned, base = _planted(N, K, r, 1)
    res = (tuned - base).float()
    l = 16 * -(-(r + 8) // 16)
    with _routes() as rt:
        U, Sg, Vh = S.topr_svd(res.to(DEV), r, generator=torch.Generator(device=DEV).manual_seed(0))
        up, down = S.distill_pair(tuned.to(DEV), base.to(DEV), r, 0.99, generator=torch.Generator(device=DEV).manual_seed(0))
    assert rt.routes == {"wide_planes": 2}, rt.routes
    assert rt.seen and all(max(sh[-2:]) <= l for sh in rt.seen), rt.seen
    Ue, Se, Vhe = torch.linalg.svd(res, full_matrices=False)
    floor = 1e-3
    sig = Se[:r] > 10 * floor
    assert bool(sig.all())
    assert torch.allclose(Sg.cpu()[sig], Se[:r][sig], rtol=1e-3, atol=1e-6), (Sg.cpu(), Se[:r])
    assert torch.allclose(Sg.cpu(), Se[:r], rtol=0.1, atol=floor)
    approx = (U @ torch.diag(Sg) @ Vh).cpu()
    exact = Ue[:, :r] @ torch.diag(Se[:r]) @ Vhe[:r]
    rel = float((approx - exact).norm() / exact.norm())
    print(f"wide {N}x{K} r{r}: product {rel:.3e}, singular values {float(((Sg.cpu() - Se[:r]) / Se[:r]).abs().max()):.3e}")
    assert rel <= 5e-3
    assert torch.allclose(U.t() @ U, torch.eye(r, device=DEV), atol=1e-4)
    assert torch.allclose(Vh @ Vh.t(), torch.eye(r, device=DEV), atol=1e-4)
    # the clamp (ref cli_svd.py:39-47) against the recipe on the CPU
    U_ref, Vh_ref = Ue[:, :r] * Se[:r], Vhe[:r]
    hi_ref = float(torch.quantile(torch.cat([U_ref.flatten(), Vh_ref.flatten()]), 0.99))
    Us, Vs = (U * Sg).cpu(), Vh.cpu()
    sgn = torch.sign((Vs * Vh_ref).sum(1))
    Ua, Vha = Us * sgn[None, :], Vs * sgn[:, None]
    hi_al = float(torch.quantile(torch.cat([Ua.flatten(), Vha.flatten()]), 0.99))
    assert abs(hi_al - hi_ref) <= 5e-3 * hi_ref
    prod_ref = U_ref.clamp(-hi_ref, hi_ref) @ Vh_ref.clamp(-hi_ref, hi_ref)
    prod_al = Ua.clamp(-hi_al, hi_al) @ Vha.clamp(-hi_al, hi_al)
    assert float((prod_al - prod_ref).norm()) <= 5e-3 * float(prod_ref.norm())
    hi_native = float(torch.quantile(torch.cat([Us.flatten(), Vs.flatten()]), 0.99))
    assert abs(hi_native - hi_ref) <= 0.1 * hi_ref
    assert up.shape == (N, r) and down.shape == (r, K)
    assert float(up.abs().max()) <= hi_native * (1 + 1e-6) and float(down.abs().max()) <= hi_native * (1 + 1e-6)
    assert float(((up @ down).cpu() - prod_ref).norm()) <= 0.05 * float(prod_ref.norm())


def test_ragged_model_of_three_shape_groups_at_rank_32():
    """``distill_model`` over three shape groups at rank 32 (one wide iteration for all of them, residuals and planes from one
    launch) equals ``distill_group`` group by group.  The two draw different sketches, so "equals" is the rank-r product: each
    is within the iteration's error of the exact truncation, 1e-4 as test_distill_group_equals_per_site_recipe_on_device asks."""
    shapes = [(2, 320, 320), (1, 640, 96), (2, 64, 576)]
    groups = []
    for gi, (B, N, K) in enumerate(shapes):
        tb = [_planted(N, K, 32, 10 * gi + i) for i in range(B)]
        groups.append(([t.to(DEV) for t, _ in tb], [b.to(DEV) for _, b in tb]))
    with _routes() as rt:
        res = S.distill_model(groups, 32, generator=torch.Generator(device=DEV).manual_seed(0))
    assert rt.routes == {"wide_planes": 5}, rt.routes
    assert all(max(sh[-2:]) <= 48 for sh in rt.seen), rt.seen
    for (tuned, base), (up, down), (B, N, K) in zip(groups, res, shapes):
        assert up.shape == (B, N, 32) and down.shape == (B, 32, K)
        up1, down1 = S.distill_group(tuned, base, 32, generator=torch.Generator(device=DEV).manual_seed(1))
        p, p1 = torch.bmm(up, down), torch.bmm(up1, down1)
        assert float((p - p1).norm()) <= 1e-4 * float(p1.norm())


def test_routes_of_odd_shapes_and_of_the_switch():
    """A site whose K is no multiple of 32 takes the exact SVD at rank 32; with ``WIDE`` off so does every site of rank 64."""
    tuned, base = _planted(320, 328, 32, 3)
    with _routes() as rt:
        up, down = S.distill_pair(tuned.to(DEV), base.to(DEV), 32)
    assert rt.routes == {"exact": 1} and rt.seen == [(320, 328)]
    assert up.shape == (320, 32) and bool(torch.isfinite(up).all())
    tuned, base = _planted(96, 128, 64, 4)
    prev, S.WIDE = S.WIDE, False
    try:
        with _routes() as rt:
            S.distill_pair(tuned.to(DEV), base.to(DEV), 64)
    finally:
        S.WIDE = prev
    assert rt.routes == {"exact": 1}
    with _routes() as rt:
        S.distill_pair(tuned.to(DEV), base.to(DEV), 64)
    assert rt.routes == {"wide_planes": 1}


def test_svd_distill_cli_at_rank_32(tmp_path):
    out = str(tmp_path / "d.safetensors")
    S.svd_distill("standin:1", "standin:2", rank=32, device=DEV, save_path=out)
    loras = L.load_safeloras(out)
    assert set(loras) == {"unet", "text_encoder"}
    ups, ranks = loras["unet"][0][0::2], loras["unet"][1]
    assert ups and all(rk == 32 for rk in ranks)
    assert all(u.shape[1] == 32 and bool(torch.isfinite(u).all()) for u in ups)
    assert max(float(u.detach().abs().max()) for u in ups) > 0
