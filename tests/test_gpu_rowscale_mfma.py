"""Row-table form of the matrix-core rank update (csrc/rank16_mfma.hip rank_update16_mfma_kernel<.., RSC = true>) through
lora_amd_rank_update_rowscale, after the pattern of tests/test_gpu_r16_wide.py::check_rank_update: every case asks
lora_amd_rank_update_rowscale_mfma_takes first, runs the entry with the hook on and off, and holds BOTH results to the float64
restatement want = y0 + s mask . ((T . RS[q]) F), q = (m // rps) % nsel, at tests/test_gpu_kernels.close's own constants (the
per-term arithmetic is that of the plain rank update: bf16 rows, T and F as hi + lo; the f32 multiply by the table adds 2^-24).
Then the two bit rules of the table, and the routes of lora_amd/ops.py and of a LoRAManager that reach the entry."""
import copy
import types

import numpy as np
import pytest
import torch

import lora_amd as L
from lora_amd import _C, ops
from lora_amd.lora_manager import LoRAManager
from lora_amd.standin import tiny_unet
from oracle import lora_numpy as O
from tests.test_gpu_kernels import DEV, close, n, rnd
from tests.test_gpu_per_sample import _conv_case, _err, _oracle_per_sample, _rows
from tests.test_gpu_r16_wide import f64_rk, factor, lay, mask_of
from tests.test_gpu_rank16 import valu

pytestmark = pytest.mark.gpu

RANKS = [9, 16, 17, 32, 40, 64]   # the narrow form's ends; a one-rank last slice, exact slices, a half slice, the maximum
LAYOUTS = ["RK", "KR"]
SEED, OFF, S = 77, (1 << 33) + 5, 1.3


def check(y0, r, layout, p, M, N, nsel, rps):
    t = rnd((M, r), "f32", 0.5, seed=2)
    f = factor(r, N, layout, 3)
    rows = _rows(nsel, r, seed=6)
    assert bool((rows < 0).any()), "the table must hold negative entries"
    assert _C.rank16_mfma(-1) == 1 and _C.rank_update_rowscale_takes(y0, r) == 1
    if y0.is_contiguous():
        y, yv = y0.clone(), y0.clone()
    else:   # views of the caller's row stride, the gap columns pre-filled
        ld = y0.stride(0)
        ya, yb = (torch.full((M, ld), 5.0, dtype=y0.dtype, device=DEV) for _ in range(2))
        ya[:, :N].copy_(y0)
        yb[:, :N].copy_(y0)
        y, yv = ya[:, :N], yb[:, :N]
        assert _C.rank_update_rowscale_takes(y, r) == 1
    _C.rank_update_rowscale_(y, t, f, lay(layout), S, rows, rps, p, SEED, OFF)
    with valu():
        assert _C.rank_update_rowscale_takes(y0, r) == 0
        _C.rank_update_rowscale_(yv, t, f, lay(layout), S, rows, rps, p, SEED, OFF)
    F = f64_rk(f, layout)
    q = (np.arange(M) // rps) % nsel
    ts = n(t).astype(np.float64) * n(rows).astype(np.float64)[q]
    want = n(y0).astype(np.float64) + S * mask_of(M, N, p, SEED, OFF) * (ts @ F)
    bound = np.abs(n(y0)) + S / (1 - p) * (np.abs(ts) @ np.abs(F))
    what = f"{M}x{N} r{r} {layout} p{p} nsel{nsel} rps{rps}"
    print(f"{what}: worst |err| / bound  mfma {np.max(np.abs(n(y) - want) / bound):.3e}  "
          f"valu {np.max(np.abs(n(yv) - want) / bound):.3e}")
    close(n(y), want, bound, "bf16", msg=f"rank_update_rowscale mfma {what}")
    close(n(yv), want, bound, "bf16", msg=f"rank_update_rowscale valu {what}")
    if not y0.is_contiguous():
        assert bool((ya[:, N:] == 5.0).all()) and bool((yb[:, N:] == 5.0).all())


# 5.1: one row; a new table row on every row, a ragged slab and a partial 32-column group; samples that split a slab; the
# % nsel wrap with two samples per table row; samples that straddle workgroup row blocks
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("M,N,nsel,rps", [(1, 320, 1, 1), (33, 328, 3, 1), (100, 648, 4, 13), (462, 320, 3, 77),
                                          (577, 1280, 3, 250)])
def test_rowscale_mfma_vs_float64_and_vs_valu(M, N, nsel, rps, r, layout, p):
    check(rnd((M, N), "bf16", seed=1), r, layout, p, M, N, nsel, rps)


# 5.2: one case per rows-per-workgroup value of the dispatcher (r16_ru_rows; tests/test_gpu_r16_wide.py has the arithmetic):
# 64 rows by the grid rule, 128 rows, 64 rows by the four-slice image
@pytest.mark.parametrize("M,N,r,layout,p", [(9216, 320, 32, "KR", 0.1), (9984, 1280, 17, "RK", 0.1), (9984, 2560, 64, "KR", 0.0)])
def test_rowscale_mfma_rows_per_workgroup(M, N, r, layout, p):
    check(rnd((M, N), "bf16", seed=1), r, layout, p, M, N, 4, 1024)


# 5.3
@pytest.mark.parametrize("r,layout,p", [(40, "KR", 0.1), (64, "RK", 0.0), (9, "RK", 0.1)])
def test_rowscale_mfma_on_a_column_slice(r, layout, p):
    M, N = 100, 648
    wide = rnd((M, N + 64), "bf16", seed=1)
    check(wide[:, :N], r, layout, p, M, N, 4, 13)


# 5.4
@pytest.mark.parametrize("r,p", [(17, 0.1), (64, 0.0)])
def test_rowscale_mfma_two_calls_give_equal_bits(r, p):
    M, N, nsel, rps = 577, 648, 3, 50
    y0, t, f, rows = rnd((M, N), "bf16", seed=1), rnd((M, r), "f32", 0.5, seed=2), factor(r, N, "KR", 3), _rows(nsel, r, 6)
    assert _C.rank_update_rowscale_takes(y0, r) == 1
    a, b = y0.clone(), y0.clone()
    _C.rank_update_rowscale_(a, t, f, _C.FACTOR_KR, S, rows, rps, p, SEED, OFF)
    _C.rank_update_rowscale_(b, t, f, _C.FACTOR_KR, S, rows, rps, p, SEED, OFF)
    assert torch.equal(a, b) and not torch.equal(a, y0)


# 5.5
def _no_zeros(*ts):
    for t in ts:
        assert not bool((t == 0).any())


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("r", [16, 40, 64])
def test_all_ones_table_gives_the_bits_of_the_plain_matrix_core_launch(r, layout, p):
    M, N, nsel, rps = 462, 328, 4, 77
    y0, t, f = rnd((M, N), "bf16", seed=1), rnd((M, r), "f32", 0.5, seed=2), factor(r, N, layout, 3)
    _no_zeros(y0, t, f)
    assert _C.rank16_mfma(-1) == 1 and _C.rank16_mfma_takes(1, y0, r) == 1 and _C.rank_update_rowscale_takes(y0, r) == 1
    ref, y = y0.clone(), y0.clone()
    _C.rank_update_(ref, t, f, lay(layout), S, p, SEED, OFF)
    _C.rank_update_rowscale_(y, t, f, lay(layout), S, torch.ones((nsel, r), device=DEV), rps, p, SEED, OFF)
    assert torch.equal(y, ref) and not torch.equal(y, y0)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("r", [16, 40, 64])
def test_power_of_two_rows_give_the_plain_bits_at_scale_c(r, layout):
    """p = 0: a row of the table that is a constant c in {1, 0.5, 2, 0} scales T's hi + lo split, the products and their sums
    exactly, so every sample's rows are the plain launch on that row range at scale * c."""
    M, N, rps = 462, 328, 77
    c = [1.0, 0.5, 2.0, 0.0]
    y0, t, f = rnd((M, N), "bf16", seed=1), rnd((M, r), "f32", 0.5, seed=2), factor(r, N, layout, 3)
    _no_zeros(y0, t, f)
    rows = torch.tensor(c, device=DEV)[:, None].expand(4, r).contiguous()
    assert _C.rank16_mfma(-1) == 1 and _C.rank_update_rowscale_takes(y0, r) == 1
    y = y0.clone()
    _C.rank_update_rowscale_(y, t, f, lay(layout), S, rows, rps)
    for m0 in range(0, M, rps):
        cb = c[(m0 // rps) % 4]
        want = y0[m0:m0 + rps].clone()
        assert _C.rank16_mfma_takes(1, want, r) == 1
        _C.rank_update_(want, t[m0:m0 + rps].contiguous(), f, lay(layout), S * cb)
        assert torch.equal(y[m0:m0 + rps], want), f"sample at row {m0} (multiplier {cb})"
        assert torch.equal(want, y0[m0:m0 + rps]) == (cb == 0.0)


# 5.6: the routes
class Spy:
    """Records, for every ``_C.rank_update_rowscale_`` call, (dtype, N, the predicate on the live tensors), and for every
    ``_C.rowdot`` call whether its matrix-core form took it."""

    def __init__(self, monkeypatch):
        self.updates, self.rowdots = [], []
        ru, rd = _C.rank_update_rowscale_, _C.rowdot

        def rank_update_rowscale_(y, t, f, *a, **k):
            self.updates.append((y.dtype, y.shape[1], _C.rank_update_rowscale_takes(y, t.shape[1], f.dtype)))
            return ru(y, t, f, *a, **k)

        def rowdot(x, f, layout, scale=1.0, sel=None, *a, **k):
            r = f.shape[0] if layout == _C.FACTOR_RK else f.shape[1]
            self.rowdots.append(_C.rank16_mfma_takes(0, x, r, f.dtype, sel is not None))
            return rd(x, f, layout, scale, sel, *a, **k)

        monkeypatch.setattr(_C, "rank_update_rowscale_", rank_update_rowscale_)
        monkeypatch.setattr(_C, "rowdot", rowdot)


def _linear_site(r):
    rps, K, N = 77, 768, 320
    M = 6 * rps  # [6, 77, K]: six text-token samples, two per row of the table
    x, w, b = rnd((M, K), "bf16", 1.0, seed=1), rnd((N, K), "bf16", 0.05, seed=2), rnd((N,), "bf16", 0.5, seed=3)
    down, up = rnd((r, K), "f32", 0.2, seed=4), rnd((N, r), "f32", 0.3, seed=5)
    return rps, K, N, M, x, w, b, down, up


@pytest.mark.parametrize("r", [12, 24, 48, 64, 96])
def test_linear_per_sample_route_runs_the_row_table_form(r, monkeypatch):
    rps, K, N, M, x, w, b, down, up = _linear_site(r)
    rows = _rows(3, r, seed=6)
    spy = Spy(monkeypatch)
    y = ops.lora_linear_per_sample(x.view(6, rps, K), w, b, down, up, None, 0.7, 0.0, rows).reshape(M, N)
    assert all(u == (torch.bfloat16, N, 1) for u in spy.updates), spy.updates
    if r > 16:  # past the ring kernel: the library route, one launch per rank chunk of <= 64
        assert len(spy.updates) == (r + 63) // 64
    X, W, Bv, A, U, RS = n(x), n(w), n(b), n(down), n(up), n(rows)
    y_ref, _, q = _oracle_per_sample(X, W, Bv, A, U, 0.7, RS, rps)
    branch = (np.abs(X @ A.T) * np.abs(RS[q])) @ (0.7 * np.abs(U)).T
    k = 2e-3
    absref = np.abs(X) @ np.abs(W).T + np.abs(Bv) + (1.0 + 2.0 ** -8 / k) * branch
    close(n(y), y_ref, absref, "bf16", k=k, msg=f"Y r{r}")


@pytest.mark.parametrize("r", [12, 40])
def test_linear_per_sample_with_a_module_selector_keeps_the_row_product_on_the_matrix_cores(r, monkeypatch):
    """A general [r, r] selector and an alpha-only table (scale 1, every entry of table row s is alpha_s): the row product
    runs without the selector, which is applied to the [M, r] result."""
    rps, K, N, M, x, w, b, down, up = _linear_site(r)
    sel = rnd((r, r), "f32", 0.4, seed=7)
    alphas = torch.tensor([0.5, -0.25, 1.5], device=DEV)
    rows = alphas[:, None].expand(3, r).contiguous()
    spy = Spy(monkeypatch)
    y = ops.lora_linear_per_sample(x.view(6, rps, K), w, b, down, up, sel, 1.0, 0.0, rows).reshape(M, N)
    assert spy.rowdots == [1], spy.rowdots
    assert spy.updates == [(torch.bfloat16, N, 1)], spy.updates
    X, W, Bv, A, U, Sm = n(x), n(w), n(b), n(down), n(up), n(sel)
    q = (np.arange(M) // rps) % 3
    y_ref = np.empty((M, N), np.float32)
    for s in range(3):
        y_ref[q == s], _ = O.lora_linear_forward(X[q == s], W, Bv, A, U, 1.0, selector=float(alphas[s]) * Sm)
    branch = ((np.abs(X @ A.T) @ np.abs(Sm).T) * np.abs(n(alphas))[q][:, None]) @ np.abs(U).T
    k = 2e-3
    absref = np.abs(X) @ np.abs(W).T + np.abs(Bv) + (1.0 + 2.0 ** -8 / k) * branch
    close(n(y), y_ref, absref, "bf16", k=k, msg=f"Y r{r} with a selector")


@pytest.mark.parametrize("r", [12, 32, 64])
def test_conv3_nhwc_site_per_sample(r, monkeypatch):
    nsel = 3
    m, x = _conv_case("nhwc", 3, r, nsel)
    assert m.conv.weight.shape[:2] == (96, 64)
    rows = _rows(nsel, r, seed=7)
    L.set_lora_diag_per_sample(torch.nn.Sequential(m), rows)
    spy = Spy(monkeypatch)
    with torch.no_grad():
        y = m(x)
    assert y.shape == (x.shape[0], 96, 16, 16)
    assert spy.updates and all(u == (torch.bfloat16, 96, 1) for u in spy.updates), spy.updates
    X, W, Bv, A, U = n(x), n(m.conv.weight), n(m.conv.bias), n(m.lora_down.weight), n(m.lora_up.weight)
    for b in range(x.shape[0]):
        Sd = np.diag(n(rows)[b % nsel])
        want, _ = O.lora_conv2d_forward(X[b:b + 1], W, Bv, A, U, 0.6, padding=(1, 1), selector=Sd)
        absref, _ = O.lora_conv2d_forward(np.abs(X[b:b + 1]), np.abs(W), np.abs(Bv), np.abs(A), np.abs(U), 0.6,
                                          padding=(1, 1), selector=np.abs(Sd))
        close(n(y[b:b + 1]), want, absref, "bf16", k=4e-3, msg=f"nhwc 3x3 r{r} sample {b}")


# 5.7: a UNet
UNET_MIXES = [[1.0, 0.0], [0.5, 2.0], [-0.5, 1.0], [0.0, 0.0]]   # a one-hot row, two general rows, a zero row


def _manager_pipe(tmp_path, ranks=(8, 12)):
    """tests/test_gpu_per_sample._manager_pipe with members of rank 8 and 12: joined rank 20, a ragged second slice."""
    paths = []
    for i, r in enumerate(ranks):
        torch.manual_seed(i + 1)
        unet = tiny_unet()
        L.inject_trainable_lora(unet, r=r)
        for up, _ in L.extract_lora_ups_down(unet):
            up.weight.data.normal_(0, 0.05)
        p = str(tmp_path / f"m{i}.safetensors")
        L.save_safeloras({"unet": (unet, L.UNET_DEFAULT_TARGET_REPLACE)}, p)
        paths.append(p)
    torch.manual_seed(0)
    pipe = types.SimpleNamespace(unet=tiny_unet(), text_encoder=torch.nn.Identity(), tokenizer=None)
    mgr = LoRAManager(paths, pipe)
    pipe.unet.to(DEV).to(torch.bfloat16).eval()
    for m in pipe.unet.modules():  # factors stay f32 masters (what injection on a device model gives)
        if type(m).__name__ == "LoraInjectedLinear":
            m.lora_down.weight.data = m.lora_down.weight.data.float()
            m.lora_up.weight.data = m.lora_up.weight.data.float()
    return mgr, pipe


@torch.no_grad()
def test_manager_tune_per_sample_on_unet_at_joined_rank_20(tmp_path, monkeypatch):
    """The bracket of tests/test_gpu_per_sample.py::test_manager_tune_per_sample_on_unet (batch 8 = 4 mixes x 2) at joined rank
    20, with the hook on and off: against the same model in f32, the per-sample batch must be as close as today's bf16
    routes are.  With the hook on, every rank_update_rowscale_ call on bf16 rows with N % 8 == 0 runs the row-table form."""
    mgr, pipe = _manager_pipe(tmp_path)
    assert list(mgr.ranklist) == [8, 12]
    m32 = copy.deepcopy(pipe.unet).float()
    torch.manual_seed(3)
    cfg, B = 2, 8
    x = torch.randn(B, 4, 64, 64, device=DEV, dtype=torch.bfloat16)
    t = torch.full((B,), 500, device=DEV)
    ehs = torch.randn(B, 7, 32, device=DEV, dtype=torch.bfloat16)
    mgr.tune_per_sample(UNET_MIXES)
    spy = Spy(monkeypatch)
    ys = {}
    for hook in (1, 0):
        prev = _C.rank16_mfma(hook)
        try:
            del spy.updates[:]
            ys[hook] = pipe.unet(x, t, ehs).sample
            took = [u for u in spy.updates if u[0] == torch.bfloat16 and u[1] % 8 == 0]
            assert took and all(u[2] == hook for u in took), (hook, spy.updates)
        finally:
            _C.rank16_mfma(prev)
    L.clear_lora_per_sample(pipe.unet)
    rows = []
    for q, mix in enumerate(UNET_MIXES):
        idx = [q + 4 * c for c in range(cfg)]
        mgr.tune(mix)
        L.set_lora_diag(m32, torch.repeat_interleave(torch.tensor(mix), torch.tensor(mgr.ranklist)))
        ref = m32(x[idx].float(), t[idx], ehs[idx].float()).sample
        today = pipe.unet(x[idx], t[idx], ehs[idx]).sample
        whole = pipe.unet(x, t, ehs).sample[idx]
        rows.append((_err(ys[1][idx], ref), _err(ys[0][idx], ref), _err(today, ref), _err(whole, ref)))
    plain = copy.deepcopy(pipe.unet)
    L.monkeypatch_remove_lora(plain)
    ref0 = copy.deepcopy(plain).float()(x[3::4].float(), t[3::4], ehs[3::4].float()).sample
    e_plain = _err(plain(x[3::4], t[3::4], ehs[3::4]).sample, ref0)
    print("errors against f32 (hook on, hook off, today, whole batch):", rows, "zero row:",
          _err(ys[1][3::4], ref0), _err(ys[0][3::4], ref0), e_plain)
    for q, (e_on, e_off, e_today, e_whole) in enumerate(rows):
        bracket = max(e_today, e_whole)
        assert bracket < 5e-2, (q, rows)  # the bf16 runs themselves are sane
        assert e_on <= 1.25 * bracket and e_off <= 1.25 * bracket, (q, rows)
    for hook in (1, 0):
        assert _err(ys[hook][3::4], ref0) <= 1.25 * max(e_plain, max(r[2] for r in rows)), (hook, rows)
