"""Wide forms (ranks 17..64) of the matrix-core row product and rank update (csrc/rank16_mfma.hip) through the C ABI, after the
pattern of tests/test_gpu_rank16.py: every case asks lora_amd_rank16_mfma_takes first, runs the entry point with the hook on and
off, and holds BOTH results to the float64 restatement at tests/test_gpu_kernels.close's own constants — the per-term
arithmetic (bf16 data, factor hi + lo) and the sum lengths are those of ranks 9..16.  The dropout mask is rebuilt by
tests/helpers.philox_dropout_mask."""
import numpy as np
import pytest
import torch

import lora_amd as L
from lora_amd import _C, ops
from lora_amd import trainer as T
from tests import helpers as H
from tests import memguard as MG
from tests.test_gpu_kernels import DEV, close, n, rnd
from tests.test_gpu_rank16 import valu

pytestmark = pytest.mark.gpu

RANKS = [17, 32, 40, 64]   # a one-rank last slice, exact slices, a half slice, the maximum
LAYOUTS = ["RK", "KR"]
ROWDOT, RANK_UPDATE = 0, 1


def mask_of(M, N, p, seed, off):
    if p == 0.0:
        return np.ones((M, N), np.float64)
    return H.philox_dropout_mask(M * N, p, seed, off, device=DEV).view(M, N).double().cpu().numpy()


def lay(layout):
    return _C.FACTOR_RK if layout == "RK" else _C.FACTOR_KR


def factor(r, C, layout, seed, scale=0.3):
    return rnd((r, C) if layout == "RK" else (C, r), "f32", scale, seed=seed)


def f64_rk(f, layout):
    F = n(f).astype(np.float64)
    return F if layout == "RK" else F.T


def check_rowdot(x, r, layout, p, M, C):
    f = factor(r, C, layout, 2)
    seed, off, s = 0x51ED5EED, 12345, 0.7
    assert _C.rank16_mfma(-1) == 1 and _C.rank16_mfma_takes(ROWDOT, x, r) == 1
    got = _C.rowdot(x, f, lay(layout), s, None, False, p, seed, off)
    with valu():
        assert _C.rank16_mfma_takes(ROWDOT, x, r) == 0
        old = _C.rowdot(x, f, lay(layout), s, None, False, p, seed, off)
    F = f64_rk(f, layout)
    xm = n(x).astype(np.float64) * mask_of(M, C, p, seed, off)
    want = s * (xm @ F.T)
    bound = s * (np.abs(xm) @ np.abs(F.T))
    close(n(got), want, bound, msg=f"rowdot16 wide {M}x{C} r{r} {layout} p{p}")
    close(n(old), want, bound, msg=f"rowdot valu {M}x{C} r{r} {layout} p{p}")


# single k-step / single row / ragged slab (one wave per slab); several slabs per workgroup (two waves per slab); several
# workgroups (eight waves per slab); short stacks of long rows (the cross-wave meeting at its widest: 16 waves per slab)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("M,C", [(1, 32), (17, 96), (33, 320), (577, 1280), (33, 2560), (144, 10240)])
def test_rowdot_wide_vs_float64_and_vs_valu(M, C, r, layout, p):
    check_rowdot(rnd((M, C), "bf16", seed=1), r, layout, p, M, C)


@pytest.mark.parametrize("r,layout,p", [(40, "KR", 0.1), (64, "RK", 0.0)])
def test_rowdot_wide_on_a_column_slice(r, layout, p):
    M, C = 100, 640
    wide = rnd((M, C + 64), "bf16", seed=1)
    check_rowdot(wide[:, :C], r, layout, p, M, C)


@pytest.mark.parametrize("r,layout,p", [(32, "KR", 0.1), (64, "RK", 0.1)])
def test_rowdot_wide_many_rows(r, layout, p):
    check_rowdot(rnd((9216, 320), "bf16", seed=1), r, layout, p, 9216, 320)


def check_rank_update(y0, r, layout, p, M, N):
    t = rnd((M, r), "f32", 0.5, seed=2)
    f = factor(r, N, layout, 3)
    seed, off, s = 77, (1 << 33) + 5, 1.3
    assert _C.rank16_mfma(-1) == 1 and _C.rank16_mfma_takes(RANK_UPDATE, y0, r) == 1
    if y0.is_contiguous():
        y, yv = y0.clone(), y0.clone()
    else:   # views of the caller's row stride, the gap columns pre-filled
        ld = y0.stride(0)
        ya, yb = (torch.full((M, ld), 5.0, dtype=y0.dtype, device=DEV) for _ in range(2))
        ya[:, :N].copy_(y0)
        yb[:, :N].copy_(y0)
        y, yv = ya[:, :N], yb[:, :N]
    _C.rank_update_(y, t, f, lay(layout), s, p, seed, off)
    with valu():
        assert _C.rank16_mfma_takes(RANK_UPDATE, y0, r) == 0
        _C.rank_update_(yv, t, f, lay(layout), s, p, seed, off)
    F = f64_rk(f, layout)
    prod = n(t).astype(np.float64) @ F
    want = n(y0).astype(np.float64) + s * mask_of(M, N, p, seed, off) * prod
    bound = np.abs(n(y0)) + s / (1 - p) * (np.abs(n(t)) @ np.abs(F))
    close(n(y), want, bound, "bf16", msg=f"rank_update16 wide {M}x{N} r{r} {layout} p{p}")
    close(n(yv), want, bound, "bf16", msg=f"rank_update valu {M}x{N} r{r} {layout} p{p}")
    if not y0.is_contiguous():
        assert bool((ya[:, N:] == 5.0).all()) and bool((yb[:, N:] == 5.0).all())


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("M,N", [(1, 320), (33, 328), (100, 648), (577, 1280)])
def test_rank_update_wide_vs_float64_and_vs_valu(M, N, r, layout, p):
    check_rank_update(rnd((M, N), "bf16", seed=1), r, layout, p, M, N)


# One case per rows-per-workgroup value of the wide dispatcher (r16_ru_rows: the T image of ns = ceil(r / 16) slices holds
# 256 / ns rounded down to a power of two rows, halved down to 64 while fewer than 768 workgroups would start):
#   r = 32 (2 slices), 9216 x 320:  72 x 3 workgroups of 128 rows < 768           -> 64 rows
#   r = 17 (2 slices), 9984 x 1280: 78 x 10 workgroups of 128 rows >= 768         -> 128 rows
#   r = 64 (4 slices), 9984 x 2560: the image holds 64 rows, whatever the grid    -> 64 rows (maskless: the host-side mask)
@pytest.mark.parametrize("M,N,r,layout,p", [(9216, 320, 32, "KR", 0.1), (9984, 1280, 17, "RK", 0.1), (9984, 2560, 64, "KR", 0.0)])
def test_rank_update_wide_rows_per_workgroup(M, N, r, layout, p):
    check_rank_update(rnd((M, N), "bf16", seed=1), r, layout, p, M, N)


@pytest.mark.parametrize("r,layout,p", [(40, "KR", 0.1), (64, "RK", 0.0)])
def test_rank_update_wide_on_a_column_slice(r, layout, p):
    M, N = 100, 648
    wide = rnd((M, N + 64), "bf16", seed=1)
    check_rank_update(wide[:, :N], r, layout, p, M, N)


# ----------------------------------------------------------------------------- zero padding: the bits of the rank-16 kernel
def _pad_factor(f, layout, r):
    if layout == "RK":
        out = torch.zeros((r, f.shape[1]), device=DEV)
        out[:16] = f
    else:
        out = torch.zeros((f.shape[0], r), device=DEV)
        out[:, :16] = f
    return out


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,N", [(100, 648), (577, 1280)])
def test_rank_update_of_zero_padded_ranks_gives_the_bits_of_the_rank_16_kernel(M, N, layout, p):
    """The slices chain into the narrow kernel's two accumulators, slice 0 first: ranks whose factor rows are zero change no
    bit, whatever T holds there."""
    y0, t16 = rnd((M, N), "bf16", seed=1), rnd((M, 16), "f32", 0.5, seed=2)
    f16 = factor(16, N, layout, 3)
    seed, off, s = 77, (1 << 33) + 5, 1.3
    assert _C.rank16_mfma(-1) == 1
    ref = y0.clone()
    _C.rank_update_(ref, t16, f16, lay(layout), s, p, seed, off)
    for r in (32, 64):
        t = rnd((M, r), "f32", 0.5, seed=4)
        t[:, :16] = t16
        y = y0.clone()
        assert _C.rank16_mfma_takes(RANK_UPDATE, y, r) == 1
        _C.rank_update_(y, t.contiguous(), _pad_factor(f16, layout, r), lay(layout), s, p, seed, off)
        assert torch.equal(y, ref), r


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", [32, 96])
def test_rowdot_of_zero_padded_ranks_gives_the_bits_of_the_rank_16_kernel(C, layout, p):
    """Rows this short are never split across waves: slice 0 of the wide kernel runs the narrow kernel's chain."""
    M = 100
    x, f16 = rnd((M, C), "bf16", seed=1), factor(16, C, layout, 2)
    seed, off, s = 0x51ED5EED, 12345, 0.7
    assert _C.rank16_mfma(-1) == 1
    ref = _C.rowdot(x, f16, lay(layout), s, None, False, p, seed, off)
    for r in (32, 64):
        assert _C.rank16_mfma_takes(ROWDOT, x, r) == 1
        got = _C.rowdot(x, _pad_factor(f16, layout, r), lay(layout), s, None, False, p, seed, off)
        assert torch.equal(got[:, :16], ref), r
        assert not bool(got[:, 16:].any()), r


# ----------------------------------------------------------------------------- footprint
@pytest.mark.parametrize("layout", LAYOUTS)
def test_wide_footprint_with_guards_and_poisoned_sources(layout):
    """T of (33, 40) and Y of (33, 328) at row stride 392 in guarded allocations pre-filled with the sentinel NaN; X, T (as an
    input) and the factors in poisoned ones.  Guards intact, no NaN in the written set, Y's gap columns untouched."""
    M, C, N, r, p = 33, 320, 328, 40, 0.1
    assert _C.rank16_mfma(-1) == 1
    x = MG.poisoned(rnd((M, C), "bf16", seed=1), ld=C + 64)
    fd = MG.poisoned(factor(r, C, layout, 2))
    t_out = MG.Guarded((M, r), torch.float32, DEV)
    assert _C.rank16_mfma_takes(ROWDOT, x, r) == 1
    _C.rowdot(x, fd, lay(layout), 0.7, None, False, p, 5, 9, out=t_out.data)
    torch.cuda.synchronize()
    t_out.check("rowdot16 wide: T")
    MG.assert_written(t_out.data, "rowdot16 wide: T")
    MG.assert_finite(t_out.data, what="rowdot16 wide: T")

    yg = MG.Guarded((M, N + 64), torch.bfloat16, DEV)
    y = yg.data[:, :N]
    y.copy_(rnd((M, N), "bf16", seed=3))
    t_in = MG.poisoned(rnd((M, r), "f32", 0.5, seed=4))
    fu = MG.poisoned(factor(r, N, layout, 5))
    assert _C.rank16_mfma_takes(RANK_UPDATE, y, r) == 1
    _C.rank_update_(y, t_in, fu, lay(layout), 1.3, p, 5, 9)
    torch.cuda.synchronize()
    yg.check("rank_update16 wide: Y")
    MG.assert_finite(y, what="rank_update16 wide: Y")
    MG.assert_untouched(yg.data[:, N:], "rank_update16 wide: Y's gap columns")


# ----------------------------------------------------------------------------- replay
def test_wide_masked_launches_replay_bit_equal_from_a_device_offset():
    M, C, N, r, p = 144, 2560, 648, 40, 0.1
    x, y0 = rnd((M, C), "bf16", seed=1), rnd((M, N), "bf16", seed=2)
    fd, fu = factor(r, C, "KR", 3), factor(r, N, "KR", 4)
    t_in = rnd((M, r), "f32", 0.5, seed=5)
    off = torch.tensor([(1 << 40) + 17], dtype=torch.int64, device=DEV)
    t_out, y = torch.empty((M, r), device=DEV), y0.clone()
    assert _C.rank16_mfma(-1) == 1
    assert _C.rank16_mfma_takes(ROWDOT, x, r) == 1 and _C.rank16_mfma_takes(RANK_UPDATE, y, r) == 1

    def run():
        _C.rowdot(x, fd, _C.FACTOR_KR, 0.7, None, False, p, 5, off, out=t_out)
        _C.rank_update_(y, t_in, fu, _C.FACTOR_KR, 1.3, p, 5, off)

    run()
    torch.cuda.synchronize()
    eager = (t_out.clone(), y.clone())
    # the device offset is what the kernels read: the host-offset call of the same value draws the same mask
    assert torch.equal(_C.rowdot(x, fd, _C.FACTOR_KR, 0.7, None, False, p, 5, int(off.item())), eager[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(2):
        t_out.fill_(float("nan"))
        y.copy_(y0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(t_out, eager[0]) and torch.equal(y, eager[1]), "a replay differs from the eager launch"


# ----------------------------------------------------------------------------- module
@pytest.fixture
def path_log():
    ops.PATH_LOG = log = []
    yield log
    ops.PATH_LOG = None


def _module(r, p):
    torch.manual_seed(0)
    m = L.LoraInjectedLinear(320, 640, True, r=r, dropout_p=p).to(DEV).to(torch.bfloat16)
    m.linear.requires_grad_(False)
    T.promote_lora_to_fp32(m)
    m.lora_up.weight.data.normal_(0, 0.05)
    return m


def test_wide_dropout_module_forward_backward_on_both_kernels(path_log):
    """LoraInjectedLinear(320, 640, r = 32, dropout 0.1) in bf16 training mode: the route stays lib+primitives / primitives
    with the hook on and off (only what the primitives run on changes); y, dX and both factor gradients of both runs against
    a float64 run of the same formula under the same mask, bounds as in tests/test_gpu_merged_wide.py's module test."""
    r, p, B, S, K, N = 32, 0.1, 2, 77, 320, 640
    M = B * S
    m = _module(r, p).train()
    s = float(m.scale)
    assert float(m.lora_up.weight.detach().abs().max()) > 0
    x0, gy = rnd((B, S, K), "bf16", seed=5), rnd((B, S, N), "bf16", seed=6)
    torch.manual_seed(3)
    seed, off = ops.next_dropout_stream(DEV)
    mask = mask_of(M, N, p, seed, int(off.item()))
    assert 0.05 < float((mask == 0).mean()) < 0.15
    X, G = n(x0).astype(np.float64).reshape(M, K), n(gy).astype(np.float64).reshape(M, N)
    W, b = n(m.linear.weight).astype(np.float64), n(m.linear.bias).astype(np.float64)
    A, U = n(m.lora_down.weight).astype(np.float64), n(m.lora_up.weight).astype(np.float64)
    Tn = X @ A.T
    yo = X @ W.T + b + s * mask * (Tn @ U.T)
    Gm = G * mask
    Gt = s * (Gm @ U)
    dxo, duo, ddo = G @ W + Gt @ A, s * (Gm.T @ Tn), Gt.T @ X
    aT = np.abs(X) @ np.abs(A).T
    absy = np.abs(X) @ np.abs(W).T + np.abs(b) + s / (1 - p) * (aT @ np.abs(U).T)
    aGt = s * (np.abs(Gm) @ np.abs(U))
    absdx = np.abs(G) @ np.abs(W) + aGt @ np.abs(A)
    absu, absd = s * (np.abs(Gm).T @ aT), aGt.T @ np.abs(X)
    for hook in (1, 0):
        prev = _C.rank16_mfma(hook)
        try:
            x = x0.clone().requires_grad_(True)
            m.lora_up.weight.grad = m.lora_down.weight.grad = None
            del path_log[:]
            torch.manual_seed(3)
            y = m(x)
            y.backward(gy)
        finally:
            _C.rank16_mfma(prev)
        assert [(ph, path) for ph, path, *_ in path_log] == [("fwd", "lib+primitives"), ("bwd", "primitives")], path_log
        assert path_log[0][2:] == (M, K, N, r)
        yv, dxv = n(y).reshape(M, N), n(x.grad).reshape(M, K)
        assert np.all(np.abs(yv - yo) <= 2.0 ** -8 * absy + 2.0 ** -8 * np.abs(yo) + 1e-3), hook
        assert np.all(np.abs(dxv - dxo) <= 2.0 ** -8 * absdx + 2.0 ** -8 * np.abs(dxo) + 1e-3), hook
        close(n(m.lora_up.weight.grad), duo, absu, "f32", msg=f"dUp hook {hook}")
        close(n(m.lora_down.weight.grad), ddo, absd, "f32", msg=f"dDown hook {hook}")


def test_wide_module_in_eval_on_both_kernels(path_log):
    """The inference route of a rank-64 file: forward only, no mask."""
    r, B, S, K, N = 64, 2, 77, 320, 640
    M = B * S
    m = _module(r, 0.1).eval()
    s = float(m.scale)
    x = rnd((B, S, K), "bf16", seed=5)
    X = n(x).astype(np.float64).reshape(M, K)
    W, b = n(m.linear.weight).astype(np.float64), n(m.linear.bias).astype(np.float64)
    A, U = n(m.lora_down.weight).astype(np.float64), n(m.lora_up.weight).astype(np.float64)
    yo = X @ W.T + b + s * ((X @ A.T) @ U.T)
    absy = np.abs(X) @ np.abs(W).T + np.abs(b) + s * ((np.abs(X) @ np.abs(A).T) @ np.abs(U).T)
    for hook in (1, 0):
        prev = _C.rank16_mfma(hook)
        try:
            del path_log[:]
            with torch.no_grad():
                y = m(x)
        finally:
            _C.rank16_mfma(prev)
        assert [(ph, path) for ph, path, *_ in path_log] == [("fwd", "lib+primitives")], path_log
        yv = n(y).reshape(M, N)
        assert np.all(np.abs(yv - yo) <= 2.0 ** -8 * absy + 2.0 ** -8 * np.abs(yo) + 1e-3), hook
