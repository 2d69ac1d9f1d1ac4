"""Matrix-core column reduction (csrc/rank16_mfma.hip colreduce16_mfma_kernel, ranks 9..64) through the C ABI, after the
pattern of tests/test_gpu_r16_wide.py: every case asks _C.rank16_mfma_takes (op 2: lora_amd_colreduce_mfma_takes) first, runs lora_amd_colreduce with
the switch on and off, and holds BOTH results to the float64 restatement D = beta D0 + s T^T (mask . X) at
tests/test_gpu_kernels.close's own constants (k = 2e-5 of |D0| + s |T|^T |mask . X|: bf16 data is exact, T enters as hi + lo to
~2^-16, the sums are f32).  The dropout mask is rebuilt by tests/helpers.philox_dropout_mask."""
import numpy as np
import pytest
import torch

from lora_amd import _C, ops
from tests import memguard as MG
from tests.test_gpu_kernels import DEV, close, n, rnd
from tests.test_gpu_r16_wide import _module, lay, mask_of, path_log  # noqa: F401  (path_log: a fixture)
from tests.test_gpu_rank16 import valu

pytestmark = pytest.mark.gpu

RANKS = [9, 16, 17, 32, 40, 64]   # one slice ragged / full, a one-rank last slice, exact slices, a half slice, the maximum
LAYOUTS = ["RK", "KR"]
COLREDUCE = 2


class switch_off:
    """lora_amd_colreduce_mfma(0) for the block: the VALU two-stage kernel, the other matrix-core forms untouched."""

    def __enter__(self):
        self.prev = _C.colreduce_mfma(0)

    def __exit__(self, *a):
        _C.colreduce_mfma(self.prev)


def reference(x, t, layout, s, beta, d0, p, seed, off):
    M, K = x.shape
    xm = n(x).astype(np.float64) * mask_of(M, K, p, seed, off)
    T = n(t).astype(np.float64)
    want, bound = s * (T.T @ xm), s * (np.abs(T).T @ np.abs(xm))
    if layout == "KR":
        want, bound = want.T, bound.T
    if beta != 0.0:
        D0 = n(d0).astype(np.float64)
        want, bound = want + beta * D0, bound + abs(beta) * np.abs(D0)
    return want, bound


def run(x, t, layout, s, beta, d0, p, seed, off):
    out = d0.clone()
    assert _C.colreduce(x, t, lay(layout), s, out=out, beta=beta, dropout_p=p, seed=seed, offset=off) is out
    return out


def check_colreduce(x, r, layout, p, beta, takes=1, seed=0x51ED5EED, off=12345, s=0.7):
    M, K = x.shape
    t = rnd((M, r), "f32", 0.5, seed=2)
    shape = (r, K) if layout == "RK" else (K, r)
    d0 = rnd(shape, "f32", seed=7) if beta != 0.0 else torch.full(shape, float("nan"), device=DEV)
    assert _C.rank16_mfma(-1) == 1 and _C.colreduce_mfma(-1) == 1
    assert _C.rank16_mfma_takes(COLREDUCE, x, r) == takes
    got = run(x, t, layout, s, beta, d0, p, seed, off)
    with switch_off():
        assert _C.rank16_mfma_takes(COLREDUCE, x, r) == 0
        old = run(x, t, layout, s, beta, d0, p, seed, off)
    want, bound = reference(x, t, layout, s, beta, d0, p, seed, off)
    what = f"{M}x{K} r{r} {layout} p{p} beta{beta}"
    close(n(got), want, bound, msg=f"colreduce16 {what}")
    close(n(old), want, bound, msg=f"colreduce valu {what}")
    return got


# one row, one group | a ragged second 32-row step, three groups (a non-power-of-two tile count: one workgroup, its fourth
# wave idle) | ten groups (three column tiles, the last half empty) | two row blocks at r <= 32 | twenty column tiles
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("M,K", [(1, 32), (33, 96), (65, 320), (130, 1280), (33, 2560)])
def test_colreduce_mfma_vs_float64_and_vs_valu(M, K, r, layout, p, beta):
    check_colreduce(rnd((M, K), "bf16", seed=1), r, layout, p, beta)


# One M just above the launcher's row-block height (r16_cr_rows: 128 rows at one and two slices, 256 at three and four), so
# that a second row block leaves a partial and the fold launch runs:
#   NS = 1: r = 9, 16 at M = 129;  NS = 2: r = 17, 32 at M = 129;  NS = 3: r = 40 at M = 257;  NS = 4: r = 64 at M = 257
# and one M with three blocks per height (two partials: the fold's block order).
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,r", [(129, 9), (129, 16), (129, 17), (129, 32), (257, 40), (257, 64), (300, 32), (600, 64)])
def test_colreduce_mfma_folds_row_block_partials(M, r, layout, p, beta):
    check_colreduce(rnd((M, 96), "bf16", seed=1), r, layout, p, beta)


@pytest.mark.parametrize("r,layout,p", [(40, "KR", 0.1), (64, "RK", 0.0), (9, "RK", 0.1)])
def test_colreduce_mfma_on_a_column_slice(r, layout, p):
    M, K = 100, 640
    wide = rnd((M, K + 64), "bf16", seed=1)
    check_colreduce(wide[:, :K], r, layout, p, 1.0)


@pytest.mark.parametrize("r,layout,p", [(32, "KR", 0.1), (64, "KR", 0.1)])
def test_colreduce_mfma_many_rows(r, layout, p):
    check_colreduce(rnd((9216, 320), "bf16", seed=1), r, layout, p, 0.0)


@pytest.mark.parametrize("M,K,r,p", [(9216, 320, 64, 0.1), (257, 96, 40, 0.0), (33, 2560, 17, 0.1)])
def test_two_calls_give_the_same_bits(M, K, r, p):
    """Row-block partials are added in block order by a second launch: no atomics, nothing depends on arrival order."""
    x, t = rnd((M, K), "bf16", seed=1), rnd((M, r), "f32", 0.5, seed=2)
    d0 = rnd((K, r), "f32", seed=7)
    assert _C.rank16_mfma_takes(COLREDUCE, x, r) == 1
    a = run(x, t, "KR", 0.7, 1.0, d0, p, 5, 9)
    b = run(x, t, "KR", 0.7, 1.0, d0, p, 5, 9)
    assert torch.equal(a, b)


def test_device_offset_draws_the_mask_of_the_host_offset():
    M, K, r, p = 130, 320, 32, 0.1
    x, t = rnd((M, K), "bf16", seed=1), rnd((M, r), "f32", 0.5, seed=2)
    off = torch.tensor([(1 << 40) + 17], dtype=torch.int64, device=DEV)
    assert _C.rank16_mfma_takes(COLREDUCE, x, r) == 1
    a = _C.colreduce(x, t, _C.FACTOR_KR, 0.7, dropout_p=p, seed=5, offset=off)
    b = _C.colreduce(x, t, _C.FACTOR_KR, 0.7, dropout_p=p, seed=5, offset=int(off.item()))
    assert torch.equal(a, b)


# ----------------------------------------------------------------------------- footprint
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,K,r", [(257, 320, 64), (1, 32, 17)])
def test_footprint_with_guards_and_poisoned_sources(M, K, r, layout):
    """D and a workspace of exactly lora_amd_colreduce_workspace bytes in guarded allocations; X (row stride K + 8, the gaps
    poisoned) and T in poisoned ones.  Guards intact, the result finite and at the float64 restatement."""
    p, seed, off, s = 0.1, 5, 9, 0.7
    lib = _C.require()
    x0, t0 = rnd((M, K), "bf16", seed=1), rnd((M, r), "f32", 0.5, seed=2)
    x, t = MG.poisoned(x0, ld=K + 8), MG.poisoned(t0)
    d0 = rnd((r, K) if layout == "RK" else (K, r), "f32", seed=7)
    D = MG.guarded_like(d0)
    wsb = int(lib.lora_amd_colreduce_workspace(M, K, r))
    ws = MG.Guarded((max(wsb // 4, 1),), torch.float32, DEV)
    assert _C.rank16_mfma_takes(COLREDUCE, x, r) == 1
    rc = lib.lora_amd_colreduce(x.data_ptr(), x.stride(0), t.data_ptr(), D.ptr, M, K, r, _C.BF16, lay(layout), s, 1.0, p, seed,
                                off, None, ws.ptr, wsb, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _C.require().lora_amd_last_error()
    torch.cuda.synchronize()
    D.check("colreduce16: D")
    ws.check("colreduce16: workspace")
    MG.assert_finite(D.data, what="colreduce16: D")
    want, bound = reference(x0, t0, layout, s, 1.0, d0, p, seed, off)
    close(n(D.data), want, bound, msg=f"guarded colreduce16 {M}x{K} r{r} {layout}")


# ----------------------------------------------------------------------------- predicate
@pytest.mark.parametrize("dt,M,K,r", [("f16", 65, 320, 32), ("f32", 65, 320, 32), ("bf16", 65, 328, 32), ("bf16", 65, 320, 8),
                                      ("bf16", 65, 320, 4)])
def test_what_the_matrix_core_form_does_not_take_stays_on_the_valu_kernel(dt, M, K, r):
    x, t = rnd((M, K), dt, seed=1), rnd((M, r), "f32", 0.5, seed=2)
    assert _C.rank16_mfma(-1) == 1 and _C.colreduce_mfma(-1) == 1
    assert _C.rank16_mfma_takes(COLREDUCE, x, r) == 0
    d0 = rnd((K, r), "f32", seed=7)
    got = run(x, t, "KR", 0.7, 1.0, d0, 0.1, 5, 9)
    want, bound = reference(x, t, "KR", 0.7, 1.0, d0, 0.1, 5, 9)
    close(n(got), want, bound, msg=f"colreduce valu {dt} {M}x{K} r{r}")


@pytest.mark.parametrize("hook", ["global", "own"])
def test_either_hook_off_routes_to_the_valu_kernel(hook):
    M, K, r = 65, 320, 32
    x, t = rnd((M, K), "bf16", seed=1), rnd((M, r), "f32", 0.5, seed=2)
    d0 = rnd((K, r), "f32", seed=7)
    assert _C.rank16_mfma_takes(COLREDUCE, x, r) == 1
    with (valu() if hook == "global" else switch_off()):
        assert _C.rank16_mfma_takes(COLREDUCE, x, r) == 0
        assert _C.rank16_mfma_takes(0, x, r) == (0 if hook == "global" else 1)   # the row product keeps its own answer
        got = run(x, t, "KR", 0.7, 1.0, d0, 0.1, 5, 9)
    assert _C.rank16_mfma_takes(COLREDUCE, x, r) == 1
    want, bound = reference(x, t, "KR", 0.7, 1.0, d0, 0.1, 5, 9)
    close(n(got), want, bound, msg=f"colreduce with the {hook} hook off")


def test_switch_returns_the_previous_value_and_defaults_to_on():
    assert _C.colreduce_mfma(-1) == 1 and _C.colreduce_mfma(0) == 1 and _C.colreduce_mfma(-1) == 0 and _C.colreduce_mfma(1) == 0
    assert _C.colreduce_mfma(-1) == 1 and ops.COLREDUCE_MFMA is True


# ----------------------------------------------------------------------------- autograd, without a trainer state
@pytest.fixture
def calls(monkeypatch):
    """Every ``ops.colreduce_any`` call of the block, with its result: what the autograd layer asked of the kernel."""
    log, inner = [], ops.colreduce_any

    def recording(x, t, layout, scale=1.0, out=None, beta=0.0, p=0.0, seed=0, off=0):
        assert out is None, "no sink in these tests"
        res = inner(x, t, layout, scale, out, beta, p, seed, off)
        log.append((x.detach().clone(), t.detach().clone(), layout, float(scale), float(p), int(seed), int(off), res.detach().clone()))
        return res

    monkeypatch.setattr(ops, "colreduce_any", recording)
    return log


def _on_and_off(step, calls, path_log, monkeypatch, want_calls):
    """``step()`` with COLREDUCE_MFMA on and off: the same route names, every colreduce call of both runs at its float64
    restatement, on the matrix-core form exactly when the constant is on."""
    routes, grads = [], []
    for on in (True, False):
        monkeypatch.setattr(ops, "COLREDUCE_MFMA", on)
        prev = _C.colreduce_mfma(1 if on else 0)
        try:
            del calls[:], path_log[:]
            grads.append(step())
            torch.cuda.synchronize()
            assert len(calls) == want_calls, len(calls)
            for x, t, layout, s, p, seed, off, res in calls:
                assert _C.rank16_mfma_takes(COLREDUCE, x, t.shape[1]) == (1 if on else 0)
                name = "RK" if layout == _C.FACTOR_RK else "KR"
                want, bound = reference(x, t, name, s, 0.0, None, p, seed, off)
                close(n(res), want, bound, msg=f"COLREDUCE_MFMA={on} {tuple(x.shape)} r{t.shape[1]} {name}")
        finally:
            _C.colreduce_mfma(prev)
        routes.append([(ph, path) for ph, path, *_ in path_log])
    assert routes[0] == routes[1] and routes[0], routes
    return routes[0], grads


def test_linear_function_factor_gradients_on_both_kernels(calls, path_log, monkeypatch):
    """ops.LoraLinearFunction at rank 32 with dropout 0.1 (M 77, K 320, N 640), no trainer state: dUp = s (mask . G)^T T and
    dDown = Gt^T X are two colreduce calls of the site's backward."""
    r, p, S, K, N = 32, 0.1, 77, 320, 640
    m = _module(r, p).train()
    x0, gy = rnd((1, S, K), "bf16", seed=5), rnd((1, S, N), "bf16", seed=6)

    def step():
        x = x0.clone().requires_grad_(True)
        m.lora_up.weight.grad = m.lora_down.weight.grad = None
        torch.manual_seed(3)
        m(x).backward(gy)
        return n(m.lora_up.weight.grad).copy(), n(m.lora_down.weight.grad).copy()

    routes, grads = _on_and_off(step, calls, path_log, monkeypatch, 2)
    assert routes == [("fwd", "lib+primitives"), ("bwd", "primitives")], routes
    for a, b in zip(*grads):
        assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()


def test_conv3_wide_function_up_gradient_on_both_kernels(calls, path_log, monkeypatch):
    """ops.LoraConv3NhwcWideFunction at rank 32 (B 1, C 64, 8 x 8): dUp comes whole from one colreduce call on the pixel
    rows of G (dDown does not pass through it)."""
    import lora_amd as L

    B, C, Hh, Ww, r = 1, 64, 8, 8, 32
    torch.manual_seed(0)
    m = L.LoraInjectedConv2d(C, C, 3, 1, 1, r=r, dropout_p=0.0, scale=0.8)
    m.lora_up.weight.data.normal_(0, 0.05)
    m.to(DEV)
    m.conv.to(torch.bfloat16)
    x0 = rnd((B, C, Hh, Ww), "bf16", seed=5).contiguous(memory_format=torch.channels_last)
    gy = rnd((B, C, Hh, Ww), "bf16", seed=6).contiguous(memory_format=torch.channels_last)

    def step():
        x = x0.clone(memory_format=torch.preserve_format).requires_grad_(True)
        m.lora_up.weight.grad = m.lora_down.weight.grad = None
        m(x).backward(gy)
        return n(m.lora_up.weight.grad).copy(), n(m.lora_down.weight.grad).copy()

    routes, grads = _on_and_off(step, calls, path_log, monkeypatch, 1)
    M = B * Hh * Ww
    assert [e for e in routes if e[1].startswith("conv3")] == [("fwd", "conv3_nhwc_wide"), ("bwd", "conv3_nhwc_wide")], routes
    (up_on, _), (up_off, _) = grads
    assert up_on.shape == up_off.shape == (C, r, 1, 1) and calls[0][0].shape == (M, C)
