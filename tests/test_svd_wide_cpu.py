"""cli_svd's sketch rule and routing for LoRA ranks 17..64 (``cli_svd.WIDE``), the entry points' argument checks without a
GPU, and the CPU restatement of why the capped sketch was not enough at rank 32."""
import ctypes as C

import pytest
import torch

from lora_amd import _C, ops
from lora_amd import cli_svd as S
from tests.test_cli_svd import _planted


def _parent_width(rank, oversample):
    """The rule before the wide path (and of ranks <= 16 and > 64 now): rank + max(oversample, rank) in granules of 8, capped."""
    return min(-(-(rank + max(oversample, rank)) // 8) * 8, 32)


def test_sketch_rule():
    assert S.WIDE and ops.SVD_WIDE
    table = {(17, 24): 32, (25, 40): 48, (41, 56): 64, (57, 64): 80}
    for (lo, hi), l in table.items():
        for rank in range(lo, hi + 1):
            assert S._sketch_width(rank, 8, 320, 768) == l, rank
    for rank in range(17, 65):   # another oversampling: the same rule, not the table
        assert S._sketch_width(rank, 20, 320, 768) == 16 * -(-(rank + 20) // 16)
    for over in (8, 20):
        for rank in list(range(1, 17)) + [65, 66, 96, 128]:
            assert S._sketch_width(rank, over, 320, 768) == _parent_width(rank, over), (rank, over)
    prev, S.WIDE = S.WIDE, False
    try:
        for rank in range(1, 70):
            assert S._sketch_width(rank, 8, 320, 768) == _parent_width(rank, 8)
        assert S.group_supported(320, 768, 32) and S.group_supported(320, 328, 32)   # the capped sketch took K % 8
        assert not S.group_supported(320, 768, 33) and not S.group_supported(1280, 320, 64)
    finally:
        S.WIDE = prev


def test_group_supported_per_shape():
    assert S.group_supported(320, 768, 17) and S.group_supported(320, 768, 32) and S.group_supported(1280, 320, 64)
    assert S.group_supported(96, 128, 64)            # l = 80 <= min(N, K)
    assert not S.group_supported(64, 128, 64)        # l = 80 > N
    assert not S.group_supported(320, 328, 32)       # K % 32
    assert not S.group_supported(328, 320, 32)       # N % 32
    assert not S.group_supported(320, 776, 17)       # a multiple of 8 is not enough at these ranks
    assert not S.group_supported(32, 64, 32)         # l = 48 > min(N, K)
    assert not S.group_supported(1280, 1280, 64, oversample=24)   # l = 96: past the kernels' 80 columns
    assert not S.group_supported(1280, 1280, 65)     # ranks above 64: unchanged (exact)
    # ranks <= 16 as before: K % 8 and the sketch inside the matrix
    assert S.group_supported(77, 40, 3) and S.group_supported(320, 328, 16) and not S.group_supported(320, 324, 16)
    assert not S.group_supported(24, 24, 16)


def test_ab_switch_knows_svd_wide():
    ns = {"SVD_WIDE": True}
    assert ops.apply_ab_overrides("SVD_WIDE=0", ns) == {"SVD_WIDE": False} and ns == {"SVD_WIDE": False}


def test_distill_model_on_cpu_at_rank_32_is_distill_group():
    gs = [([_planted(48, 64, 40, 1e-3, i)[0] for i in range(2)], [_planted(48, 64, 40, 1e-3, i)[1] for i in range(2)]),
          ([_planted(96, 64, 40, 1e-3, 5)[0]], [_planted(96, 64, 40, 1e-3, 5)[1]])]
    before = dict(S.ROUTES)
    res = S.distill_model(gs, 32)
    assert S.ROUTES["exact"] - before["exact"] == 3
    assert all(S.ROUTES[k] == before[k] for k in ("fused16", "ragged_f32", "wide_planes"))
    for (t, b), (up, down) in zip(gs, res):
        up1, down1 = S.distill_group(t, b, 32)
        assert up.shape[2] == 32 and torch.equal(up, up1) and torch.equal(down, down1)


@pytest.mark.skipif(not _C.available(), reason="C-ABI library not built")
def test_entry_points_check_their_new_ranges_on_the_host():
    """Argument checks run before any launch: 81 columns / l = 81 are refused with the codes of the header."""
    lib = _C.require()
    assert lib.lora_amd_rowdot16_planes(C.c_void_p(256), 1, 1, 81, _C.dtype_code(torch.bfloat16), None) == -2   # ERANK
    assert lib.lora_amd_rowdot16_planes(C.c_void_p(256), 1, 1, 0, _C.dtype_code(torch.bfloat16), None) == -2
    assert lib.lora_amd_chol_inverse_batched(C.c_void_p(256), C.c_void_p(512), 81, 1, 0.0, None) == -1          # EINVAL


def _restated(res, rank, l, n_iter=4, seed=0):
    """The subspace iteration in f32 on the CPU (Householder QR in place of CholeskyQR3): the rank-r product."""
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(res @ torch.randn(res.shape[1], l, generator=g))
    for _ in range(n_iter):
        qz, _ = torch.linalg.qr(res.t() @ q)
        q, _ = torch.linalg.qr(res @ qz)
    ub, s, vh = torch.linalg.svd(q.t() @ res, full_matrices=False)
    return (q @ ub[:, :rank]) * s[:rank] @ vh[:rank]


def test_capped_sketch_misses_the_product_bound_at_rank_32():
    """Why the sketch rule changed: on the planted spectrum 0.6 0.95^i (36 values) at 320 x 768 the iteration with the sketch
    capped at 32 columns (no oversampling at rank 32) leaves the rank-32 product percents away from the exact truncation,
    outside the 5e-3 tests/test_cli_svd.py allows; with the 48 columns of the new rule it is inside by orders of magnitude."""
    g = torch.Generator().manual_seed(1)
    u, _ = torch.linalg.qr(torch.randn(320, 36, generator=g))
    v, _ = torch.linalg.qr(torch.randn(768, 36, generator=g))
    res = (u * (0.6 * 0.95 ** torch.arange(36, dtype=torch.float32))) @ v.t()
    ue, se, vhe = torch.linalg.svd(res.double(), full_matrices=False)
    exact = ((ue[:, :32] * se[:32]) @ vhe[:32]).float()
    err = {l: float((_restated(res, 32, l) - exact).norm() / exact.norm()) for l in (32, 48)}
    assert S._sketch_width(32, 8, 320, 768) == 48
    assert err[48] <= 5e-3 / 100, err
    assert err[32] > 5e-3, err
