"""CPU checks of the matrix-core column reduction (csrc/rank16_mfma.hip colreduce16_mfma_kernel): the A/B constant, and the
lane-level model of the kernel's index arithmetic (scripts/r16_model.py: staging tile and transpose reads, T fragment order per
slice, accumulator -> D store map, the hi + lo split) against float64 T^T X."""
import os
import sys

import numpy as np
import pytest
import torch

from lora_amd import _C, ops
from tests import helpers as H

sys.path.insert(0, os.path.join(H.REPO, "scripts"))
import r16_model  # noqa: E402


def test_ab_override_flips_the_constant_and_rejects_unknown_names():
    ns = {"COLREDUCE_MFMA": True}
    assert ops.apply_ab_overrides("COLREDUCE_MFMA=0", ns) == {"COLREDUCE_MFMA": False} and ns["COLREDUCE_MFMA"] is False
    assert ops.apply_ab_overrides("COLREDUCE_MFMA=1", ns) == {"COLREDUCE_MFMA": True} and ns["COLREDUCE_MFMA"] is True
    with pytest.raises(ValueError, match="unknown constant 'COLREDUCE_VALU'"):
        ops.apply_ab_overrides("COLREDUCE_VALU=1", ns)
    assert isinstance(ops.COLREDUCE_MFMA, bool)


# whole steps at one ragged slice; a ragged last step with a one-rank last slice; three steps at four full slices
@pytest.mark.parametrize("layout", ["RK", "KR"])
@pytest.mark.parametrize("r,M", [(9, 32), (17, 45), (64, 70)])
def test_lane_level_model_of_the_column_reduction_equals_the_dense_formula(r, M, layout):
    rng = np.random.default_rng(r)
    X = r16_model.bf16_round(rng.standard_normal((M, 96)).astype(np.float32))
    T = rng.standard_normal((M, r))
    D, dead = r16_model.colreduce16(X, T, layout)
    want = T.T @ X
    assert D.shape == ((r, 96) if layout == "RK" else (96, r))
    assert np.allclose(D, want if layout == "RK" else want.T)      # the tolerance of the sibling model tests
    assert not np.isnan(D).any(), "an element of D no lane stores"
    # lanes at or past r read zero and are never stored
    assert (len(dead) > 0) == (r % 16 != 0) and not dead.any()


@pytest.mark.parametrize("r,M", [(9, 32), (17, 45), (64, 70)])
def test_model_reproduces_the_hi_lo_split(r, M):
    """T enters as two bf16 fragments into one accumulator: the result is (hi + lo)^T X, within 2^-15 of the sum of |terms|
    of T^T X (two roundings to 8 bits), where hi alone is not."""
    rng = np.random.default_rng(100 + r)
    X = r16_model.bf16_round(rng.standard_normal((M, 32)).astype(np.float32))
    T = rng.standard_normal((M, r)).astype(np.float32).astype(np.float64)
    D, _ = r16_model.colreduce16(X, T, "RK", split=True)
    hi, lo = r16_model.split_hi_lo(T)
    assert np.array_equal(hi, r16_model.bf16_round(T.astype(np.float32)))
    assert np.allclose(D, (hi + lo).T @ X)
    bound = np.abs(T).T @ np.abs(X)
    assert np.all(np.abs(D - T.T @ X) <= 2.0 ** -15 * bound)
    assert np.abs(hi.T @ X - T.T @ X).max() > 2.0 ** -15 * bound.max()


ADDR = 4096   # a made-up aligned address: the predicate inspects it for alignment only


def takes(K, r, *, x=ADDR, ld=None, M=577, dt=None):
    return _C.require().lora_amd_colreduce_mfma_takes(x, K if ld is None else ld, M, K, r, _C.BF16 if dt is None else dt)


@pytest.mark.skipif(not _C.available(), reason="C-ABI library not built")
def test_host_predicate_of_the_column_reduction():
    assert _C.rank16_mfma(-1) == 1 and _C.colreduce_mfma(-1) == 1
    for r in (9, 16, 17, 32, 33, 64):
        assert takes(320, r) == 1 and takes(32, r, M=1) == 1 and takes(320, r, ld=328) == 1 and takes(2560, r, M=9216) == 1
        assert takes(320, r, dt=_C.F16) == 0 and takes(320, r, dt=_C.F32) == 0      # f16 / f32 rows
        assert takes(328, r) == 0                                                   # K % 32
        assert takes(320, r, ld=324) == 0 and takes(320, r, x=ADDR + 8) == 0        # ld % 8, base not 16-byte aligned
        assert takes(320, r, M=0) == 0
    for r in (1, 4, 8, 65):
        assert takes(320, r) == 0
    for flip in (_C.rank16_mfma, _C.colreduce_mfma):                               # either switch off
        prev = flip(0)
        try:
            assert takes(320, 32) == 0
        finally:
            flip(prev)
        assert takes(320, 32) == 1
    # the wrapper's op 2 is this entry; the C entry of ops 0 and 1 answers 0 for any other op, as before
    x = torch.zeros(65, 320, dtype=torch.bfloat16)
    assert _C.rank16_mfma_takes(2, x, 32) == 1 and _C.rank16_mfma_takes(2, x, 8) == 0
    lib = _C.require()
    assert lib.lora_amd_rank16_mfma_takes(2, ADDR, 320, 577, 320, 32, _C.BF16, _C.F32, 0) == 0
    assert lib.lora_amd_rank16_mfma_takes(0, ADDR, 320, 577, 320, 32, _C.BF16, _C.F32, 0) == 1


def test_model_self_check():
    assert r16_model.check_colreduce16()
