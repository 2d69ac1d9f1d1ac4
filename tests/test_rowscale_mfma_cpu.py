"""CPU checks of the row-table form of the matrix-core rank update (csrc/rank16_mfma.hip rank_update16_mfma_kernel<.., RSC =
true>, reached through lora_amd_rank_update_rowscale): the launcher's own predicate as the C entry
lora_amd_rank_update_rowscale_mfma_takes exposes it, and the lane-level model of the staging (scripts/r16_model.py: row -> table
row once per lane and slab, the multiply in f32, the hi + lo split per slice) against float64 and against the two bit rules
of the table."""
import os
import sys

import numpy as np
import pytest
import torch

from lora_amd import _C
from tests import helpers as H

sys.path.insert(0, os.path.join(H.REPO, "scripts"))
import r16_model  # noqa: E402

ADDR = 4096   # a made-up aligned address: the predicate inspects it for alignment only
needs_lib = pytest.mark.skipif(not _C.available(), reason="C-ABI library not built")


def takes(N, r, *, y=ADDR, ld=None, M=577, dt=None, fdt=None):
    return _C.require().lora_amd_rank_update_rowscale_mfma_takes(y, N if ld is None else ld, M, N, r,
                                                                 _C.BF16 if dt is None else dt, _C.F32 if fdt is None else fdt)


@needs_lib
def test_host_predicate_of_the_row_table_form():
    assert _C.rank16_mfma(-1) == 1
    for r in range(9, 65):
        assert takes(328, r) == 1 and takes(328, r, M=1) == 1 and takes(328, r, M=9216) == 1 and takes(328, r, ld=328 + 64) == 1
    for r in (9, 16, 17, 32, 40, 64):
        assert takes(320, r, dt=_C.F16) == 0 and takes(320, r, dt=_C.F32) == 0          # f16 / f32 rows
        assert takes(320, r, fdt=_C.BF16) == 0 and takes(320, r, fdt=_C.F16) == 0       # 16-bit factors
        assert takes(324, r) == 0                                                       # N % 8
        assert takes(320, r, ld=324) == 0 and takes(320, r, y=ADDR + 8) == 0            # ld % 8, base not 16-byte aligned
        assert takes(320, r, M=0) == 0
    for r in (1, 4, 8, 65, 96):
        assert takes(320, r) == 0
    prev = _C.rank16_mfma(0)
    try:
        for r in (9, 16, 40, 64):
            assert takes(328, r) == 0
    finally:
        _C.rank16_mfma(prev)
    assert takes(328, 40) == 1


@needs_lib
def test_wrapper_asks_the_same_entry():
    for shape, dt in (((65, 328), torch.bfloat16), ((65, 328), torch.float16), ((65, 324), torch.bfloat16),
                      ((1, 8), torch.bfloat16)):
        y = torch.zeros(shape, dtype=dt)
        for r in (8, 9, 40, 64, 65):
            for fdt in (torch.float32, torch.bfloat16):
                want = _C.require().lora_amd_rank_update_rowscale_mfma_takes(y.data_ptr(), y.stride(0), shape[0], shape[1], r,
                                                                             _C.dtype_code(dt), _C.dtype_code(fdt))
                assert _C.rank_update_rowscale_takes(y, r, fdt) == want
    wide = torch.zeros(33, 328 + 64, dtype=torch.bfloat16)
    assert _C.rank_update_rowscale_takes(wide[:, :328], 40) == 1          # a column-slice view: ld = N + 64
    assert _C.rank_update_rowscale_takes(wide[:, 4:332], 40) == 0         # its base 8 bytes off
    assert _C.rank_update_rowscale_takes(torch.zeros(65, 328, dtype=torch.bfloat16), 8) == 0


@needs_lib
def test_rank16_mfma_takes_keeps_its_answers():
    lib = _C.require()
    for op in (2, 3):
        assert lib.lora_amd_rank16_mfma_takes(op, ADDR, 320, 577, 320, 32, _C.BF16, _C.F32, 0) == 0
    assert lib.lora_amd_rank16_mfma_takes(0, ADDR, 320, 577, 320, 32, _C.BF16, _C.F32, 0) == 1
    assert lib.lora_amd_rank16_mfma_takes(1, ADDR, 320, 577, 320, 32, _C.BF16, _C.F32, 0) == 1
    assert lib.lora_amd_rank16_mfma_takes(0, ADDR, 320, 577, 320, 32, _C.BF16, _C.F32, 1) == 0
    assert lib.lora_amd_abi_version() == 8


def _case(r, rows, nsel, seed):
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((rows, r)).astype(np.float32)
    U = rng.standard_normal((32, r)).astype(np.float32).astype(np.float64)
    RS = (rng.random((nsel, r)) * 2 - 0.5).astype(np.float32)
    return T, U, RS


# rows-per-sample values that split a 16-row slab (5, 7, 13), a slab-aligned one that changes sample between slabs (16), a
# first row off zero (the workgroup's m0), and ragged last slabs
CASES = [(9, 16, 2, 5, 0), (16, 23, 3, 7, 64), (17, 40, 2, 13, 128), (40, 37, 3, 16, 192), (64, 33, 4, 5, 64)]


@pytest.mark.parametrize("r,rows,nsel,rps,m0", CASES)
def test_lane_model_of_the_row_table_staging_against_float64(r, rows, nsel, rps, m0):
    """Both operands enter as hi + lo: within 2^-15 of the sum of |terms| (the constant of the model's split tests; the f32
    multiply by the table adds 2^-24)."""
    T, U, RS = _case(r, rows, nsel, r)
    q = ((m0 + np.arange(rows)) // rps) % nsel
    assert len(set(q[:16])) > 1 or rps == 16, "the case must split a slab"
    TS = T.astype(np.float64) * RS.astype(np.float64)[q]
    got = r16_model.rank_update16_rows(T, U, 0.75, RS, nsel, rps, m0)
    assert got.shape == (rows, 32)
    assert np.all(np.abs(got - 0.75 * TS @ U.T) <= 2.0 ** -15 * 0.75 * (np.abs(TS) @ np.abs(U).T))
    # and it is not the plain product: the table matters on every row whose multipliers are not all one
    plain = r16_model.rank_update16_rows(T, U, 0.75)
    assert np.abs(got - plain).max() > 0.01


@pytest.mark.parametrize("r,rows,nsel,rps,m0", CASES)
def test_lane_model_all_ones_table_gives_the_plain_bits(r, rows, nsel, rps, m0):
    T, U, _ = _case(r, rows, nsel, 100 + r)
    plain = r16_model.rank_update16_rows(T, U, 0.75)
    assert np.array_equal(r16_model.rank_update16_rows(T, U, 0.75, np.ones((nsel, r), np.float32), nsel, rps, m0), plain)
    assert np.all(np.abs(plain - 0.75 * T.astype(np.float64) @ U.T) <= 2.0 ** -15 * 0.75 * (np.abs(T) @ np.abs(U).T))


@pytest.mark.parametrize("r,rows,nsel,rps,m0", CASES)
def test_lane_model_power_of_two_rows_give_the_plain_bits_at_scale_c(r, rows, nsel, rps, m0):
    T, U, _ = _case(r, rows, nsel, 200 + r)
    c = np.array([1.0, 0.5, 2.0, 0.0], np.float32)[:nsel]
    q = ((m0 + np.arange(rows)) // rps) % nsel
    got = r16_model.rank_update16_rows(T, U, 0.75, np.repeat(c[:, None], r, 1), nsel, rps, m0)
    for k in range(nsel):
        assert (q == k).any()
        assert np.array_equal(got[q == k], r16_model.rank_update16_rows(T, U, 0.75 * c[k])[q == k])


def test_model_self_check():
    assert r16_model.check_rank_update16_rows()
