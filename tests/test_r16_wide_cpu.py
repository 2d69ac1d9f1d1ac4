"""lora_amd_rank16_mfma_takes: the launchers' own predicate of the matrix-core row product and rank update (ranks 9..64),
asked on the host.  No launch, no device: ``rows`` is a made-up aligned address, inspected for alignment only."""
import pytest

from lora_amd import _C

ROWDOT, RANK_UPDATE = 0, 1
ADDR = 4096


def takes(op, cols, r, *, rows=ADDR, ld=None, M=577, act=_C.BF16, fdt=_C.F32, sel=0):
    return _C.require().lora_amd_rank16_mfma_takes(op, rows, cols if ld is None else ld, M, cols, r, act, fdt, sel)


@pytest.fixture(autouse=True)
def hook_on():
    prev = _C.rank16_mfma(1)
    yield
    _C.rank16_mfma(prev)


@pytest.mark.parametrize("r", [9, 16, 17, 32, 33, 64])
def test_takes_ranks_9_to_64(r):
    """r = 17 / 32 / 33 / 64 are the wide forms: these answers are 0 (the symbol is absent) without them."""
    assert takes(ROWDOT, 320, r) == 1
    assert takes(RANK_UPDATE, 328, r) == 1
    assert takes(ROWDOT, 320, r, M=1) == 1 and takes(RANK_UPDATE, 328, r, M=9216) == 1
    assert takes(ROWDOT, 320, r, ld=384) == 1 and takes(RANK_UPDATE, 328, r, ld=392) == 1


@pytest.mark.parametrize("op,cols", [(ROWDOT, 320), (RANK_UPDATE, 328)])
def test_what_it_refuses(op, cols):
    for r in (8, 65):
        assert takes(op, cols, r) == 0
    for r in (16, 32, 64):
        assert takes(op, cols, r) == 1
        assert takes(op, cols, r, act=_C.F16) == 0            # f16 rows
        assert takes(op, cols, r, act=_C.F32) == 0
        assert takes(op, cols, r, fdt=_C.BF16) == 0           # 16-bit factors
        assert takes(op, cols, r, sel=1) == 0                 # selector calls keep the VALU kernel
        assert takes(op, cols, r, rows=ADDR + 8) == 0         # rows not 16-byte aligned
        assert takes(op, cols, r, ld=cols + 4) == 0           # ld % 8
        assert takes(op, cols, r, M=0) == 0
    for r in (16, 32, 64):
        assert takes(ROWDOT, 328, r) == 0                     # C % 32
        assert takes(RANK_UPDATE, 324, r) == 0                # N % 8
    assert takes(2, cols, 32) == 0


def test_the_hook_turns_every_answer_off_and_back_on():
    cases = [(op, cols, r) for op, cols in ((ROWDOT, 320), (RANK_UPDATE, 328)) for r in (9, 16, 17, 32, 33, 64)]
    assert all(takes(*c) == 1 for c in cases)
    prev = _C.rank16_mfma(0)
    try:
        assert all(takes(*c) == 0 for c in cases)
    finally:
        _C.rank16_mfma(prev)
    assert all(takes(*c) == 1 for c in cases)
