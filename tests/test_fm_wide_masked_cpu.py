"""CPU checks of the masked matrix-core factor pass at ranks 17..64 (csrc/factor_mfma.hip, DROP and WIDE together;
``ops.WIDE_DROPOUT``): the ragged plan with dropout at these ranks (same arithmetic as the maskless plan of
tests/test_fm_wide_cpu.py: grid, block begins, block map, wide and narrow tables kept apart), the launch entry's argument
checks under both flag bits (they come before any launch), the table the binding plans, and the switch.  Needs the built
library, no GPU."""
import ctypes as C

import pytest
import torch

from lora_amd import _C, ops
from tests.test_fm_wide_cpu import _fm_sites, launch_refusals

needs_lib = pytest.mark.skipif(not _C.available(), reason="C-ABI library not built")
EINVAL, ERANK = -1, -2
BF = torch.bfloat16


def _plan(specs, cls=1, rows=64):
    arr, grid = _fm_sites(specs, rows), C.c_int64(-1)
    return _C.require().lora_amd_factors_mfma_ragged_plan(arr, len(specs), _C.BF16, cls, C.byref(grid)), arr, grid.value


@needs_lib
def test_masked_plan_of_one_wide_dropout_site():
    """M = 70 at 64-row blocks: two row blocks; rank 33: three slices -> 2 x 3 consecutive workgroups, all of site 0."""
    rc, arr, grid = _plan([(70, 64, 96, 33, 0.1)])
    assert rc == 0 and grid == 6
    assert list(_C.factors_mfma_block_map(arr, grid)) == [0] * 6
    # the same table by a raw call
    g = C.c_int64(0)
    assert _C.require().lora_amd_factors_mfma_ragged_plan(_fm_sites([(70, 64, 96, 33, 0.1)]), 1, _C.BF16, 1, C.byref(g)) == 0
    assert g.value == 6


@needs_lib
def test_masked_and_maskless_wide_sites_share_a_table():
    """Ranks 33 / 64 / 17 (3, 4, 2 slices; 2, 4, 1 row blocks), masked and maskless mixed: the maskless plan's block begins."""
    specs = [(70, 64, 96, 33, 0.1), (200, 96, 64, 64, 0.0), (64, 64, 64, 17, 0.1)]
    rc, arr, grid = _plan(specs)
    assert rc == 0 and [q.block_begin for q in arr] == [0, 6, 22] and grid == 24
    assert list(_C.factors_mfma_block_map(arr, grid)) == [0] * 6 + [1] * 16 + [2] * 2
    # field for field the maskless plan of the same shapes (the mask changes no geometry)
    plain = _fm_sites([s[:4] + (0.0,) for s in specs])
    g = C.c_int64(0)
    assert _C.require().lora_amd_factors_mfma_ragged_plan(plain, 3, _C.BF16, 1, C.byref(g)) == 0 and g.value == grid
    for a, b in zip(arr, plain):
        b.dropout_p = a.dropout_p
        assert bytes(a) == bytes(b)


@needs_lib
def test_masked_plan_keeps_wide_and_narrow_apart():
    for specs in ([(70, 64, 96, 33, 0.1), (70, 64, 96, 16, 0.1)], [(70, 64, 96, 16, 0.0), (70, 64, 96, 17, 0.1)]):
        assert _plan(specs)[0] == ERANK
    assert _plan([(70, 64, 96, 65, 0.1)])[0] == ERANK
    # a narrow table with a dropout site
    rc, arr, grid = _plan([(70, 64, 96, 16, 0.1), (200, 96, 64, 9, 0.0)])
    assert rc == 0 and grid == 2 + 4 and [q.reserved for q in arr] == [0, 0]
    # the argument checks of the plan
    g = C.c_int64(0)
    lib = _C.require()
    assert lib.lora_amd_factors_mfma_ragged_plan(_fm_sites([(70, 64, 96, 33, 0.1)]), 1, _C.BF16, 3, C.byref(g)) == EINVAL
    assert lib.lora_amd_factors_mfma_ragged_plan(_fm_sites([(70, 64, 96, 33, 0.1)]), 1, _C.F32, 1, C.byref(g)) == EINVAL
    assert lib.lora_amd_factors_mfma_ragged_plan(_fm_sites([(70, 60, 96, 33, 0.1)]), 1, _C.BF16, 1, C.byref(g)) == EINVAL


@needs_lib
def test_wide_masked_launch_checks_its_arguments_before_any_launch():
    """No device is touched: every call below is refused by the argument checks."""
    launch_refusals(_C.FM_TABLE_MASKED | _C.FM_TABLE_WIDE)
    # the same checks whatever the flag word, and a bit outside it next to the pair is refused
    for flags in (0, _C.FM_TABLE_MASKED, _C.FM_TABLE_WIDE):
        launch_refusals(flags)
    fn = _C.require().lora_amd_linear_bwd_factors_mfma_ragged
    assert fn(4096, 1, 1, None, 1, 64, _C.BF16, _C.FM_TABLE_MASKED | _C.FM_TABLE_WIDE | 4, None) == EINVAL


class _T:
    """What factors_mfma_table reads of a tensor."""

    def __init__(self, rows, cols):
        self.shape = (rows, cols)

    def data_ptr(self):
        return 4096

    def stride(self, _):
        return self.shape[1]


@needs_lib
def test_binding_takes_the_masked_plan_only_for_a_wide_dropout_site():
    def site(M, K, N, r, drop):
        plan = _C.factors_mfma_plan(M, K, N, r, BF, wide=r > 16)
        assert plan.supported
        t = _T(1, 1)
        return (_T(M, N), _T(M, K), t, t, t, t, 0.5, None, None, r, plan, drop)

    arr, grid = _C.factors_mfma_table([site(70, 64, 96, 33, (0.1, 7, 3)), site(200, 96, 64, 64, None)], BF, 1)
    assert grid == 6 + 16 and [q.block_begin for q in arr] == [0, 6]
    assert arr[0].dropout_p == pytest.approx(0.1) and arr[0].scale == pytest.approx(0.5 / 0.9) and (arr[0].seed, arr[0].offset) == (7, 3)
    assert arr[1].dropout_p == 0.0 and arr[1].scale == 0.5
    arr, grid = _C.factors_mfma_table([site(70, 64, 96, 33, (0.0, 7, 3))], BF, 1)   # p = 0: a maskless site
    assert grid == 6 and arr[0].dropout_p == 0.0


def test_switch_is_a_module_constant_of_the_ab_spec():
    assert ops.WIDE_DROPOUT is True
    ns = {}
    assert ops.apply_ab_overrides("WIDE_DROPOUT=0", ns) == {"WIDE_DROPOUT": False} and ns["WIDE_DROPOUT"] is False
    assert ops.apply_ab_overrides("WIDE_DROPOUT=1", {}) == {"WIDE_DROPOUT": True}
