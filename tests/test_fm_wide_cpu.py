"""CPU checks of the matrix-core factor pass at ranks 17..64 (csrc/factor_mfma.hip, the WIDE form: a rank-r site is
ns = ceil(r / 16) independent rank-16 slices on the same G and X): the host planner's answers under LORA_AMD_FM_PLAN_WIDE, the
pack plan, the ragged plan (grid, block map, wide and narrow tables kept apart, no dropout) and the lane-level index model
(scripts/fm_model.py) assembling the [16 ns][C] slab from per-slice blocks.  Needs the built library, no GPU."""
import ctypes as C
import os
import sys

import pytest
import torch

from lora_amd import _C
from tests import helpers as H

sys.path.insert(0, os.path.join(H.REPO, "scripts"))
import fm_model  # noqa: E402

needs_lib = pytest.mark.skipif(not _C.available(), reason="C-ABI library not built")
EINVAL, ERANK = -1, -2
BF = torch.bfloat16


@needs_lib
@pytest.mark.parametrize("r,rt", [(17, 32), (32, 32), (33, 48), (48, 48), (64, 64)])
def test_wide_plan_is_the_rank_16_geometry_with_ns_slices(r, rt):
    M, K, N = 1024, 320, 320
    ns = rt // 16
    assert _C.FM_PLAN_WIDE == 2
    pl, p16 = _C.factors_mfma_plan(M, K, N, r, BF, wide=True), _C.factors_mfma_plan(M, K, N, 16, BF)
    assert pl.supported == 1 and p16.supported == 1 and pl.rank_tile == rt
    assert (pl.lds_class, pl.rows_per_block, pl.lds_bytes) == (p16.lds_class, p16.rows_per_block, p16.lds_bytes)
    assert pl.nparts == p16.nparts == -(-M // pl.rows_per_block) and pl.blocks_per_wg == 1
    assert pl.up_part_floats == pl.nparts * rt * N and pl.down_part_floats == pl.nparts * rt * K
    assert pl.pack_up_elems == ns * (2 * N * 16 + 8) and pl.pack_down_elems == ns * (2 * K * 16 + 8)


@needs_lib
def test_wide_plan_refusals_and_the_flag_changes_nothing_below_17():
    M, K, N = 1024, 320, 320
    assert not _C.factors_mfma_plan(M, K, N, 65, BF, wide=True).supported        # past the kernels' rank limit
    assert not _C.factors_mfma_plan(M, K, N, 32, torch.float32, wide=True).supported   # f32 activations
    assert not _C.factors_mfma_plan(M, 328, N, 32, BF, wide=True).supported      # K not a multiple of 32
    assert not _C.factors_mfma_plan(M, K, N, 17, BF).supported                   # without the flag: as before
    raw = _C.FactorsMfmaPlan()
    assert _C.require().lora_amd_factors_mfma_plan(M, K, N, 17, _C.BF16, 0, 0, C.byref(raw)) == 0 and raw.supported == 0
    for r in (1, 4, 8, 9, 16):   # the flag at rank <= 16: today's plan, field by field
        a, b = _C.factors_mfma_plan(M, K, N, r, BF), _C.factors_mfma_plan(M, K, N, r, BF, wide=True)
        assert bytes(a) == bytes(b), r


def _pack_sites(specs):
    arr = (_C.PackSite * len(specs))()
    for q, (N, K, r) in zip(arr, specs):
        q.down = q.up = q.pk_down = q.pk_up = 4096   # any non-null, 16-byte aligned address: the plan only does arithmetic
        q.N, q.K, q.r = N, K, r
    return arr


@needs_lib
def test_pack_plan_counts_slices():
    N, K = 96, 64
    total = C.c_int64(0)
    lib = _C.require()
    for r, ns in ((17, 2), (64, 4)):
        arr = _pack_sites([(N, K, r)])
        assert lib.lora_amd_factor_pack_plan(arr, 1, C.byref(total)) == 0
        assert total.value == ((N + K) // 8) * 16 * ns
    arr = _pack_sites([(N, K, 17), (N, K, 4), (N, K, 64)])   # every site's work items begin where the last one's end
    assert lib.lora_amd_factor_pack_plan(arr, 3, C.byref(total)) == 0
    per = (N + K) // 8
    assert [q.begin for q in arr] == [0, per * 32, per * 32 + per * 4] and total.value == per * (32 + 4 + 64)
    assert lib.lora_amd_factor_pack_plan(_pack_sites([(N, K, 65)]), 1, C.byref(total)) == ERANK


def _fm_sites(specs, rows=64):
    arr = (_C.FmSite * len(specs))()
    for q, (M, K, N, r, p) in zip(arr, specs):
        q.g = q.x = q.pk_up = q.pk_down = q.up_part = q.down_part = 4096
        q.ldg, q.ldx, q.M, q.N, q.K, q.r, q.scale, q.rows_per_block = N, K, M, N, K, r, 1.0, rows
        q.blocks_per_wg, q.dropout_p = 1, p
    return arr


@needs_lib
def test_ragged_plan_of_wide_tables():
    lib, grid = _C.require(), C.c_int64(0)
    # M = 70 at 64-row blocks: two row blocks; rank 33: three slices -> the site owns 2 x 3 consecutive workgroups
    arr = _fm_sites([(70, 64, 96, 33, 0.0)])
    assert lib.lora_amd_factors_mfma_ragged_plan(arr, 1, _C.BF16, 1, C.byref(grid)) == 0 and grid.value == 2 * 3
    assert list(_C.factors_mfma_block_map(arr, grid.value)) == [0] * 6
    # two wide sites of different slice counts share a table
    arr = _fm_sites([(70, 64, 96, 33, 0.0), (200, 96, 64, 64, 0.0), (64, 64, 64, 17, 0.0)])
    assert lib.lora_amd_factors_mfma_ragged_plan(arr, 3, _C.BF16, 1, C.byref(grid)) == 0
    assert [q.block_begin for q in arr] == [0, 6, 6 + 4 * 4] and grid.value == 6 + 16 + 2
    assert list(_C.factors_mfma_block_map(arr, grid.value)) == [0] * 6 + [1] * 16 + [2] * 2
    # a wide and a narrow site together, in either order
    for specs in ([(70, 64, 96, 33, 0.0), (70, 64, 96, 16, 0.0)], [(70, 64, 96, 16, 0.0), (70, 64, 96, 17, 0.0)]):
        assert lib.lora_amd_factors_mfma_ragged_plan(_fm_sites(specs), 2, _C.BF16, 1, C.byref(grid)) == ERANK
    assert lib.lora_amd_factors_mfma_ragged_plan(_fm_sites([(70, 64, 96, 65, 0.0)]), 1, _C.BF16, 1, C.byref(grid)) == ERANK
    # dropout at these ranks changes no geometry: the two row blocks x three slices of the maskless site above
    assert lib.lora_amd_factors_mfma_ragged_plan(_fm_sites([(70, 64, 96, 33, 0.1)]), 1, _C.BF16, 1, C.byref(grid)) == 0
    assert grid.value == 6
    # a narrow table reads as before
    arr = _fm_sites([(70, 64, 96, 16, 0.1), (200, 96, 64, 9, 0.0)])
    assert lib.lora_amd_factors_mfma_ragged_plan(arr, 2, _C.BF16, 1, C.byref(grid)) == 0 and grid.value == 2 + 4
    assert [q.reserved for q in arr] == [0, 0]


def launch_refusals(flags):
    """The argument checks of lora_amd_linear_bwd_factors_mfma_ragged under the flag word ``flags``: every call is refused
    before any launch, so no device is touched."""
    def fn(table, n, grid, block_map, lds_class, rows, act_dtype):
        return _C.require().lora_amd_linear_bwd_factors_mfma_ragged(table, n, grid, block_map, lds_class, rows, act_dtype, flags, None)

    assert fn(4096, 1, 1, None, 3, 64, _C.BF16) == EINVAL      # lds_class outside {1, 2}
    assert fn(4096, 1, 1, None, 0, 64, _C.BF16) == EINVAL
    assert fn(4096, 1, 1, None, 1, 48, _C.BF16) == EINVAL      # rows_per_block outside {0, 32, 64}
    assert fn(4096, 1, 1, None, 1, 0, _C.BF16) == EINVAL       # a class-1 table has one block height
    assert fn(4096, 1, 1, None, 1, 64, _C.F32) == EINVAL       # 16-bit activations only
    assert fn(None, 1, 1, None, 1, 64, _C.BF16) == EINVAL      # no table
    assert fn(4096, 1, 0, None, 1, 64, _C.BF16) == EINVAL      # empty grid
    assert fn(4096, 1, 1, 4098, 1, 64, _C.BF16) == EINVAL      # misaligned block map


@needs_lib
def test_launch_flags_refuse_masked_and_wide_together():
    """The pair of flag bits is a launch like any other: its argument checks come before the launch (no device is touched);
    a bit outside the two is refused."""
    assert (_C.FM_TABLE_MASKED, _C.FM_TABLE_WIDE) == (1, 2)
    lib = _C.require()
    launch_refusals(_C.FM_TABLE_MASKED | _C.FM_TABLE_WIDE)
    assert lib.lora_amd_linear_bwd_factors_mfma_ragged(4096, 1, 1, None, 1, 64, _C.BF16, 4, None) != 0


@pytest.mark.parametrize("args", [dict(M=70, K=64, N=96, r=33, R=64), dict(M=40, K=320, N=96, r=17, R=32),
                                  dict(M=50, K=320, N=320, r=64, R=32, gh=(8, 40, 64))])
def test_lane_level_model_assembles_the_wide_slab_from_rank_16_slices(args):
    """scripts/fm_model.py at ranks above 16: every (row block, slice) workgroup reads its own rank-16 pack and writes 16 rows of
    the [16 ns][C] slab; the fold over the row blocks equals the dense formula at the model's 1e-9."""
    assert fm_model.slices(args["r"]) == -(-args["r"] // 16)
    fm_model.check(**args)
