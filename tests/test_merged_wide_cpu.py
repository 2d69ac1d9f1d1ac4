"""Ranks 17..64 of the in-step merge, host side: ``lora_amd_merge_step_plan`` takes them (it is host arithmetic: no GPU),
tiles a table exactly as it tiles the same table at rank 16, still refuses rank 65 and refuses f32 masters above rank 16;
``MERGED_WIDE`` is a constant of the A/B spec."""
from __future__ import annotations

import ctypes as C

import pytest

from lora_amd import _C, ops

SHAPES = [(320, 320), (2560, 328), (136, 72)]


def _table(r, src_f32=0):
    sites = (_C.MstepSite * len(SHAPES))()
    for s, (N, K) in zip(sites, SHAPES):
        s.N, s.K, s.r = N, K, r
        s.w = s.up = s.down = s.out = s.out_t = 4096   # aligned fake pointers: the plan never dereferences them
        s.ld_out, s.ld_out_t = K, N
        s.src_f32 = src_f32
    return sites


def _plan(sites):
    val = C.c_int64(0)
    rc = _C.require().lora_amd_merge_step_plan(sites, len(sites), _C.BF16, C.byref(val))
    return rc, val.value


@pytest.mark.parametrize("r", [17, 32, 64])
def test_plan_takes_wide_ranks_with_the_tiles_of_rank_16(r):
    narrow, wide = _table(16), _table(r)
    rc16, val16 = _plan(narrow)
    rc, val = _plan(wide)
    assert rc16 == _C.OK and rc == _C.OK, _C.require().lora_amd_last_error()
    assert val == val16
    for a, b in zip(narrow, wide):
        assert (a.tile_begin, a.tiles_k) == (b.tile_begin, b.tiles_k)
    want = sum(-(-N // 128) * -(-K // 128) for N, K in SHAPES)
    assert val == want | (2 << 40)


def test_plan_keeps_every_tile_geometry_for_wide_ranks():
    for tile in range(4):
        got = {}
        for r in (16, 33):
            sites = _table(r)
            _C.merge_step_set_tuning(tile, -1)
            try:
                rc, val = _plan(sites)
            finally:
                _C.merge_step_set_tuning(2, -1)
            assert rc == _C.OK
            got[r] = (val, [(s.tile_begin, s.tiles_k) for s in sites])
        assert got[16] == got[33] and got[16][0] >> 40 == tile


def test_plan_refuses_rank_65_and_wide_f32_masters():
    lib = _C.require()
    rc, _ = _plan(_table(65))
    assert rc == -2 and b"rank 65" in lib.lora_amd_last_error()
    rc, _ = _plan(_table(0))
    assert rc == -2
    rc, _ = _plan(_table(16, src_f32=1))
    assert rc == _C.OK
    rc, _ = _plan(_table(17, src_f32=1))
    assert rc == -5 and b"f32 master" in lib.lora_amd_last_error()
    # the launch checks its rank argument before anything reaches a stream
    assert lib.lora_amd_merge_step(4096, 1, 1 | (2 << 40), 65, _C.BF16, 1.0, _C.ROUND_ONCE, None) == -2
    assert lib.lora_amd_merge_step(4096, 1, 1 | (2 << 40) | (1 << 48), 17, _C.BF16, 1.0, _C.ROUND_ONCE, None) == -5


def test_the_switch_is_a_module_constant_of_the_ab_spec():
    assert isinstance(ops.MERGED_WIDE, bool)
    assert ops.apply_ab_overrides("MERGED_WIDE=0", {}) == {"MERGED_WIDE": False}
    ns = {}
    ops.apply_ab_overrides("MERGED_WIDE=1", ns)
    assert ns == {"MERGED_WIDE": True}
