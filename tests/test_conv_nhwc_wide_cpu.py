"""``lora_amd_conv3_nhwc_wide_plan`` is pure host arithmetic: which ranks it takes, the pack / partial sizes of the ns = ceil(r / 16)
rank-16 slices, its cuts, and that the rank <= 16 plan answers as before.  No GPU."""
import ctypes as C

import pytest

from lora_amd import _C, ops

SITES = [(1, 320, 96, 96), (1, 640, 48, 48), (1, 1280, 24, 24), (1, 1280, 12, 12), (4, 320, 32, 32), (1, 64, 1, 1), (3, 64, 5, 7),
         (1, 64, 3, 70), (2, 192, 12, 12), (1, 2560, 24, 24)]


def _raw(B, Ci, H, W, r):
    pl = _C.Conv3NhwcPlan()
    rc = _C.require().lora_amd_conv3_nhwc_wide_plan(B, Ci, H, W, r, C.byref(pl))
    return rc, pl


def test_accepted_and_refused_ranks():
    for r, native in ((17, 0), (18, 0), (20, 1), (64, 1), (4, 0), (16, 0), (22, 0), (63, 0)):
        rc, pl = _raw(1, 320, 32, 32, r)
        assert rc == _C.OK and pl.native == native, r
        if not native:
            assert bytes(pl) == bytes(C.sizeof(pl)), "a refused plan is all zeros"
    rc, _ = _raw(1, 320, 32, 32, 65)
    assert rc == -2   # LORA_AMD_ERANK
    with pytest.raises(Exception):
        _C.conv3_nhwc_wide_plan(1, 320, 32, 32, 65)
    assert not _C.conv3_nhwc_wide_ok(1, 320, 32, 32, 65) and not _C.conv3_nhwc_wide_ok(1, 320, 32, 32, 16)
    # the geometry conditions are the narrow plan's
    assert _raw(1, 96, 32, 32, 32)[1].native == 0       # C_in % 64
    assert _raw(1, 320, 8, 512, 32)[1].native == 0      # too wide for a staged strip
    assert C.sizeof(_C.Conv3NhwcPlan) == 72


def test_the_rank_16_plan_is_unchanged():
    assert _C.conv3_nhwc_plan(1, 320, 32, 32, 20).native == 0
    assert _C.conv3_nhwc_plan(1, 320, 32, 32, 64).native == 0
    p16 = _C.conv3_nhwc_plan(1, 320, 32, 32, 16)
    assert p16.native == 1 and p16.rank_pad == 16 and p16.ks == 5 and p16.pf_elems == 9 * 320 * 16


@pytest.mark.parametrize("r", [20, 24, 32, 36, 48, 52, 64])
@pytest.mark.parametrize("B,Ci,H,W", SITES)
def test_sizes_and_cuts(B, Ci, H, W, r):
    pl = _C.conv3_nhwc_wide_plan(B, Ci, H, W, r)
    p16 = _C.conv3_nhwc_plan(B, Ci, H, W, 16)
    assert pl.native == 1 and p16.native == 1
    ns, M = -(-r // 16), B * H * W
    assert pl.rank_pad == 16 * ns and pl.ks == 5
    assert pl.pf_elems == ns * p16.pf_elems == ns * 9 * Ci * 16
    assert pl.pd_elems == ns * p16.pd_elems == ns * Ci * 5 * 32
    # the pixel tiles and strips do not depend on the rank
    assert (pl.pt, pl.ksplit, pl.pr, pl.fwd_tiles) == (p16.pt, p16.ksplit, p16.pr, p16.fwd_tiles)
    assert pl.t_part_floats == (pl.ksplit * M * r if pl.ksplit > 1 else 0)
    assert 1 <= pl.csplit <= Ci // 64
    nstrips = B * -(-H // pl.pr)
    assert 1 <= pl.nsplit <= nstrips and pl.nsplit * (Ci // 64) <= max(256, Ci // 64)
    assert pl.down_part_floats == pl.nsplit * 16 * ns * Ci * 9
    # the cap on the dDown partials, in real bytes / with the real rank: at most 30 % of the X stream or 16 MiB
    if pl.nsplit > 1:
        share = pl.nsplit * 18.0 * r / M
        assert share <= 0.30 + 1e-9 or pl.down_part_floats * 4 <= 16 << 20, (share, pl.down_part_floats * 4)


def test_route_constant_and_its_override():
    assert ops.CONV3_WIDE is True
    ns = {"CONV3_WIDE": True}
    assert ops.apply_ab_overrides("CONV3_WIDE=0", ns) == {"CONV3_WIDE": False} and ns["CONV3_WIDE"] is False


def test_binding_rows_exist():
    names = {row[0] for row in _C.FUNCTIONS}
    for leaf in ("plan", "pack", "down_fwd", "bwd_dx", "bwd_down"):
        assert f"lora_amd_conv3_nhwc_wide_{leaf}" in names
        assert hasattr(_C.require(), f"lora_amd_conv3_nhwc_wide_{leaf}")
