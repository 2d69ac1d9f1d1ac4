"""Host side of the resident channels_last GroupNorm (csrc/hostops.hip): the route is a pure function of the geometry and
the `lora_amd_groupnorm_nhwc_resident` flag; no device is needed.  The table is the flagship step's 61 sites at batch 4
(DESIGN.md section 3.5): 43 run resident forward, 30 backward."""
import pytest
import torch

from lora_amd import _C, ops

pytestmark = pytest.mark.skipif(_C.load() is None, reason="liblora_amd.so not built")

# (C, pixels, sites, resident forward, resident backward, workspace bytes of the parent commit); B = 4, 32 groups, bf16
STEP_SITES = [
    (1280, 64, 12, True, True, 204800),
    (2560, 64, 3, True, True, 737280),
    (640, 256, 1, True, True, 184320),
    (1280, 256, 11, True, True, 696320),
    (1920, 256, 1, True, True, 552960),
    (2560, 256, 2, True, True, 2703360),
    (320, 1024, 1, True, False, 174080),
    (640, 1024, 11, True, False, 675840),
    (960, 1024, 1, False, False, 430080),    # 240 KB per workgroup: the 1024-thread form spilled, so it does not exist
    (1280, 1024, 1, True, False, 1679360),
    (1920, 1024, 1, False, False, 860160),
    (320, 4096, 13, False, False, 409600),
    (640, 4096, 2, False, False, 819200),
    (960, 4096, 1, False, False, 430080),
]
B, G, DT = 4, 32, torch.bfloat16


@pytest.fixture(autouse=True)
def _restore_flag():
    prev = _C.groupnorm_nhwc_resident(-1)
    try:
        yield
    finally:
        _C.groupnorm_nhwc_resident(prev)


def test_step_table_follows_the_documented_rule():
    assert len(STEP_SITES) == 14 and sum(s[2] for s in STEP_SITES) == 61
    _C.groupnorm_nhwc_resident(1)
    for C, HW, _, fwd, bwd, _ in STEP_SITES:
        assert _C.groupnorm_nhwc_route(B, C, HW, G, DT, False) == fwd, (C, HW, "forward")
        assert _C.groupnorm_nhwc_route(B, C, HW, G, DT, True) == bwd, (C, HW, "backward")
    assert sum(n for _, _, n, fwd, _, _ in STEP_SITES if fwd) == 43
    assert sum(n for _, _, n, _, bwd, _ in STEP_SITES if bwd) == 30


def test_rule_is_capacity_in_bytes():
    """Forward: 16 chunks of 16 bytes per thread (f32: 16 of 32 bytes) on 512 / chunks-per-bundle pixel slots; backward a
    quarter of the forward's bytes per operand.  C = 640: 5 chunks per bundle, 102 slots."""
    _C.groupnorm_nhwc_resident(1)
    for dt, bwd, most in ((torch.bfloat16, False, 1632), (torch.float16, False, 1632), (torch.float32, False, 1632),
                          (torch.bfloat16, True, 816), (torch.float16, True, 816), (torch.float32, True, 408)):
        assert _C.groupnorm_nhwc_route(1, 640, most, 32, dt, bwd)
        assert not _C.groupnorm_nhwc_route(1, 640, most + 1, 32, dt, bwd)
    # the batch does not enter: a workgroup owns one bundle of one sample
    assert _C.groupnorm_nhwc_route(1, 640, 1024, 32, DT, False) == _C.groupnorm_nhwc_route(64, 640, 1024, 32, DT, False)
    # a bundle of more than 32 chunks (cpg = 264 -> 264 channels) has no form
    assert not _C.groupnorm_nhwc_route(1, 528, 4, 2, DT, False)


def test_flag_off_sends_everything_streaming_and_reads_do_not_write():
    assert _C.groupnorm_nhwc_resident(-1) == 1, "resident is the default"
    assert _C.groupnorm_nhwc_resident(0) == 1
    assert _C.groupnorm_nhwc_resident(-1) == 0 and _C.groupnorm_nhwc_resident(-1) == 0
    for C, HW, *_ in STEP_SITES:
        assert not _C.groupnorm_nhwc_route(B, C, HW, G, DT, False)
        assert not _C.groupnorm_nhwc_route(B, C, HW, G, DT, True)
    assert _C.groupnorm_nhwc_resident(1) == 0 and _C.groupnorm_nhwc_resident(-1) == 1


def test_route_refuses_what_the_entry_points_refuse():
    for C, groups in ((36, 4), (40, 3)):   # C % 8 != 0, C % groups != 0
        with pytest.raises(RuntimeError, match="not supported"):
            _C.groupnorm_nhwc_route(1, C, 16, groups, DT, False)


def test_ab_override_names_the_switch():
    ns = {}
    assert ops.apply_ab_overrides("GN_RESIDENT=0", ns) == {"GN_RESIDENT": False} and ns["GN_RESIDENT"] is False
    assert ops.apply_ab_overrides("GN_RESIDENT=1", {}) == {"GN_RESIDENT": True}
    assert ops.GN_RESIDENT is True


def test_workspace_is_what_the_parent_commit_returned():
    lib = _C.require()
    for flag in (1, 0):
        _C.groupnorm_nhwc_resident(flag)
        for C, HW, _, _, _, nbytes in STEP_SITES:
            assert int(lib.lora_amd_groupnorm_nhwc_workspace(B, C, HW, G)) == nbytes, (C, HW)
