"""What tests/test_gpu_rank_sweep.py relies on, checked without a GPU: its inputs make its bounds bite, its route table names a
route for every case, and its case count is the constant written in it.

The bite: for every site kind and activation dtype, at r = 17 and r = 64, the
float64 reference and the same reference with its LAST RANK REMOVED, both rounded to the activation dtype, differ by more than
FOUR times the bound the sweep applies — in ``y - y0`` (not in ``y``: the frozen term hides a rank), ``dx``, ``d lora_up`` and
``d lora_down``.  A kernel that dropped the last rank (a live-rank mask off by one, a lost last chunk) could not pass the sweep."""
import pytest
import torch

from tests import test_gpu_rank_sweep as S

KIND_DT = sorted({(kind, dt) for kind, dt, _ in S.TESTS})


def _bite_ranks(kind):
    ranks = S.KINDS[kind].ranks
    return [r for r in (17, 64) if r in ranks] or [max(ranks)]


@pytest.mark.parametrize("kind,dt", KIND_DT, ids=[f"{k}-{d}" for k, d in KIND_DT])
def test_a_dropped_last_rank_exceeds_four_times_every_bound(kind, dt):
    kd = S.KINDS[kind]
    for r in _bite_ranks(kind):
        full, cut = S.reference(kind, dt, r), S.reference(kind, dt, r, drop_last=True)
        bnd = S.bounds(dt, full, S.on_library_conv_route(kind, dt, r))
        for q in ("low",) if kd.half else ("low", "dx", "dup", "ddown"):
            a, b = full[q], cut[q]
            if q in ("low", "dx"):      # the stored quantities; the factor gradients leave in f32
                a, b = a.to(S.DT[dt]).double(), b.to(S.DT[dt]).double()
            delta = float((a - b).abs().max())
            bound = float(torch.as_tensor(bnd[q]).max())
            assert delta > 4.0 * bound, (kind, dt, r, q, delta, bound)


def test_the_frozen_term_does_not_drown_the_branch():
    """The low-rank term of y carries about LOW_TO_FROZEN times the norm of the frozen term at the first and the last rank
    (within a factor of 2: one rank is one random direction, a selector scales it by 0.5 .. 1.5, dropout by 1 / sqrt(1 - p))."""
    for kind, dt in KIND_DT:
        ranks = S.KINDS[kind].ranks
        for r in (ranks[0], ranks[-1]):
            ref = S.reference(kind, dt, r)
            low, frozen = float(ref["low"].norm()), float((ref["y"] - ref["low"]).norm())
            assert S.LOW_TO_FROZEN / 2 <= low / frozen <= 2 * S.LOW_TO_FROZEN, (kind, dt, r, low / frozen)


def test_the_route_table_names_a_route_for_every_case():
    n = 0
    for kind, dt, hook, r in S.cases():
        route = S.expected_route(kind, dt, r, hook)
        assert isinstance(route, S.Route) and (route.log or route.launches), (kind, dt, hook, r)
        for op, cols, rank, form in route.prims:
            assert op in ("rowdot", "rank_update", "colreduce") and form in ("mfma", "valu") and 1 <= rank <= 64
            assert hook or form == "valu", (kind, dt, r, op)     # hook off: every primitive on the VALU kernels
        n += 1
    assert n == S.N_CASES


def test_the_case_count_is_the_constant():
    assert sum(len(S.KINDS[kind].ranks) for kind, _, _ in S.TESTS) == S.N_CASES == len(list(S.cases()))
    for kind, kd in S.KINDS.items():
        assert list(kd.ranks) == sorted(set(kd.ranks)) and kd.ranks[0] == 1, kind
        if kind != "lin_ring":     # 4097 rows: ranks 1..16, then 17 and 64 once
            assert set(range(1, 65)) <= set(kd.ranks), kind
    assert set(range(1, 17)) | {17, 64} == set(S.KINDS["lin_ring"].ranks)
    assert {65, 96, 128} <= set(S.KINDS["lin_lib"].ranks) and {65, 96, 128} <= set(S.KINDS["lin_drop@lib"].ranks)
    assert {65, 68} <= set(S.KINDS["conv3_cl"].ranks)
    # NCHW 3x3: the native kernels up to rank 16, the library route above, in bf16 and in f32
    for dt in ("bf16", "f32"):
        assert all("conv_down_fwd" in S.expected_route("conv3_nchw", dt, r, True).launches for r in range(1, 17))
        assert all(S.on_library_conv_route("conv3_nchw", dt, r) for r in range(17, 65))


def test_routes_of_the_recorded_defect():
    """Ranks 12 and 16 of the fused channels-last 3x3 site in bf16: the folded G pass with the hook on, ``linear_bwd_g`` +
    ``sum_parts`` with it off (the combination that raised before ``_C.linear_bwd_g_folded_ok`` asked the hook)."""
    for kind in ("conv3_cl", "conv3_cl_drop"):
        for r in (12, 16):
            on, off = S.expected_route(kind, "bf16", r, True), S.expected_route(kind, "bf16", r, False)
            assert "linear_bwd_g_folded" in on.launches and "sum_parts" not in on.launches
            assert {"linear_bwd_g", "sum_parts"} <= off.launches and "linear_bwd_g_folded" not in off.launches
