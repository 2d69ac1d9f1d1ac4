"""Self-tests of tests/memguard.py: each shows that the harness reports the error it exists to catch."""
import pytest
import torch

from tests import memguard as MG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.uint8])
@pytest.mark.parametrize("align", [256, 16])
def test_a_byte_written_into_a_guard_is_reported_with_its_offset(dt, align):
    g = MG.Guarded((3, 37), dt, DEV, align=align)
    assert g.ptr % align == 0 and (align == 256 or g.ptr % 32 == 16)
    assert g.guard >= 64 * 1024
    g.data.zero_()
    g.check("untouched")                                   # writing the data is fine
    end = g.off + g.nbytes
    g.raw[end + 5] ^= 0x01
    with pytest.raises(AssertionError, match=r"after the data changed: first changed byte at \+5 bytes"):
        g.check("overrun")
    g.raw[end + 5] ^= 0x01
    g.check("restored")
    g.raw[g.off - 3] = 0
    with pytest.raises(AssertionError, match=r"before the data changed: first changed byte at -3 bytes"):
        g.check("underrun")


def test_float_sentinels_are_nans_no_arithmetic_produces():
    """A NaN made by arithmetic (0 / 0, inf - inf, sqrt(-1)) is never the sentinel.  Arithmetic ON the sentinel carries
    its payload through: an output element holding it was either never written or computed from an over-read."""
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        g = MG.Guarded((8,), dt, DEV)
        assert bool(torch.isnan(g.data).all()) and bool(MG.is_sentinel(g.data).all())
        zero = torch.zeros((), dtype=dt, device=DEV)
        made = torch.stack([zero / 0, torch.full((), float("inf"), dtype=dt, device=DEV) - float("inf"), (zero - 1).sqrt()])
        assert bool(torch.isnan(made).all()) and not bool(MG.is_sentinel(made).any()), dt
        # arithmetic on the input poison keeps the poison's payload: never the output sentinel
        pz = MG.poisoned(torch.ones(4, dtype=dt, device=DEV))._memguard.raw[:64].view(dt)
        assert bool(torch.isnan(pz).all()) and not bool(MG.is_sentinel(torch.stack([pz[0] * 0.75, pz[0] + 1])).any()), dt


def test_a_sentinel_left_inside_an_output_is_reported():
    g = MG.Guarded((4, 16), torch.float32, DEV)
    g.data[:, :15] = 1.0
    MG.assert_untouched(g.data[:, 15:], "pad column")
    with pytest.raises(AssertionError, match="4 of 64 elements of the written set still hold the sentinel"):
        MG.assert_written(g.data, "output")
    g.data[2, 15] = 0.0
    with pytest.raises(AssertionError, match="1 of 4 elements outside the written set changed"):
        MG.assert_untouched(g.data[:, 15:], "pad column")


def test_poisoned_inputs_hold_nan_in_row_gaps_and_around():
    src = torch.arange(12, dtype=torch.bfloat16, device=DEV).view(3, 4)
    v = MG.poisoned(src, ld=8)
    assert v.stride(0) == 8 and torch.equal(v, src)
    assert bool(torch.isnan(v._memguard.data[:, 4:]).all())
    flat = MG.poisoned(src)
    raw = flat._memguard.raw
    assert bool(torch.isnan(raw[:flat._memguard.off].view(torch.bfloat16)).all())


def test_freed_storage_read_through_its_old_pointer_is_nan_after_poisoning():
    keep = torch.ones(256, device=DEV)                     # live neighbours must not be touched
    x = torch.ones(4096, device=DEV)
    ptr = x.data_ptr()
    del x
    blocks = MG.free_blocks()
    assert any(a <= ptr < a + n for a, n in blocks), "the freed block is not among the free blocks"
    has_addr = all("address" in b for seg in torch.cuda.memory_snapshot() for b in seg["blocks"])
    print(f"snapshot blocks carry 'address': {has_addr}")
    assert MG.poison_free_blocks() >= 4096 * 4
    words = MG.read_words(ptr, 4096)
    assert bool((words == MG._signed(MG.POISON_WORD, 32)).all())
    assert bool(torch.isnan(words.view(torch.float32)).all())
    assert bool((keep == 1).all())


def test_poisoning_reaches_the_private_pool_of_a_captured_graph():
    """A block freed inside a capture is a free block of the graph's private pool: it is poisoned and reads back as such."""
    static = torch.ones(1 << 16, device=DEV)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            (static * 2).sum()
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(g):
            tmp = static * 3                                 # freed inside the capture: a free block of the graph's pool
            out = tmp.sum()
            del tmp
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    pool = tuple(g.pool())
    blocks = [(int(b["address"]), int(b["size"])) for seg in torch.cuda.memory_snapshot()
              if tuple(seg.get("segment_pool_id", (0, 0))) == pool for b in seg["blocks"] if b["state"] == "inactive"]
    assert blocks, "no free block in the graph's private pool"
    assert all(any(a <= x < a + n for x, _ in MG.free_blocks()) for a, n in blocks)
    MG.poison_free_blocks()
    a, n = max(blocks, key=lambda b: b[1])
    words = MG.read_words(a, min(n // 4, 4096))
    assert bool((words == MG._signed(MG.POISON_WORD, 32)).all())
    g.replay()
    torch.cuda.synchronize()
    assert float(out) == 3.0 * (1 << 16)
