"""CPU: the memory harness (tests/arena.py) on host tensors with planted violations - each one must be reported, so that
the harness is not the thing that cannot fail - and a clean case that must pass."""
import numpy as np
import pytest
import torch

import arena as A

NBYTES = 1 << 20
G = 4096           # a small guard keeps these arenas small; the GPU cases use the default 64 KiB
H, W, D, DP = 3, 5, 6, 8


def _case(plant=None):
    """A 'kernel' in torch: out[h, w] = min over d < D of vol[h, w, d], and a byte map next to it."""
    def case(arena):
        rng = np.random.default_rng(0)
        v = np.zeros((H, W, DP), np.float32)
        v[..., :D] = rng.random((H, W, D), dtype=np.float32)
        vol = arena.put(v, guard=G, name="vol", pads_from=D)
        out = arena.take((H, W), torch.float32, guard=G, name="out", output=True)
        flags = arena.take((7,), torch.uint8, guard=G, name="flags", output=True)
        arena.poison()
        out.copy_(vol[..., :D].min(-1).values)
        flags.fill_(3)
        if plant == "before":
            e = arena.entry_of(out)
            arena.base[e.start - 4:e.start] = 1          # one element in front of `out`, inside the arena
        elif plant == "after":
            e = arena.entry_of(out)
            arena.base[e.start + e.nbytes:e.start + e.nbytes + 4] = 1
        elif plant == "after_bytes":
            e = arena.entry_of(flags)
            arena.base[e.start + e.nbytes + 2] = 9
        elif plant == "pad":
            out[1, 2] = vol[1, 2, D]                     # an unmasked lane
        elif plant == "pad_min":
            out.copy_(vol.min(-1).values)                # the minimum over all Dp lanes: wrong under fill A only
        elif plant == "red_zone":
            e = arena.entry_of(vol)
            out[0, 0] = arena.base[e.start + e.nbytes:e.start + e.nbytes + 4].view(torch.float32)[0]   # one past the end
        elif plant == "unwritten":
            out[2, 4] = arena.base[arena.entry_of(out).start - 4:arena.entry_of(out).start].view(torch.float32)[0]
        return {"out": out, "flags": flags, "vol": vol}
    return case


def test_take_alignment_guards_and_fills():
    a = A.Arena(NBYTES, "cpu")
    for mod in (0, 4, 8, 12, 0):
        t = a.take((H, W, DP), torch.float32, base_mod16=mod, guard=G, pads_from=D)
        assert t.data_ptr() % 16 == mod and t.is_contiguous() and tuple(t.shape) == (H, W, DP)
        e = a.entry_of(t)
        assert e.start - G >= 0 and e.start + e.nbytes + G <= a.base.numel()
    b = a.take((5,), torch.uint8, guard=G)
    starts = sorted((e.start - e.guard, e.start + e.nbytes + e.guard) for e in a.entries)
    assert all(x[1] <= y[0] for x, y in zip(starts, starts[1:])), "red zones overlap a neighbour"
    with pytest.raises(ValueError):
        a.take((4,), torch.float32, base_mod16=2, guard=G)
    for fill, fbits, byte in (("A", 0xFF800000, 0xFF), ("B", 0x7FC00001, 0x00)):
        a.poison(fill)
        for e in a.entries[:-1]:
            assert (e.tensor[..., D:].numpy().view(np.uint32) == fbits).all()
            for lo in (e.start - G, e.start + e.nbytes):
                assert (a.base[lo:lo + G].numpy().view(np.uint32) == fbits).all()
        e = a.entries[-1]
        assert (a.base[e.start - G:e.start].numpy() == byte).all() and (a.base[e.start + 5:e.start + 5 + G].numpy() == byte).all()
        a.check()
        assert a.holds_fill(a.entries[0].tensor[..., D:]) and not a.holds_fill(torch.full((3,), 1, dtype=torch.uint8))
    assert np.isneginf(np.array([0xFF800000], np.uint32).view(np.float32)[0])
    assert np.isnan(np.array([0x7FC00001], np.uint32).view(np.float32)[0])


def test_a_clean_case_passes_and_returns_both_runs():
    ra, rb = A.run_twice(_case(), NBYTES, "cpu")
    assert np.array_equal(ra["out"], rb["out"]) and (ra["flags"] == 3).all()
    assert np.isneginf(ra["vol"][..., D:]).all() and np.isnan(rb["vol"][..., D:]).all()     # whole tensors come back


@pytest.mark.parametrize("plant,names", [("before", ("out", "before", "-4 .. -1")),
                                         ("after", ("out", "after", "+%d .. +%d" % (H * W * 4, H * W * 4 + 3))),
                                         ("after_bytes", ("flags", "after", "+9 .. +9"))])
def test_a_write_outside_a_buffer_is_reported_with_buffer_side_and_offsets(plant, names):
    with pytest.raises(A.Violation) as e:
        A.run_twice(_case(plant), NBYTES, "cpu")
    msg = str(e.value)
    assert "red zones changed" in msg and all(n in msg for n in names), msg


@pytest.mark.parametrize("plant", ["pad", "pad_min", "red_zone", "unwritten"])
def test_an_output_that_depends_on_a_pad_or_a_red_zone_is_reported(plant):
    with pytest.raises(A.Violation) as e:
        A.run_twice(_case(plant), NBYTES, "cpu")
    msg = str(e.value)
    assert "depend on the fill" in msg and msg.count("out:") == 1 and "flags" not in msg, msg


def test_check_needs_poison_and_a_case_must_poison():
    a = A.Arena(NBYTES, "cpu")
    a.take((4,), torch.float32, guard=G)
    with pytest.raises(RuntimeError):
        a.check()
    with pytest.raises(AssertionError):
        A.run_twice(lambda arena: {"x": arena.take((4,), torch.float32, guard=G)}, NBYTES, "cpu")
    with pytest.raises(MemoryError):
        a.take((NBYTES,), torch.uint8, guard=G)
