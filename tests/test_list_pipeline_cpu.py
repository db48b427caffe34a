"""CPU: the decode / submit / collect core of match.py --pipeline (list_matcher.ListPipeline) with a fake backend:
ordering, the capture policy, back-pressure and error handling."""
import threading
import time

import numpy as np
import pytest

import list_matcher as lm


class FakeBackend(object):
    """'Matches' a job by returning its index and key; records what it was asked to do."""

    def __init__(self, saturate_at=()):
        self.calls = []              # (slot, index, mode) in submit order
        self.retired = []
        self.threads = set()
        self.saturate_at = set(saturate_at)

    def thread_init(self):
        self.threads.add(threading.current_thread().name)

    def submit(self, slot, job, mode):
        self.calls.append((slot, job.index, mode))
        return ("ticket", job.index, mode)

    def wait(self, ticket):
        time.sleep(0.001)
        return ticket

    def retire(self, slot, job, ticket):
        self.retired.append((slot, job.index))
        if job.index in self.saturate_at:
            return ("ticket", job.index, "redo")
        return None


def _reader(keys, delay=None, fail_at=None, live=None):
    def read(i):
        if delay:
            time.sleep(delay(i))
        if fail_at is not None and i == fail_at:
            raise KeyError("reader failed on entry %d" % i)
        if live is not None:
            live.append(i)
        return lm.Job(i, "pair%d" % i, keys[i])
    return read


def _no_pipeline_threads():
    return not [t for t in threading.enumerate() if t.name.startswith(("list-reader", "list-writer"))]


A, B, C3 = (40, 64, 16, 1), (32, 48, 8, 1), (40, 64, 16, 3)


def test_outputs_in_list_order_with_mixed_shapes():
    keys = [A, B, A, A, B, B, A, C3, A, B, A, A]
    written = []
    # later entries decode faster than earlier ones: order must still be the list's
    p = lm.ListPipeline(_reader(keys, delay=lambda i: 0.002 * (len(keys) - i)), FakeBackend(),
                        lambda job, res, sec: written.append((job.index, res[1], sec)), slots=2, readers=4)
    counters = p.run(range(len(keys)))
    assert [w[0] for w in written] == list(range(len(keys))) and all(w[0] == w[1] for w in written)
    assert all(w[2] >= 0 for w in written)
    assert counters["pairs"] == len(keys) == counters["captures"] + counters["replays"] + counters["eager"]
    assert [c[0] for c in p.backend.calls] == [i % 2 for i in range(len(keys))]         # slots round-robin
    assert [r[1] for r in p.backend.retired] == list(range(len(keys)))                 # every pair retired, oldest first
    assert _no_pipeline_threads()


def test_capture_policy_run_of_equal_shapes():
    """Four equal shapes in one slot: the first eager, the second captures, the third and fourth only replay."""
    b = FakeBackend()
    p = lm.ListPipeline(_reader([A] * 4), b, lambda *a: None, slots=1)
    counters = p.run(range(4))
    assert [c[2] for c in b.calls] == ["eager", "capture", "replay", "replay"]
    assert (counters["eager"], counters["captures"], counters["replays"]) == (1, 1, 2)
    assert p.summary() == "pipeline: pairs=4 captures=1 replays=2 eager=1"


def test_capture_policy_alternating_shapes_never_capture():
    b = FakeBackend()
    p = lm.ListPipeline(_reader([A, B] * 4), b, lambda *a: None, slots=1)
    assert p.run(range(8))["captures"] == 0
    assert {c[2] for c in b.calls} == {"eager"}
    # ... but with two slots every slot sees one shape only: each captures on its second pair
    b = FakeBackend()
    p = lm.ListPipeline(_reader([A, B] * 4), b, lambda *a: None, slots=2)
    assert p.run(range(8)) == dict(pairs=8, captures=2, replays=4, eager=2, redone=0)
    assert [c[2] for c in b.calls] == ["eager"] * 2 + ["capture"] * 2 + ["replay"] * 4


def test_capture_policy_shape_change_drops_the_graph_channel_change_keeps_it():
    b = FakeBackend()
    #        eager capture replay eager(C)  replay eager(B) eager  capture
    keys = [A,    A,      A,     C3,       A,     B,       A,     A]
    lm.ListPipeline(_reader(keys), b, lambda *a: None, slots=1).run(range(len(keys)))
    assert [c[2] for c in b.calls] == ["eager", "capture", "replay", "eager", "replay", "eager", "eager", "capture"]


def test_reader_queue_never_exceeds_its_bound():
    keys = [A] * 40
    live = []
    taken = []

    class Slow(FakeBackend):
        def submit(self, slot, job, mode):
            time.sleep(0.003)                        # the consumer is the bottleneck: the readers run ahead
            taken.append(job.index)
            # read and not yet consumed, this job included
            assert len(live) - len(taken) + 1 <= 3, (len(live), len(taken))
            return FakeBackend.submit(self, slot, job, mode)

    p = lm.ListPipeline(_reader(keys, live=live), Slow(), lambda *a: None, slots=1, readers=4, depth=3)
    p.run(range(len(keys)))
    assert 1 <= p.max_read_ahead <= 3
    assert sorted(live) == list(range(40))


def test_a_reader_that_raises_ends_the_run_with_its_exception():
    keys = [A] * 12
    written = []
    p = lm.ListPipeline(_reader(keys, fail_at=5), FakeBackend(), lambda job, res, sec: written.append(job.index),
                        slots=2, readers=3)
    with pytest.raises(KeyError, match="reader failed on entry 5"):
        p.run(range(len(keys)))
    assert written == [0, 1, 2, 3, 4]                # what was submitted before it is still written, in order
    assert _no_pipeline_threads()


def test_a_writer_that_raises_ends_the_run_with_its_exception():
    def write(job, res, sec):
        if job.index == 3:
            raise OSError("disk full")
    p = lm.ListPipeline(_reader([A] * 30), FakeBackend(), write, slots=1, writer_depth=2)
    with pytest.raises(OSError, match="disk full"):
        p.run(range(30))
    assert p.counters["pairs"] < 30                  # the run stopped early
    assert _no_pipeline_threads()


def test_saturation_redo_is_written_over_the_first_result():
    written = []
    b = FakeBackend(saturate_at={2})
    p = lm.ListPipeline(_reader([A] * 5), b, lambda job, res, sec: written.append((job.index, res[2])), slots=1)
    assert p.run(range(5))["redone"] == 1
    assert [w for w in written if w[0] == 2] == [(2, "replay"), (2, "redo")]
    assert [w[0] for w in written] == [0, 1, 2, 2, 3, 4]     # repeated before its slot is reused


def test_decode_u8_keeps_the_stored_bytes(tmp_path):
    from PIL import Image
    import util
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, size=(9, 11, 3), dtype=np.uint8)
    rgba = rng.integers(0, 256, size=(9, 11, 4), dtype=np.uint8)
    grey = rng.integers(0, 256, size=(9, 11), dtype=np.uint8)
    for name, arr, mode in (("rgb", rgb, "RGB"), ("rgba", rgba, "RGBA"), ("l", grey, "L")):
        path = str(tmp_path / (name + ".png"))
        Image.fromarray(arr, mode=mode).save(path)
        got = lm.decode_u8(path)
        assert got.dtype == np.uint8 and np.array_equal(got, arr)
        # the device's grey formula on those bytes is util.read_gray
        if got.ndim == 3:
            c = got[:, :, :3].astype(np.uint32)
            g = ((c[:, :, 0] * 9797 + c[:, :, 1] * 19234 + c[:, :, 2] * 3737) >> 15).astype(np.uint8)
        else:
            g = got
        assert np.array_equal(g, util.read_gray(path))
    pal = Image.fromarray(grey, mode="L").convert("P")
    pal.save(str(tmp_path / "p.png"))
    assert np.array_equal(lm.decode_u8(str(tmp_path / "p.png")), util.read_gray(str(tmp_path / "p.png")))
    assert np.array_equal(lm._three_channels(grey)[:, :, 1], grey) and lm._three_channels(rgba).shape == (9, 11, 3)


def test_reader_refuses_a_shape_outside_the_envelope_before_decoding(tmp_path):
    import stereo_device as sd
    d = tmp_path / "p"
    d.mkdir()
    (d / "calib.txt").write_text("a\nb\nc\nd\nwidth=64\nheight=40\nndisp=2000\n")
    paths = lambda i: dict(left=str(d / "im0.png"), right=str(d / "im1.png"), calib=str(d / "calib.txt"),   # noqa: E731
                           res_dir=str(tmp_path / "r"), img_dir=str(tmp_path / "i"), out="", out_time="", out_img="")
    read = lm.make_reader(paths, lambda h, w, nd: sd.check_envelope(h, w, nd), to_host_buffer=lambda a: a)
    with pytest.raises(ValueError, match="ndisp=2000"):     # im0.png does not even exist: nothing was decoded
        read(0)
    assert not (tmp_path / "r").exists()
