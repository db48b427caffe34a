"""match.py --pipeline: a list of pairs streamed through the matcher instead of handled one at a time on one thread.

    readers (N threads)         main thread, per slot              writer (1 thread)
    calib.txt, envelope check,  H2D of the bytes (non-blocking),   waits for the pair's event,
    PNG -> raw uint8 in pinned  ingest + match: eager, or one      PFM / PGM / time files
    host memory, list order     hipGraph replay; map -> pinned
                                host buffer + event

ListPipeline is the decode / submit / collect core: ordering, back-pressure, the capture policy and error handling.  It
knows nothing of the GPU - it is handed `read` (entry -> job, run on the reader threads), a match `backend` and `write`
(run on the writer thread), so all of that is tested on the CPU with a fake backend.  MatcherBackend is the real one.

Capture policy.  A graph costs two warm-up pairs plus a capture, and a matcher keeps one shape resident, so a slot
captures a (H, W, ndisp, C) only when it sees it for the second time in a row; first sight and alternating shapes run
eagerly (match_u8).  Once captured, a key is replayed for as long as the slot's shape (H, W, ndisp) stays.

The backend's interface:
    thread_init()                     called once on every reader / writer thread
    submit(slot, job, mode) -> ticket mode in ("eager", "capture", "replay"); enqueues, never blocks on the GPU
    wait(ticket) -> result            blocks until the pair's map is on the host (writer thread, and main on slot reuse)
    retire(slot, job, ticket)         the slot is about to be reused; returns None, or the ticket of a repeated pair
                                      (the saturation redo of match.py) whose result replaces the first one's files
"""
import collections
import os
import queue
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import util

DEFAULT_READERS = 4          # the GPU hosts allow a process 16 CPUs; never sized by os.cpu_count()


class Job(object):
    """One decoded pair: what a reader hands to the main thread."""

    def __init__(self, index, name, key, **fields):
        self.index = index           # position in the list file
        self.name = name             # for the log
        self.key = key               # (H, W, ndisp, C): what a captured graph is good for
        self.__dict__.update(fields)


class ListPipeline(object):
    def __init__(self, read, backend, write, slots=1, readers=DEFAULT_READERS, depth=None, writer_depth=8):
        self.read, self.backend, self.write = read, backend, write
        self.slots = max(1, int(slots))
        self.readers = max(1, int(readers))
        # jobs handed to the readers and not yet taken by the main thread (being decoded or waiting, decoded): the bound
        # of the reader queue - pinned host memory in use is at most this many pairs + the pairs in flight
        self.depth = max(1, int(depth if depth is not None else 2 * self.readers))
        self.writer_depth = max(1, int(writer_depth))
        self.counters = dict(pairs=0, captures=0, replays=0, eager=0, redone=0)
        # where the wall time went: the main thread waiting for a decoded pair / for a slot's previous pair / enqueuing,
        # and the writer thread waiting for maps / writing files (which stage bounds the run: tools/bench_list.py)
        self.seconds = dict(main_wait_readers=0.0, main_wait_slot=0.0, main_submit=0.0, writer_wait_gpu=0.0,
                            writer_files=0.0)
        self.submitted_at = []       # host clock at every submit: the steady rate behind the first pairs' capture
        self.max_read_ahead = 0      # the largest number of outstanding reader jobs seen (tests: <= depth)
        self._last_key = [None] * self.slots
        self._captured = [set() for _ in range(self.slots)]

    # ---- capture policy -------------------------------------------------------------------------------------------
    def mode_for(self, slot, key):
        """'replay' for a key this slot has captured, 'capture' when the slot sees the key for the second time in a row,
        'eager' otherwise.  A change of shape (everything but the channel count) drops the slot's captured keys: the
        matcher keeps one shape resident."""
        last = self._last_key[slot]
        if last is not None and tuple(last[:3]) != tuple(key[:3]):
            self._captured[slot].clear()
        self._last_key[slot] = key
        if key in self._captured[slot]:
            return "replay"
        if key == last:
            self._captured[slot].add(key)
            return "capture"
        return "eager"

    # ---- writer thread --------------------------------------------------------------------------------------------
    def _writer_loop(self):
        failed = False
        try:
            self.backend.thread_init()
        except BaseException as e:       # noqa: B902 - handed to the main thread
            self._writer_error, failed = e, True
        while True:
            item = self._writer_q.get()
            if item is None:
                return
            if failed:
                continue                 # keep draining: the main thread must never block on a full queue
            job, ticket, t0 = item
            try:
                t1 = time.time()
                result = self.backend.wait(ticket)
                t2 = time.time()
                job.vertical = getattr(ticket, "vertical", None)     # (a repeated pair's ticket brings its own)
                self.write(job, result, t2 - t0)
                self.seconds["writer_wait_gpu"] += t2 - t1
                self.seconds["writer_files"] += time.time() - t2
            except BaseException as e:   # noqa: B902
                self._writer_error, failed = e, True

    def _check_writer(self):
        if self._writer_error is not None:
            raise self._writer_error

    # ---- main thread ----------------------------------------------------------------------------------------------
    def _retire(self, slot, inflight):
        if inflight[slot] is None:
            return
        job, ticket, t0 = inflight[slot]
        inflight[slot] = None
        again = self.backend.retire(slot, job, ticket)
        if again is not None:            # repeated pair: written after (and over) the first result, same writer
            self.counters["redone"] += 1
            self._writer_q.put((job, again, t0))

    def run(self, entries):
        """Matches `entries` in order; returns the counters.  An exception of a reader, of the backend or of the writer
        ends the run: the pairs already submitted are still written (unless the writer is what failed), every thread
        is joined, and the exception is raised."""
        entries = list(entries)
        self._writer_error = None
        self._writer_q = queue.Queue(maxsize=self.writer_depth)
        writer = threading.Thread(target=self._writer_loop, name="list-writer", daemon=True)
        pool = ThreadPoolExecutor(max_workers=self.readers, thread_name_prefix="list-reader",
                                  initializer=self.backend.thread_init)
        inflight = [None] * self.slots
        futures = []
        fed = 0
        writer.start()
        try:
            for n in range(len(entries)):
                while fed < len(entries) and fed - n < self.depth:
                    futures.append(pool.submit(self.read, entries[fed]))
                    fed += 1
                self.max_read_ahead = max(self.max_read_ahead, fed - n)
                ta = time.time()
                job = futures[n].result()            # list order; a reader's exception surfaces here
                futures[n] = None
                self._check_writer()
                slot = n % self.slots
                tb = time.time()
                self._retire(slot, inflight)         # the oldest pair is the one that used this slot
                mode = self.mode_for(slot, job.key)
                t0 = time.time()
                self.submitted_at.append(t0)
                ticket = self.backend.submit(slot, job, mode)
                self.seconds["main_wait_readers"] += tb - ta
                self.seconds["main_wait_slot"] += t0 - tb
                self.seconds["main_submit"] += time.time() - t0
                self.counters["pairs"] += 1
                self.counters[{"eager": "eager", "capture": "captures", "replay": "replays"}[mode]] += 1
                inflight[slot] = (job, ticket, t0)
                self._writer_q.put((job, ticket, t0))
            for k in range(self.slots):              # oldest first
                self._retire((len(entries) + k) % self.slots, inflight)
        finally:
            for f in futures:
                if f is not None:
                    f.cancel()
            pool.shutdown(wait=True)
            self._writer_q.put(None)
            writer.join()
        self._check_writer()
        return dict(self.counters)

    def summary(self):
        c = self.counters
        return "pipeline: pairs=%d captures=%d replays=%d eager=%d" % (c["pairs"], c["captures"], c["replays"], c["eager"])


# ---- the readers' side of match.py ------------------------------------------------------------------------------------
def decode_u8(path):
    """A PNG as raw bytes: uint8 [H,W] ('L'), [H,W,3] ('RGB') or [H,W,4] ('RGBA') as stored - no grey conversion, no
    float.  Any other PIL mode goes through the same convert() calls as util.read_gray up to its uint8 array."""
    from PIL import Image
    im = Image.open(path)
    if im.mode in ("L", "P", "1", "I;16", "I"):
        if im.mode != "L":
            im = im.convert("L")
    elif im.mode not in ("RGB", "RGBA"):
        im = im.convert("RGB")
    return np.asarray(im, dtype=np.uint8)


def _three_channels(a):
    """[H,W] or [H,W,4] -> [H,W,3] with the same grey value: (v, v, v) maps to v, alpha is ignored anyway."""
    return np.repeat(a[:, :, None], 3, axis=2) if a.ndim == 2 else a[:, :, :3]


def pinned_u8(a):
    import torch
    t = torch.empty(a.shape, dtype=torch.uint8, pin_memory=True)
    np.copyto(t.numpy(), a)
    return t


def pinned(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory()


def make_reader(paths, check_shape, to_host_buffer=pinned_u8, truth=None, shape=None, truth_right=None, calibration=None):
    """read(index) for ListPipeline on top of match.py's file layout.  `paths(index)` -> dict(left, right, calib, out,
    out_time, out_img, res_dir, img_dir[, dirs: every directory the outputs need]); `check_shape(H, W, ndisp)` raises for
    a pair outside the envelope - before anything of that pair reaches the GPU.  `shape`: None - the size and ndisp are
    those of the pair's calib.txt, checked before anything is decoded - or shape(left_path, left_image) -> (H, W, ndisp)
    for a data set whose size is the decoded left image's (datasets.py: the KITTI layouts).  `truth(left_path)` (match.py
    --evaluate: the layout's load_truth) -> (ground truth, mask or None) or None: read here as well, into pinned memory
    beside the images (job.gt, job.mask; job.gt None = a pair without ground truth).  `truth_right` (--views both): the
    same for the right view's ground truth (job.gt_right, job.mask_right).  `calibration(paths)` (match.py --depth /
    --point_cloud) -> the pair's calibration (hashable): read here as well (job.calib) and appended to the job's key, since
    a captured graph holds it by value - the capture policy then replays a pair only where shape and calibration repeat."""
    def read(index):
        p = paths(index)
        if shape is None:
            height, width, ndisp = util.parseCalib(p["calib"])
            check_shape(height, width, ndisp)
        for d in p.get("dirs", (p["res_dir"], p["img_dir"])):
            util.recurMk(os.path.abspath(d))
        left = decode_u8(p["left"])
        if shape is not None:
            height, width, ndisp = shape(p["left"], left)
            check_shape(height, width, ndisp)
        right = decode_u8(p["right"])
        if left.shape[2:] != right.shape[2:]:
            left, right = _three_channels(left), _three_channels(right)
        for a, which in ((left, p["left"]), (right, p["right"])):
            if a.shape[:2] != (height, width):
                raise ValueError("%s is %dx%d, %s says %dx%d" % (which, a.shape[1], a.shape[0],
                                                                 "its calib.txt" if shape is None else "the left view",
                                                                 width, height))
        channels = 1 if left.ndim == 2 else left.shape[2]
        def pinned_truth(load, what):
            found = load(p["left"]) if load is not None else None
            if found is None:
                return None, None
            if found[0].shape != (height, width):
                raise ValueError("%s: the %s is %s, the disparity map %s (resampling is not supported)"
                                 % (p["left"], what, found[0].shape, (height, width)))
            return pinned(found[0]), (pinned(found[1]) if found[1] is not None else None)

        gt, mask = pinned_truth(truth, "ground truth")
        gt_right, mask_right = pinned_truth(truth_right, "right view's ground truth")
        calib = calibration(p) if calibration is not None else None
        key = (height, width, ndisp, channels) + ((calib,) if calib is not None else ())
        return Job(index, p["left"], key, height=height, width=width, ndisp=ndisp,
                   left=to_host_buffer(left), right=to_host_buffer(right), paths=p, gt=gt, mask=mask, gt_right=gt_right,
                   mask_right=mask_right, calib=calib)
    return read


def _save_middlebury(result, p):
    util.saveDisparity(result.map, p["out_img"])
    util.writePfm(result.map, p["out"])


def make_writer(rank=0, log=print, scorer=None, eval_file="evalMCCNN.json", save=_save_middlebury, save_vertical=None):
    """write(job, result, seconds) for ListPipeline: the files of match.py, with the existing util functions; with a
    `scorer` (evaluation.ListScorer, match.py --evaluate) also the evaluation of a pair that was scored (job.scored: of
    the map these files hold, or of the repeat that replaces it), once its bytes are on the host.  `save(result, paths)`
    writes what the PairResult of host arrays holds: the map and its preview (datasets.py: a KITTI layout's is the 16-bit
    plane), the planes (--confidence) and the sparse map (--semi_dense) - a repeated pair's files get the repeated
    pair's.  `save_vertical(offset, totals, paths[, field, cell_totals])` (match.py --vertical_offset auto | grid) writes
    the measured row offset, and the field, of a pair whose ticket brought them."""
    from datetime import datetime

    def write(job, result, seconds):
        p = job.paths
        save(result, p)
        vertical = getattr(job, "vertical", None)
        if save_vertical is not None and vertical is not None:
            save_vertical(vertical[0].numpy(), vertical[1].numpy(), p, *(v.numpy() for v in vertical[2:]))
        util.saveTimeFile(seconds, p["out_time"])
        log("[{}] {}: {:.3f} s -> {}".format(rank, datetime.now(), seconds, p["out"]))
        if scorer is not None and job.scored is not None:
            scorer.publish(job.scored, p.get("out_eval") or os.path.join(p["res_dir"], eval_file))
    return write


def slot_comes_round(redo, rematch, scorer, scored, result, slot, slot_stream, synchronize):
    """What every list loop does with a pair (its results complete) when its slot is about to be reused.  The saturation
    redo (stereo_device.SaturationRedo) is asked; a pair that is due is matched again by rematch() -> (anything, the
    repeat's PairResult on the device), and the device is synchronised.  A pair that is scored (`scored` not None) is then
    committed under slot_stream(): the slot's result buffer and scratch belong to that stream, and the commit runs in
    front of the slot's next pair, which overwrites a replayed graph's static output; the total takes the result that
    is kept, once, in list order, and a repeated pair is scored again first.  `result`: the PairResult of the first
    match, its map what is scored.  Returns what rematch() returned, or None."""
    again = None
    if redo.due():
        again = rematch()
        result = again[1]
        synchronize()
    if scored is not None:
        with slot_stream():
            if again is not None:
                scorer.score(scored, result, slot)       # not the discarded map
            scorer.commit(scored, result)
        if again is not None:
            synchronize()                                # the library matcher's output is overwritten by the next repeat
    return again


# A pair enqueued by MatcherBackend.  host: the PairResult of pinned host tensors its results are copied to; done: the
# event behind the copies; device: the PairResult on the device, its map what an evaluation scores (a KITTI layout: what
# the written PNG holds, not the matcher's map).
# vertical: the pinned host tensors (offset, totals) of a matcher that measures the row offset, else None.
Ticket = collections.namedtuple("Ticket", "host done device vertical", defaults=(None,))


class MatcherBackend(object):
    """ListPipeline's backend on StereoMatchers: one matcher and one stream per slot, as match.py --pairs_in_flight.

    scorer (evaluation.ListScorer, match.py --evaluate): a pair is scored behind the graph replay on the slot's stream,
    NOT inside the captured graph - the thresholds stay call-time arguments - and the running total takes it only in
    retire(), once it is known which map is kept (the saturation redo), in list order.  Its record hangs on the job
    (job.scored), where the writer thread finds it.
    device_output(map, scored) -> (what crosses to the host for a map, what is scored), enqueued behind the map on the
    slot's stream and like the evaluation not inside the graph (a KITTI layout: the 16-bit code, half the bytes, and what
    the file holds); None: the map itself."""

    def __init__(self, matchers, streams, make_library_matcher, rank=0, log=print, scorer=None, device_output=None,
                 vertical=False):
        import torch
        import stereo_device
        self.torch = torch
        self.matchers, self.streams = matchers, streams
        self.redo = stereo_device.SaturationRedo(matchers, make_library_matcher)
        self.device = torch.cuda.current_device()
        self.rank, self.log = rank, log
        self.scorer, self.device_output = scorer, device_output
        self.vertical = bool(vertical)       # the matchers measure the row offset: it crosses with the map

    def thread_init(self):
        self.torch.cuda.set_device(self.device)      # the current device is a per-thread setting

    def _stream(self, slot):
        import contextlib
        s = self.streams[slot]
        return self.torch.cuda.stream(s) if s is not None else contextlib.nullcontext()

    def _to_host(self, result, matcher=None, job=None):
        """The PairResult a matcher returned on its way to pinned host memory: map, planes, sparse map, the measured row
        offset of `job` on `matcher` where there is one, then the event."""
        torch = self.torch
        crossing = scored = result.map
        if self.device_output is not None:
            crossing, scored = self.device_output(result.map, self.scorer is not None)

        def pinned_copy(t):
            host = torch.empty(tuple(t.shape), dtype=t.dtype, pin_memory=True)
            return host.copy_(t, non_blocking=True)
        host = result._replace(map=crossing).apply(pinned_copy)
        vertical = None
        if self.vertical and matcher is not None:
            vertical = tuple(pinned_copy(b) for b in matcher.vertical_buffers(job.height, job.width, job.ndisp))
        done = torch.cuda.Event()
        done.record()
        return Ticket(host, done, result._replace(map=scored), vertical)

    def _truth(self, gt, mask, dev):
        """The reader's pinned ground truth on its way to the device, behind the pair on the slot's stream."""
        if gt is None:
            return None
        return gt.to(dev, non_blocking=True), (mask.to(dev, non_blocking=True) if mask is not None else None)

    def submit(self, slot, job, mode):
        self.log("[{}] pair {}: {}  ({}x{}, ndisp {}, {} byte(s) per pixel, {})".format(
            self.rank, job.index, job.name, job.width, job.height, job.ndisp, job.key[3], mode))
        m = self.matchers[slot]
        if getattr(job, "calib", None) is not None:      # a launch argument of the metric outputs, and part of the graph's key
            m.set_calibration(job.calib)
        with self._stream(slot):
            match = m.match_u8 if mode == "eager" else m.match_graph_u8
            ticket = self._to_host(m.result_of(match(job.left, job.right, job.ndisp)), m, job)
            if self.scorer is not None:
                # (the right view's truth crosses only where the pair is scored at all, and in front of the left's)
                truth_right = self._truth(job.gt_right, job.mask_right, m.device) if job.gt is not None else None
                job.scored = self.scorer.begin(job.index, job.name, self._truth(job.gt, job.mask, m.device), truth_right)
                if job.scored is not None:
                    self.scorer.score(job.scored, ticket.device, slot)
            return ticket

    def wait(self, ticket):
        ticket.done.synchronize()
        return ticket.host.apply(lambda t: t.numpy())

    def retire(self, slot, job, ticket):
        ticket.done.synchronize()

        def rematch():
            library = self.redo.matcher()
            self.log("[{}] ".format(self.rank) + self.redo.notice(job.paths["out"]))
            if getattr(job, "calib", None) is not None:
                library.set_calibration(job.calib)
            again = self._to_host(library.result_of(library.match_u8(job.left, job.right, job.ndisp)), library, job)
            return again, again.device
        again = slot_comes_round(self.redo, rematch, self.scorer, job.scored if self.scorer is not None else None,
                                 ticket.device, slot, lambda: self._stream(slot), self.torch.cuda.synchronize)
        return again[0] if again is not None else None
