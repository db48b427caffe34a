"""GPU: mccnn_evaluate_quantiles and mccnn_evaluate_quantiles_pooled against their NumPy restatement
(tests/quantiles_reference.py) - n_scored, every rank, every value as its uint32 bit pattern - on the shapes and contents
where the radix selection can go wrong, then the pool, graph capture and the Python layers."""
import numpy as np
import pytest

import quantiles_reference as qref

pytestmark = pytest.mark.gpu

A4 = qref.MIDDLEBURY
# several in one first-pass bin, two equal, unordered, both ends
Q8 = (990000, 500000, 900000, 500000, 890000, 1, 1000000, 880000)
SHAPES = [(1, 1, True), (1, 3, True), (1, 1023, True), (1, 1024, True), (1, 1025, True), (3, 7, True), (37, 53, True),
          (64, 96, False), (257, 259, True)]


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _got(result):
    """All eight entries of both regions, whatever n_q was."""
    import _hipabi
    res = _hipabi.QuantileResult.from_buffer_copy(result.cpu().numpy().tobytes())
    return {name: dict(n_scored=int(getattr(res, name).n_scored), rank=[int(r) for r in getattr(res, name).rank],
                       value=[int(v) for v in getattr(res, name).value]) for name in qref.REGIONS}


def _check(got, want, n_q):
    for name in qref.REGIONS:
        g, w = got[name], want[name]
        assert g["n_scored"] == w["n_scored"], (name, g, w)
        assert g["rank"][:n_q] == w["rank"] and g["rank"][n_q:] == [0] * (8 - n_q), (name, g, w)
        assert g["value"][:n_q] == w["value"] and g["value"][n_q:] == [0] * (8 - n_q), \
            (name, [hex(v) for v in g["value"]], [hex(v) for v in w["value"]])


def _run(disp, gt, mask, ppm, **kw):
    import stereo_device as sd
    return sd.evaluate_quantiles(_dev(disp), _dev(gt), _dev(mask), ppm, **kw)


def _run_and_check(disp, gt, mask, ppm):
    want = qref.quantiles(disp, gt, mask, ppm)
    _check(_got(_run(disp, gt, mask, ppm)), want, len(ppm))
    return want


def _from_keys(k, shape):
    """Maps whose errors are exactly the given keys: gt = 0, disp = the float of the key."""
    disp = np.asarray(k, np.uint32).view(np.float32).reshape(shape)
    return disp, np.zeros(shape, np.float32), None


@pytest.mark.parametrize("H,W,with_mask", SHAPES, ids=["%dx%d" % s[:2] for s in SHAPES])
def test_quantiles_equal_the_restatement(H, W, with_mask):
    import torch
    import stereo_device as sd
    disp, gt, mask = qref.make_case(H, W, seed=1000 * H + W, with_mask=with_mask)
    want = qref.quantiles(disp, gt, mask, Q8)
    out = torch.full((26,), -1, dtype=torch.int64, device="cuda")           # 0xFF bytes: every byte is overwritten
    sd.evaluate_quantiles(_dev(disp), _dev(gt), _dev(mask), Q8, out=out)
    _check(_got(out), want, 8)
    _run_and_check(disp, gt, mask, A4)                                       # entries past n_q: rank 0, value +0.0
    if H * W >= 1000 and with_mask:
        assert 0 < want["nonocc"]["n_scored"] < want["all"]["n_scored"]


@pytest.fixture(scope="module")
def large_case():
    """500 x 750, the size of a Middlebury quarter-resolution pair: 367 workgroups; reference computed once."""
    disp, gt, mask = qref.make_case(500, 750, seed=77, d_max=200.0)
    return disp, gt, mask, qref.quantiles(disp, gt, mask, Q8)


def test_large_map_with_eight_unordered_quantiles(large_case):
    disp, gt, mask, want = large_case
    _check(_got(_run(disp, gt, mask, Q8)), want, 8)
    v = want["all"]["value"]
    assert v[1] == v[3]                                                      # the repeated quantile
    shared = [x for x in set(v) if x >> 24 == v[2] >> 24]
    assert len(shared) >= 3 and len(set(x >> 16 for x in shared)) >= 3       # one first-pass bin, different later bins
    assert v[5] == int(np.sort(qref.keys(disp, gt, mask)["all"])[0]) and v[6] == int(qref.keys(disp, gt, mask)["all"].max())


def test_all_errors_equal():
    gt = np.random.default_rng(0).uniform(1, 50, (37, 53)).astype(np.float32)
    gt = (np.round(gt * 4) / 4).astype(np.float32)
    disp = (gt + np.float32(0.75)).astype(np.float32)
    want = _run_and_check(disp, gt, None, Q8)
    assert set(want["all"]["value"]) == {qref.bits_of(0.75)} and want["all"]["n_scored"] == 37 * 53


def test_consecutive_floats_differ_in_the_last_digit_only():
    k = np.uint32(0x3f9a5c00) + np.random.default_rng(1).permutation(256).astype(np.uint32)
    want = _run_and_check(*_from_keys(k, (8, 32)), Q8)
    assert want["all"]["value"][1] == 0x3f9a5c7f and want["all"]["value"][6] == 0x3f9a5cff


def test_errors_differ_in_the_top_digit_only():
    k = (np.random.default_rng(2).permutation(128).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00123456)
    want = _run_and_check(*_from_keys(k, (4, 32)), Q8)
    assert want["all"]["value"][5] == 0x00123456 and want["all"]["value"][6] == 0x7f123456


@pytest.mark.parametrize("form", ["gt_inf", "invalid", "mask"])
def test_zero_scored_pixels(form):
    disp, gt, mask = qref.make_case(9, 31, seed=3)
    if form == "gt_inf":
        gt[:] = np.inf
    elif form == "invalid":
        disp[:] = -1.0
        disp[::2] = np.nan
        gt = np.where(np.isfinite(gt), gt, np.float32(1)).astype(np.float32)
    else:
        mask = np.where(mask == 255, np.uint8(254), mask).astype(np.uint8)
    want = _run_and_check(disp, gt, mask, A4)
    assert want["nonocc"] == dict(n_scored=0, rank=[0] * 4, value=[qref.NAN_BITS] * 4)
    assert (want["all"]["n_scored"] > 0) == (form == "mask")


def test_exactly_one_scored_pixel():
    gt = np.full((5, 41), np.inf, np.float32)
    disp = np.full((5, 41), 7.0, np.float32)
    mask = np.full((5, 41), 255, np.uint8)
    gt[3, 17], disp[3, 17] = 4.0, 6.5
    want = _run_and_check(disp, gt, mask, Q8)
    assert want["all"] == dict(n_scored=1, rank=[0] * 8, value=[qref.bits_of(2.5)] * 8)


def test_zero_subnormal_and_overflowing_errors():
    disp = np.array([[-0.0, 1e-40, 3e38, 2.0]], np.float32)
    gt = np.array([[0.0, 0.0, -3e38, 1.0]], np.float32)
    ppm = (1, 500000, 750000, 1000000)
    want = _run_and_check(disp, gt, None, ppm)
    assert want["all"]["value"] == [0, qref.bits_of(1e-40), qref.bits_of(1.0), 0x7f800000]
    assert 0 < want["all"]["value"][1] < 0x00800000                          # a subnormal, kept


def test_one_scratch_twice_and_result_does_not_depend_on_the_pool():
    import torch
    import stereo_device as sd
    a, b = qref.make_case(37, 53, seed=10), qref.make_case(64, 96, seed=11, with_mask=False)
    scratch = sd.evaluate_quantiles_scratch(64, 96, torch.device("cuda"))
    pool = sd.evaluate_quantiles_pool(torch.device("cuda"))
    ra = sd.evaluate_quantiles(_dev(a[0]), _dev(a[1]), _dev(a[2]), Q8, scratch=scratch)
    rb = sd.evaluate_quantiles(_dev(b[0]), _dev(b[1]), _dev(b[2]), A4, scratch=scratch)
    ra_pool = sd.evaluate_quantiles(_dev(a[0]), _dev(a[1]), _dev(a[2]), Q8, pool=pool, scratch=scratch)
    _check(_got(ra), qref.quantiles(*a, Q8), 8)
    _check(_got(rb), qref.quantiles(*b, A4), 4)
    assert ra.cpu().numpy().tobytes() == ra_pool.cpu().numpy().tobytes()
    assert np.array_equal(pool.cpu().numpy().astype(np.uint64), qref.Pool().add(*a).counts)


def test_pool_accumulates_and_the_pooled_pick():
    import torch
    import stereo_device as sd
    dev = torch.device("cuda")
    pool, model = sd.evaluate_quantiles_pool(dev), qref.Pool()
    assert pool.numel() * pool.element_size() == 2 * 65536 * 8
    _check(_got(sd.evaluate_quantiles_pooled(pool, Q8)), model.pick(Q8), 8)  # zeroed pool: NaN, rank 0
    assert model.pick(A4)["all"]["value"] == [qref.NAN_BITS] * 4
    for seed, (H, W, with_mask) in enumerate([(37, 53, True), (1, 1025, True), (64, 96, False)]):
        case = qref.make_case(H, W, seed=20 + seed, with_mask=with_mask)
        assert sd.evaluate_quantiles(_dev(case[0]), _dev(case[1]), _dev(case[2]), A4, out=False, pool=pool) is None
        model.add(*case)
        before = pool.clone()                    # no pool given: not a byte of the pool may move
        sd.evaluate_quantiles(_dev(case[0]), _dev(case[1]), _dev(case[2]), A4)
        assert torch.equal(pool, before)
    assert np.array_equal(pool.cpu().numpy().astype(np.uint64), model.counts)
    _check(_got(sd.evaluate_quantiles_pooled(pool, Q8)), model.pick(Q8), 8)
    _check(_got(sd.evaluate_quantiles_pooled(pool, A4)), model.pick(A4), 4)


def test_graph_capture_and_replay():
    import torch
    import stereo_device as sd
    a, b = qref.make_case(37, 53, seed=30), qref.make_case(37, 53, seed=31)
    disp, gt, mask = _dev(a[0]), _dev(a[1]), _dev(a[2])
    out = sd.evaluate_quantiles_result(disp.device)
    scratch = sd.evaluate_quantiles_scratch(37, 53, disp.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sd.evaluate_quantiles(disp, gt, mask, Q8, out=out, scratch=scratch)        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sd.evaluate_quantiles(disp, gt, mask, Q8, out=out, scratch=scratch)
    disp.copy_(_dev(b[0]))
    gt.copy_(_dev(b[1]))
    mask.copy_(_dev(b[2]))
    out.fill_(-1)
    graph.replay()
    first = out.cpu().numpy().tobytes()
    _check(_got(out), qref.quantiles(*b, Q8), 8)
    out.fill_(-1)
    graph.replay()
    assert out.cpu().numpy().tobytes() == first


def test_evaluator_scores_commits_and_reports():
    import torch
    import evaluation as ev
    cases = [qref.make_case(37, 53, seed=40), qref.make_case(64, 96, seed=41, with_mask=False),
             qref.make_case(37, 53, seed=42)]
    ppm = ev.parse_quantiles("50,90,95,99.5")
    evaluator = ev.Evaluator(thresholds=(1.0,), slots=2, quantiles=ppm)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    scores, keep = [], []
    for i, case in enumerate(cases):
        dev = tuple(_dev(x) for x in case)
        keep.append(dev)
        streams[i % 2].wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(streams[i % 2]):
            scores.append(evaluator.score(*dev, slot=i % 2))
            evaluator.commit(*dev)
        if i == 0:
            scores[0].metrics()                  # slot 0 is reused by the third pair: its bytes are on the host first
    model = qref.Pool()
    tags = [ev.quantile_tag(q) for q in ppm]
    assert tags == ["A50", "A90", "A95", "A99.5"]
    for case, score in zip(cases, scores):
        m, want = score.metrics(), qref.quantiles(*case, ppm)
        model.add(*case)
        for r in qref.REGIONS:
            assert m.raw[r]["n_scored"] == want[r]["n_scored"] and m.raw[r]["quantile_rank"] == want[r]["rank"]
            assert [qref.bits_of(m.figures[r]["quantiles"][t]) for t in tags] == want[r]["value"]
    pooled, want = evaluator.report(), model.pick(ppm)
    assert pooled.to_dict()["quantile_bits"] == 16 and evaluator.describe() == dict(quantiles=[50.0, 90.0, 95.0, 99.5])
    for r in qref.REGIONS:
        assert pooled.raw[r]["n_scored"] == want[r]["n_scored"] and pooled.raw[r]["quantile_rank"] == want[r]["rank"]
        assert [qref.bits_of(pooled.figures[r]["quantiles"][t]) for t in tags] == want[r]["value"]
    # without quantiles: not one key more
    plain = ev.Evaluator(thresholds=(1.0,))
    d = plain.pair(*keep[0]).metrics().to_dict()
    assert sorted(d) == ["all", "nonocc", "raw"] and "quantiles" not in d["all"] and "n_scored" not in d["raw"]["all"]
    assert not hasattr(plain, "pool") and plain.describe() == {}


def test_error_quantiles_on_numpy_input_and_kitti_refusal():
    import evaluation as ev
    disp, gt, mask = qref.make_case(37, 53, seed=50)
    got = ev.error_quantiles(disp, gt, mask)
    want = qref.quantiles(disp, gt, mask, A4)
    for r in qref.REGIONS:
        assert got[r]["n_scored"] == want[r]["n_scored"] and got[r]["quantile_rank"] == want[r]["rank"]
        assert [qref.bits_of(got[r]["quantiles"][t]) for t in ("A50", "A90", "A95", "A99")] == want[r]["value"]
    got = ev.error_quantiles(disp, np.full_like(gt, np.inf), None, quantiles=(99.5,))
    assert got["all"] == dict(n_scored=0, quantile_rank=[0], quantiles={"A99.5": None})
    with pytest.raises(ValueError, match="quantiles"):
        ev.KittiEvaluator(quantiles=(500000,))
