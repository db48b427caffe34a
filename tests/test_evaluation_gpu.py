"""GPU: mccnn_evaluate against its NumPy restatement (tests/evaluation_reference.py) - counts as integers, the four sums
as uint64 bit patterns - on the shapes where the tree or the chunking can go wrong, with every special content."""
import numpy as np
import pytest

import evaluation_reference as ref

pytestmark = pytest.mark.gpu

THR = (0.5, 1.0, 2.0, 4.0)
THR8 = (0.25, 0.5, 0.75, 1.0, 2.0, 3.0, 4.0, 8.0)
# one pixel; one short of / exactly / one past a chunk; chunks straddling rows; more than one workgroup
SHAPES = [(1, 1), (1, 1023), (1, 1024), (1, 1025), (3, 341), (7, 293), (33, 97), (2, 4097)]


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(result, thresholds):
    import evaluation as ev
    return ev.Metrics.from_result(result.cpu(), thresholds).raw


def _check(got, want):
    for name in ref.REGIONS:
        g, w = got[name], want[name]
        assert (g["n_valid"], g["n_invalid"], g["n_bad"]) == (w["n_valid"], w["n_invalid"], w["n_bad"]), (name, g, w)
        for key in ("sum_abs", "sum_sq"):
            assert ref.bits(g[key]) == ref.bits(w[key]), (name, key, g[key], w[key])


def _has_every_content(disp, gt, mask):
    assert np.isposinf(gt).any() and np.isneginf(gt).any() and np.isnan(gt).any() and np.isfinite(gt).any()
    assert np.isnan(disp).any() and np.isposinf(disp).any() and np.isneginf(disp).any() and (disp == -1).any()
    assert (np.signbit(disp) & (disp == 0)).any()
    with np.errstate(invalid="ignore"):
        assert (disp > gt).any() and (disp < gt).any()
        assert any((np.abs(disp - gt) == np.float32(t)).any() for t in THR)
    if mask is not None:
        assert set(np.unique(mask)) <= {0, 1, 128, 254, 255} and (mask == 255).any() and (mask != 255).any()


@pytest.mark.parametrize("H,W", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "no_mask"])
def test_evaluate_equals_the_restatement(H, W, with_mask):
    import stereo_device as sd
    disp, gt, mask = ref.make_case(H, W, seed=1000 * H + W, with_mask=with_mask)
    if H * W >= 8:
        _has_every_content(disp, gt, mask)
    out = sd.evaluate(_dev(disp), _dev(gt), _dev(mask), THR)
    assert out.numel() * out.element_size() == 192
    _check(_raw(out, THR), ref.evaluate(disp, gt, mask, THR))


@pytest.fixture(scope="module")
def large_case():
    """2048 x 3072: 6144 chunks, the only large case; reference computed once."""
    disp, gt, mask = ref.make_case(2048, 3072, seed=77, d_max=400.0)
    return disp, gt, mask, ref.evaluate(disp, gt, mask, THR)


def test_evaluate_large_map(large_case):
    import stereo_device as sd
    disp, gt, mask, want = large_case
    _check(_raw(sd.evaluate(_dev(disp), _dev(gt), _dev(mask), THR), THR), want)


@pytest.mark.parametrize("thresholds", [(1.0,), THR, THR8], ids=["n1", "n4", "n8"])
def test_threshold_counts(thresholds):
    import evaluation as ev
    import stereo_device as sd
    disp, gt, mask = ref.make_case(33, 97, seed=5, thresholds=thresholds)
    import torch
    out = torch.full((24,), -1, dtype=torch.int64, device="cuda")           # 0xFF bytes
    sd.evaluate(_dev(disp), _dev(gt), _dev(mask), thresholds, out=out)
    _check(_raw(out, thresholds), ref.evaluate(disp, gt, mask, thresholds))
    # overwritten, every byte: the n_bad beyond n_thr are zero
    full = ev.Metrics.from_result(out.cpu(), (0,) * 8).raw
    for name in ref.REGIONS:
        assert full[name]["n_bad"][len(thresholds):] == [0] * (8 - len(thresholds))


def test_empty_regions_give_zeros_and_none():
    import evaluation as ev
    import stereo_device as sd
    import torch
    H, W = 7, 293
    disp = np.random.default_rng(0).uniform(0, 9, (H, W)).astype(np.float32)
    gt = np.full((H, W), np.inf, np.float32)
    gt[::2] = np.nan
    out = torch.full((24,), -1, dtype=torch.int64, device="cuda")
    sd.evaluate(_dev(disp), _dev(gt), None, THR, out=out)
    assert not out.cpu().numpy().any()
    m = ev.Metrics.from_result(out.cpu(), THR)
    for name in ref.REGIONS:
        f = m.figures[name]
        assert f["invalid"] is None and f["avgerr"] is None and f["rms"] is None and set(f["bad"].values()) == {None}


def test_accumulate_three_calls():
    import stereo_device as sd
    total = sd.evaluate_result("cuda")
    want = None
    for k, (H, W) in enumerate([(33, 97), (7, 293), (2, 4097)]):
        disp, gt, mask = ref.make_case(H, W, seed=40 + k, with_mask=k != 1)
        sd.evaluate(_dev(disp), _dev(gt), _dev(mask), THR, out=total, accumulate=True)
        r = ref.evaluate(disp, gt, mask, THR)
        want = r if want is None else ref.accumulate(want, r)
    _check(_raw(total, THR), want)
    # accumulating leaves the n_bad beyond n_thr alone
    import torch
    marked = torch.full((24,), 7, dtype=torch.int64, device="cuda")
    disp, gt, mask = ref.make_case(3, 341, seed=9)
    sd.evaluate(_dev(disp), _dev(gt), _dev(mask), (1.0, 2.0), out=marked, accumulate=True)
    words = marked.cpu().numpy()
    assert (words[4:10] == 7).all() and (words[12 + 4:12 + 10] == 7).all() and words[0] > 7


def test_evaluator_on_a_side_stream():
    import evaluation as ev
    import torch
    cases = [ref.make_case(33, 97, seed=60), ref.make_case(3, 341, seed=61, with_mask=False)]
    e = ev.Evaluator(thresholds=THR)
    s = torch.cuda.Stream()
    scores = []
    with torch.cuda.stream(s):
        for disp, gt, mask in cases:
            scores.append(e.pair(_dev(disp), _dev(gt), _dev(mask)))
            _check(scores[-1].metrics().raw, ref.evaluate(disp, gt, mask, THR))
    want = ref.accumulate(ref.evaluate(*cases[0], THR), ref.evaluate(*cases[1], THR))
    _check(e.report().raw, want)
    assert e.pairs == 2


def test_captured_in_a_graph_and_replayed():
    """One stream, static inputs rewritten between two replays: the eager result both times (thresholds and accumulate
    are baked in at capture)."""
    import stereo_device as sd
    import torch
    H, W = 7, 293
    cases = [ref.make_case(H, W, seed=70 + k) for k in range(3)]
    d, g, m = (_dev(a) for a in cases[0])
    out = sd.evaluate_result("cuda")
    scratch = sd.evaluate_scratch(H, W, "cuda")
    sd.evaluate(d, g, m, THR, out=out, scratch=scratch)          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sd.evaluate(d, g, m, THR, out=out, scratch=scratch)
    for disp, gt, mask in cases[1:]:
        d.copy_(_dev(disp))
        g.copy_(_dev(gt))
        m.copy_(_dev(mask))
        graph.replay()
        torch.cuda.synchronize()
        _check(_raw(out, THR), ref.evaluate(disp, gt, mask, THR))
        _check(_raw(sd.evaluate(_dev(disp), _dev(gt), _dev(mask), THR), THR), ref.evaluate(disp, gt, mask, THR))


def test_wrapper_validates_its_arguments():
    import stereo_device as sd
    import torch
    d = torch.zeros((4, 5), device="cuda")
    with pytest.raises(ValueError, match=r"\(4, 5\).*\(4, 6\)"):
        sd.evaluate(d, torch.zeros((4, 6), device="cuda"))
    with pytest.raises(ValueError):
        sd.evaluate(d, d, mask=torch.zeros((4, 5), device="cuda"))                 # float mask
    with pytest.raises(ValueError):
        sd.evaluate(d.double(), d.double())
    with pytest.raises(ValueError):
        sd.evaluate(d, d, accumulate=True)                                          # nothing to accumulate into
    with pytest.raises(ValueError):
        sd.evaluate(d, d, thresholds=())
    with pytest.raises(ValueError):
        sd.evaluate(d, d.cpu())
    with pytest.raises(sd.hip.MccnnHipError):
        sd.evaluate(d, torch.zeros((5, 4), device="cuda").t())                      # not contiguous


def test_packed_weight_cache_repacks_after_an_optimiser_step():
    """train.py --val_error keeps ONE matcher over all epochs: the net's packed-weight cache is keyed by the tensors'
    _version, so the weights an optimiser step wrote are the weights the next match packs."""
    import stereo_device as sd
    import torch
    import train
    from model import NET
    rng = np.random.default_rng(0)
    batch = [rng.standard_normal((16, 11, 11, 1)).astype(np.float32) for _ in range(3)]
    net = NET(None, batch_size=16, device="cuda", seed=3)
    t = train.Trainer(net, 0.05, 0.9, 0.2)
    before = net._split_weights()
    assert net._split_weights() is before                   # unchanged weights: the cache serves
    snapshot = [(p.clone(), s) for p, s in before]
    t.step(*batch)
    after = net._split_weights()
    assert after is not before
    fresh = [sd.conv3x3_split_pack(w) for w in net.weights[1:]]
    for (p, s), (fp, fs), (op, _os) in zip(after, fresh, snapshot):
        assert s == fs and torch.equal(p, fp)
    assert any(not torch.equal(p, op) for (p, _s), (op, _o) in zip(after, snapshot))
