"""GPU: StereoMatcher(semi_dense=...).  The returned sparse map equals the restatement (tests/semi_dense_reference.py)
applied to the returned map, the status plane a `keep=` run hands out and the returned planes, bit for bit; the dense map
and the planes have the bits of a matcher without the option; the four match entries agree; `semi_out=` is honoured."""
import numpy as np
import pytest
import torch

import semi_dense_reference as ref

pytestmark = pytest.mark.gpu

LEFT, BOTH = (64, 96, 24), (40, 48, 16)         # (H, W, D)
RULE, RULE_CONF = "lr,speckle:20:1", "lr,mmn:0.5,lrc:-1,speckle:6:0.5"


@pytest.fixture(scope="module")
def sd():
    import _hipabi
    _hipabi.require_device()
    import stereo_device
    return stereo_device


@pytest.fixture(scope="module")
def net(net_layers):
    from model import NET
    return NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def u32(t):
    return np.ascontiguousarray(host(t) if torch.is_tensor(t) else t).view(np.uint32)


def same(a, b, what):
    assert np.array_equal(u32(a), u32(b)), what


_PAIRS = {}


def pair(shape, seed=0):
    import synthetic
    key = shape + (seed,)
    if key not in _PAIRS:
        H, W, D = shape
        L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=200 + seed)
        _PAIRS[key] = (dev(L[:, :, 0].copy()), dev(R[:, :, 0].copy()))
    return _PAIRS[key]


@pytest.mark.parametrize("rule,confidence", [(RULE, ()), (RULE_CONF, ref.NAMES), ("lr", ()), ("mmn:1.5", ("mmn",))],
                         ids=["lr_speckle", "with_planes", "lr_alone", "mmn_alone"])
def test_left_view_against_the_restatement(sd, net, rule, confidence):
    H, W, D = LEFT
    l, r = pair(LEFT)
    plain = sd.StereoMatcher(net, confidence=confidence)
    want = plain.match(l, r, D)
    want_map, want_planes = want if confidence else (want, None)
    m = sd.StereoMatcher(net, confidence=confidence, semi_dense=rule)
    parsed = sd.SemiDenseRule.parse(rule)
    assert m.semi_dense == parsed
    keep = {}
    res = m.match(l, r, D, keep=keep)
    assert len(res) == (3 if confidence else 2)
    same(res[0], want_map, "the dense map of the keep= run")
    if confidence:
        same(res[1], want_planes, "the planes of the keep= run")
    planes = host(res[1]) if confidence else None
    sparse = ref.semi_dense(host(res[0]), parsed, host(keep["status"]), planes, m.confidence)
    same(res[-1], sparse, "the sparse map of the keep= run")
    assert keep["semi_dense"] is res[-1]
    kept = ref.valid(sparse)
    assert 0 < kept.sum() < ref.valid(host(res[0])).sum(), "the rule neither keeps nor drops everything"
    if parsed.speckle:
        selected = ref.select(host(res[0]), host(keep["status"]), planes, m.confidence, parsed.thresholds, parsed.require_match)
        same(keep["semi_dense_selected"], selected, "keep: the selection")
        same(keep["component_sizes"], ref.component_sizes(selected, parsed.speckle[1]), "keep: the sizes")
    else:
        assert "component_sizes" not in keep
    # the eager entry: copies of the workspace's tensors, the same bits
    res = m.match(l, r, D)
    same(res[0], want_map, "map")
    same(res[-1], sparse, "sparse")
    assert res[-1].data_ptr() != m._ws[(H, W, D)]["sparse"].data_ptr() and tuple(res[-1].shape) == (H, W)
    if confidence:
        same(res[1], want_planes, "planes")
    # semi_out=
    out = torch.full((H, W), -7.0, device="cuda")
    sout = torch.full((H, W), -7.0, device="cuda")
    res = m.match(l, r, D, out=out, semi_out=sout)
    assert res[0] is out and res[-1] is sout
    same(out, want_map, "out=")
    same(sout, sparse, "semi_out=")
    for bad in (torch.zeros((H, W + 1), device="cuda"), torch.zeros((1, H, W), device="cuda"),
                torch.zeros((H, W), dtype=torch.float64, device="cuda")):
        with pytest.raises(ValueError):
            m.match(l, r, D, semi_out=bad)
    # match_graph: the static buffers, replayed on another pair and back
    static = None
    graphed = sd.StereoMatcher(net, confidence=confidence, semi_dense=rule)
    for seed in (0, 1, 0):
        gl, gr = pair(LEFT, seed)
        g = graphed.match_graph(gl, gr, D)
        e = m.match(gl, gr, D)
        assert len(g) == len(e)
        for a, b in zip(g, e):
            same(a, b, "match_graph pair %d" % seed)
        static = static or g[-1].data_ptr()
        assert static == g[-1].data_ptr()
    assert not np.array_equal(u32(m.match(*pair(LEFT, 1), D)[-1]), u32(sparse))


def test_both_views_and_byte_entries(sd, net, golden_cases):
    H, W, D = BOTH
    g = dict(golden_cases)["ref_40x48x16_s0.npz"]
    lu, ru = dev(g["left_u8"]), dev(g["right_u8"])
    plain = sd.StereoMatcher(net, confidence=("mmn", "lrc"), views="both")
    want_map, want_planes = plain.match_u8(lu, ru, D)
    m = sd.StereoMatcher(net, confidence=("mmn", "lrc"), views="both", semi_dense=RULE_CONF)
    rule = m.semi_dense
    emap, eplanes, esparse = m.match_u8(lu, ru, D)
    same(emap, want_map, "both views: the dense maps")
    same(eplanes, want_planes, "both views: the planes")
    assert tuple(esparse.shape) == (2, H, W)
    # the status planes come from a keep= run on the images match_u8 standardised
    sl, sr, _ = m._ingest_buffers(H, W)
    keep = {}
    kmap, kplanes, ksparse = m.match(sl.clone(), sr.clone(), D, keep=keep)
    same(kmap, emap, "keep= run: maps")
    same(ksparse, esparse, "keep= run: sparse")
    for i, suffix in enumerate(("", "_right")):
        want = ref.semi_dense(host(emap[i]), rule, host(keep["status" + suffix]), host(eplanes[i]), m.confidence)
        same(esparse[i], want, "view %d against the restatement" % i)
        assert 0 < ref.valid(want).sum() < H * W
        same(keep["semi_dense" + suffix], want, "keep: semi_dense" + suffix)
        selected = ref.select(host(emap[i]), host(keep["status" + suffix]), host(eplanes[i]), m.confidence, rule.thresholds, True)
        same(keep["component_sizes" + suffix], ref.component_sizes(selected, rule.speckle[1]), "keep: sizes" + suffix)
    sout = torch.full((2, H, W), -7.0, device="cuda")
    res = m.match_u8(lu, ru, D, semi_out=sout)
    assert res[-1] is sout
    same(sout, esparse, "semi_out= with both views")
    with pytest.raises(ValueError):
        m.match_u8(lu, ru, D, semi_out=torch.zeros((H, W), device="cuda"))
    graphed = sd.StereoMatcher(net, confidence=("mmn", "lrc"), views="both", semi_dense=RULE_CONF)
    for _ in range(2):
        res = graphed.match_graph_u8(lu, ru, D)
        for a, b, what in zip(res, (emap, eplanes, esparse), ("maps", "planes", "sparse")):
            same(a, b, "match_graph_u8: " + what)


def test_option_and_workspace(sd, net):
    H, W, D = BOTH
    with pytest.raises(ValueError, match="mmn"):
        sd.StereoMatcher(net, semi_dense="lr,mmn:0.5")
    with pytest.raises(ValueError, match="lrc"):
        sd.StereoMatcher(net, confidence=("mmn",), semi_dense="mmn:0.5,lrc:-1")
    with pytest.raises(ValueError):
        sd.StereoMatcher(net, semi_dense="")
    plain = sd.StereoMatcher(net)
    assert plain.semi_dense is None
    l, r = pair(BOTH)
    assert torch.is_tensor(plain.match(l, r, D)) and "sparse" not in plain._ws[(H, W, D)]
    scratch = int(__import__("_hipabi").load().mccnn_speckle_scratch_bytes(H, W))
    assert scratch == 2 * H * W * 4
    for views in ("left", "both"):
        base = sd.workspace_bytes(H, W, D, views=views)
        assert sd.workspace_bytes(H, W, D, views=views, semi_dense=False) == base
        per_view = 3 * H * W * 4 + scratch
        assert sd.workspace_bytes(H, W, D, views=views, semi_dense=True) == base + (2 if views == "both" else 1) * per_view
        m = sd.StereoMatcher(net, views=views, semi_dense=RULE)
        ws = m.workspace(H, W, D)
        held = sum(t.numel() * t.element_size() for k in ("sparse", "semi_selected", "semi_sizes") for t in [ws[k]])
        held += sum(t.numel() * t.element_size() for t in ws["semi_scratch"])
        assert held == (2 if views == "both" else 1) * per_view


def test_process_functional(sd):
    import process_functional as pf
    assert "semi_dense" in pf.__all__ and "speckle_filter" in pf.__all__
    disp = ref.random_map(33, 70, seed=9)
    status = (np.random.default_rng(1).random(disp.shape) < 0.3).astype(np.int32)
    plane = np.random.default_rng(2).normal(size=disp.shape).astype(np.float32)
    out, sizes = pf.speckle_filter(disp, 4, 1.0, return_sizes=True)
    want_sizes = ref.component_sizes(disp, 1.0)
    assert sizes.dtype == np.uint32 and np.array_equal(sizes, want_sizes)
    same(out, ref.speckle_filter(disp, 4, 1.0, sizes=want_sizes)[0], "pf.speckle_filter")
    same(pf.speckle_filter(disp, 4), out, "max_diff defaults to 1")
    rule = sd.SemiDenseRule.parse("lr,cur:0.25,speckle:3:1")
    want = ref.semi_dense(disp, rule, status, plane[None], ("cur",))
    same(pf.semi_dense(disp, "lr,cur:0.25,speckle:3:1", status, {"cur": plane}), want, "pf.semi_dense, planes as a dict")
    same(pf.semi_dense(disp, rule, status, plane[None], ("cur",)), want, "pf.semi_dense, planes as an array")
    assert torch.is_tensor(pf.semi_dense(dev(disp), "speckle:2"))
