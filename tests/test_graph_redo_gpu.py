"""GPU: the saturation redo behind a graph replay with every result present.  A matcher whose features count as saturated
repeats the pair on its library twin, which writes the STATIC map, planes and sparse map of the captured graph: what
match_graph / match_graph_u8 return is then the library matcher's result, bit for bit, in the same static tensors on every
call, in the public shape - the map alone, or the tuple (map[, planes][, sparse])."""
import numpy as np
import pytest
import torch

import semi_dense_reference as ref

pytestmark = pytest.mark.gpu

H, W, D = 40, 48, 16
CONF, RULE_CONF = ("mmn", "lrc"), "lr,mmn:0.5,lrc:-1,speckle:6:0.5"


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


def i32(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.int32)


@pytest.mark.parametrize("views,confidence,rule", [("left", CONF, RULE_CONF), ("both", CONF, RULE_CONF), ("left", (), "lr")],
                         ids=["left", "both", "left_lr_alone"])
def test_redo_behind_a_replay_writes_every_static_result(sd, net, golden_cases, views, confidence, rule):
    import synthetic
    g = dict(golden_cases)["ref_40x48x16_s0.npz"]
    options = dict(confidence=confidence, views=views, semi_dense=rule)
    floats = tuple(dev(synthetic.standardize(g[k])[:, :, 0]) for k in ("left_u8", "right_u8"))
    want = sd.StereoMatcher(net, features="miopen", **options).match(*floats, D)
    lead = (2,) if views == "both" else ()
    shapes = [lead + (H, W)] + ([lead + (len(confidence), H, W)] if confidence else []) + [lead + (H, W)]
    assert isinstance(want, tuple) and [tuple(t.shape) for t in want] == shapes
    kept = ref.valid(want[-1].cpu().numpy())
    assert kept.any() and not kept.all(), "the expected sparse map holds kept and dropped pixels"

    m = sd.StereoMatcher(net, on_saturation="fallback", **options)
    m.features_saturated = lambda reset=True: True            # every pair counts as saturated: the twin takes it
    entries = ((m.match_graph, floats), (m.match_graph_u8, (dev(g["left_u8"]), dev(g["right_u8"]))))
    for kinds, (entry, images) in enumerate(entries, 1):
        static = None
        for call in range(2):
            got = entry(*images, D)
            assert isinstance(got, tuple) and [tuple(t.shape) for t in got] == shapes
            for k, (a, b) in enumerate(zip(got, want)):
                assert np.array_equal(i32(a), i32(b)), "%s call %d: element %d" % (entry.__name__, call, k)
            static = static or [t.data_ptr() for t in got]
            assert [t.data_ptr() for t in got] == static
        assert len(m._graphs) == kinds
    assert m._library_twin is not None
