"""GPU: the schedule that match.py, bench.py and StereoMatcher run by default, against the CPU oracle.

Every other whole-pair oracle comparison passes `keep=` to the matcher, which switches the default schedule off (the
SGM flag planes built once per pair on the side stream, the free-running one-volume chains, the fused WTA that leaves
the right volume unstored).  Here the matcher is built with nothing but `hp`, runs through match() and through the
replayed hipGraph (match_graph), and its final map must equal, bit for bit, the oracle chain fed the GPU's own conv
features (oracle.match_from_features: the split-operand features are deterministic, and every stage after them is
bit-exact).  When a map differs, the pair is run again with keep={} and the failure names the first stage that differs.
"""
import collections

import numpy as np
import pytest
import torch

from helpers import assert_bits_strict, bits_strict, first_differing_stage, stagewise

pytestmark = pytest.mark.gpu

Case = collections.namedtuple("Case", "L R D hp l r fl fr want")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def env(net_layers):
    import _hipabi as hip
    hip.require_device()
    import oracle
    import stereo_device
    from model import NET
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    return dict(o=oracle, sd=stereo_device, net=net)


def _case(env, L, R, D, hp=None):
    """The oracle's final map from the GPU's own features (computed once, shared by match() and match_graph())."""
    l, r = dev(L[:, :, 0]), dev(R[:, :, 0])
    fl, fr = (t.cpu().numpy() for t in env["net"].features_pair_hwc_split(l, r))
    assert not env["net"].split_saturated(True)
    want = env["o"].match_from_features(L, R, fl, fr, D, args=hp)
    return Case(L, R, D, hp, l, r, fl, fr, want)


def _matcher(env, hp=None, **kw):
    """The default matcher; kw: what does not touch the schedule (on_saturation)."""
    m = env["sd"].StereoMatcher(env["net"], hp=hp, **kw) if hp else env["sd"].StereoMatcher(env["net"], **kw)
    assert m.features == "split_f16" and m.pixel_major()
    assert m.free_chains and m.two_chains and m.sgm_flags_once and m.skip_unit_regions and m.refresh_first
    return m


def _arm(m, case):
    """The workspace of the case's shape, its SGM flag planes filled with a NaN sentinel (every byte 0xff)."""
    H, W = case.l.shape
    ws = m.workspace(H, W, case.D)
    assert ws["progs"] is not None, "the program-driven aggregation does not serve %dx%dx%d" % (W, H, case.D)
    for buf in ws["sgm_flags"]:
        buf.fill_(0xff)
    return ws


def _check_flags(env, m, ws, case, what):
    """The default schedule built the flag planes (the sentinel is gone) and built them from (left, right) with the
    matcher's threshold: byte for byte the planes of sgm_flag_planes on the same images."""
    torch.cuda.synchronize()
    want = [torch.full_like(b, 0xff) for b in ws["sgm_flags"]]
    env["sd"].sgm_flag_planes(case.l, case.r, case.D, m.hp["sgm_D"], out=want)
    torch.cuda.synchronize()
    for i, (got, w) in enumerate(zip(ws["sgm_flags"], want)):
        assert not bool((got == 0xff).all()), "%s: flag plane %d still holds the sentinel (the flag path did not run)" % (
            what, i)
        assert torch.equal(got, w), "%s: flag plane %d is not the plane of (left, right) at sgm_D" % (what, i)


def _check_map(env, m, case, got, what):
    got = got.cpu().numpy()
    if bits_strict(got, case.want):
        return
    keep = {}
    m.match(case.l, case.r, case.D, keep=keep)
    d = stagewise(keep, case.L, case.R, case.D, env["o"], hp=m.hp, features=(case.fl, case.fr))
    stage = first_differing_stage(d)
    where = ("first stage that differs from the oracle under keep=: %s" % stage if stage else
             "under keep= every stage equals the oracle: the difference lives in the default schedule's wiring")
    assert_bits_strict(got, case.want, "%s (%s; %s)" % (what, where, d))


def _run(env, m, case, what):
    """match(), the first match_graph() (warm-up + capture + replay) and a pure replay: each map against the oracle, the
    flag planes checked after match() and after the pure replay."""
    ws = _arm(m, case)
    _check_map(env, m, case, m.match(case.l, case.r, case.D), what + ", match()")
    _check_flags(env, m, ws, case, what + ", match()")
    _check_map(env, m, case, m.match_graph(case.l, case.r, case.D).clone(), what + ", match_graph()")
    ws = _arm(m, case)
    _check_map(env, m, case, m.match_graph(case.l, case.r, case.D).clone(), what + ", match_graph() replay")
    _check_flags(env, m, ws, case, what + ", match_graph() replay")
    return ws


def _unit_t(sup):
    """The support words' unit mask on the device: the pixels whose support region is the pixel itself."""
    return (sup & 0xfffff) == 0


def _unit(words):
    return (words.cpu().numpy().view(np.uint32).reshape(-1)[:words.shape[0] * words.shape[1]].reshape(words.shape)
            & 0xfffff) == 0


# ---------------------------------------------------------------------------------------------------------------------
# (a) shapes: H > 2*14+1 (full vertical arms inside the image), W no multiple of the patch width 20, W >= D + 2
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,D,pitch,fused", [
    (72, 301, 256, 256, True),      # cfg2's range: v4, one chunk, WTA fused into the last launch
    (56, 283, 250, 252, True),      # v4 with a padded pitch: the idle lane
    (64, 263, 192, 192, True),      # cfg3's range: v3, fused WTA
    (60, 233, 190, 192, True),      # v3 with a padded pitch
    (40, 451, 400, 400, False),     # cfg4's range: v4, two chunks, WTA as its own launch
    (45, 173, 128, 128, True),      # v2
])
def test_default_schedule_shapes(env, H, W, D, pitch, fused):
    sd = env["sd"]
    assert sd.hwd_pitch(D) == pitch and (D <= sd.cbca_hwd_wta_max_d()) == fused
    import synthetic
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=H + D)
    case = _case(env, L, R, D)
    _run(env, _matcher(env), case, "%dx%dx%d" % (W, H, D))


# ---------------------------------------------------------------------------------------------------------------------
# (b) scene classes at D = 256
# ---------------------------------------------------------------------------------------------------------------------
def _shifted_pair(scene_u8, W, shift):
    """Left view = the first W columns, right view = the scene `shift` columns on: every disparity equals `shift`."""
    import synthetic
    return synthetic.standardize(scene_u8[:, :W]), synthetic.standardize(scene_u8[:, shift:shift + W])


def _scene(kind, H, W, D):
    import synthetic
    rng = np.random.default_rng(11)
    sw = W + 24
    if kind in ("natural", "flat"):
        L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=21, kind=kind)
        return L, R
    if kind == "noise":
        # 64 random levels 4 apart, offset by 2 on a checkerboard: 4-neighbours differ by >= 2 grey levels, above the
        # arm threshold (0.02 standard deviations ~ 1.5 grey levels): every support region is the pixel itself
        i, j = np.indices((H, sw))
        scene = (4 * rng.integers(0, 64, (H, sw)) + 2 * ((i + j) % 2)).astype(np.uint8)
    else:
        # four vertical grey bands (not one: a constant image has no standard deviation)
        edges = np.sort(rng.choice(np.arange(40, sw - 40), 3, replace=False))
        scene = np.zeros((H, sw), np.uint8)
        for k, level in enumerate((40, 110, 170, 230)):
            lo = 0 if k == 0 else edges[k - 1]
            scene[:, lo:] = level
    return _shifted_pair(scene, W, 24)


@pytest.mark.parametrize("kind,H,W", [("natural", 72, 301), ("flat", 40, 301), ("noise", 72, 301), ("bands", 32, 261)])
def test_default_schedule_scene_classes(env, kind, H, W):
    """(The images whose regions are maximal are kept small: the oracle's time grows with the region size.)"""
    D = 256
    o = env["o"]
    L, R = _scene(kind, H, W, D)
    case = _case(env, L, R, D)
    m = _matcher(env)
    ws = _run(env, m, case, "%s %dx%dx%d" % (kind, W, H, D))
    share = []
    for img, sup in ((L, ws["sup_l"]), (R, ws["sup_r"])):
        # the support words' unit mask (what the skip kernels and the program builder read) is the oracle's fixed points
        unit = _unit(sup)
        want = o.cross_arms(img, m.hp["cbca_intensity"], m.hp["cbca_distance"])[1] == 1
        assert np.array_equal(unit, want), "%s: %d pixels where the unit mask differs from the oracle's" % (
            kind, int((unit != want).sum()))
        share.append(float(want.mean()))
    for s in share:
        if kind == "noise":
            assert s == 1.0, share
        elif kind == "bands":
            assert s < 0.01, share
        elif kind == "natural":
            assert s > 0.5, share
        else:
            assert s < 0.5, share


# ---------------------------------------------------------------------------------------------------------------------
# (c) iteration counts at D = 256: every branch of skip_schedule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", [(1, 1), (3, 2), (4, 3), (2, 15), (2, 16)])
def test_default_schedule_iteration_counts(env, n1, n2):
    """n1 = 1: no refresh, one full launch; odd n1: full then skips; even n1: refresh first; n2 = 1: the second
    aggregation is the WTA-carrying launch alone; n2 = 15 / 16: odd and even skip tails in front of it."""
    import synthetic
    H, W, D = 40, 283, 256
    hp = dict(cbca_num_iterations1=n1, cbca_num_iterations2=n2)
    kinds = env["sd"].skip_schedule(n1, False)
    assert kinds[0] == ("refresh" if n1 % 2 == 0 else "full")
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=n1 * 10 + n2)
    case = _case(env, L, R, D, hp)
    m = _matcher(env, hp)
    assert (m.hp["cbca_num_iterations1"], m.hp["cbca_num_iterations2"]) == (n1, n2)
    _run(env, m, case, "%d + %d iterations" % (n1, n2))


# ---------------------------------------------------------------------------------------------------------------------
# (d) state between pairs
# ---------------------------------------------------------------------------------------------------------------------
def test_default_schedule_state_between_pairs(env):
    """One matcher through match_graph: pair A, pair B (same shape, other content and other fixed points), shape C
    (workspace and graphs reset), A again - with a second matcher interleaved on the same device (the library's support
    and program registries are process-wide).  Every map equals its own oracle result."""
    import synthetic
    H, W, D = 36, 261, 256
    A = _case(env, *synthetic.make_pair(H, W, D, seed=1)[:2], D)
    B = _case(env, *synthetic.make_pair(H, W, D, seed=2, kind="natural")[:2], D)
    C = _case(env, *synthetic.make_pair(32, 171, 128, seed=3)[:2], 128)
    sup_a = env["sd"].cross_arms(A.l, 0.02, 14)
    sup_b = env["sd"].cross_arms(B.l, 0.02, 14)
    assert not torch.equal(_unit_t(sup_a), _unit_t(sup_b))
    m, m2 = _matcher(env), _matcher(env)
    steps = [(m, A, "A"), (m2, B, "B (second matcher)"), (m, B, "B after A"), (m2, A, "A (second matcher) after B"),
             (m, C, "C: new shape"), (m2, C, "C (second matcher)"), (m, A, "A again after C"),
             (m2, B, "B (second matcher) after C")]
    for i, (mm, case, what) in enumerate(steps):
        ws = _arm(mm, case)
        got = mm.match_graph(case.l, case.r, case.D).clone()
        _check_map(env, mm, case, got, "step %d, %s" % (i, what))
        _check_flags(env, mm, ws, case, "step %d, %s" % (i, what))
