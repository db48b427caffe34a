"""CPU: the quantile definition restated twice (tests/quantiles_reference.py: NumPy vs a per-pixel loop) and against
np.quantile(method="inverted_cdf"), the rank formula at its edges, the truncated-pool identity, the parsing of
--eval_quantiles, the ABI's structs and header text, and every refusal of the two entry points (each is returned before
any HIP call, so the built library answers on a machine without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

import quantiles_reference as qref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mccnn.h")
PPM = (1, 333333, 500000, 900000, 950000, 990000, 999999, 1000000)


@pytest.mark.parametrize("H,W,seed,with_mask", [(1, 1, 0, True), (3, 7, 1, True), (5, 9, 2, False), (8, 16, 3, True)])
def test_restatement_equals_the_pixel_loop(H, W, seed, with_mask):
    disp, gt, mask = qref.make_case(H, W, seed, with_mask=with_mask)
    got = qref.quantiles(disp, gt, mask, PPM)
    assert qref.same(got, qref.loop(disp, gt, mask, PPM)), got
    if with_mask and H * W > 50:
        assert got["nonocc"]["n_scored"] < got["all"]["n_scored"]


@pytest.mark.parametrize("n", [1, 2, 3, 7, 1023, 1024, 1025, 1961])
def test_rank_rule_is_numpys_inverted_cdf(n):
    rng = np.random.default_rng(n)
    err = np.abs(rng.normal(0, 2, n)).astype(np.float32)
    gt = np.full(n, 5.0, np.float32)
    disp = (gt + err).astype(np.float32)
    e = np.abs(disp - gt)
    got = qref.quantiles(disp, gt, None, PPM)["all"]
    assert got["n_scored"] == n
    for q, bits in zip(PPM, got["value"]):
        want = np.quantile(e, q / 1e6, method="inverted_cdf")
        assert bits == qref.bits_of(want), (n, q)


def test_rank_edges():
    assert qref.rank_of(500000, 1) == 0 and qref.rank_of(1, 1) == 0 and qref.rank_of(1000000, 1) == 0
    for n in (1, 2, 999, 1000, 375000, 1000000, 2 ** 32 - 1):
        assert qref.rank_of(1, n) == (0 if n <= 1000000 else 4294)   # up to 10^6 pixels: the ceiling of at most one, minus one
        assert qref.rank_of(1000000, n) == n - 1
    # n * q an exact multiple of 10^6: the ceiling is the quotient itself
    assert qref.rank_of(500000, 4) == 1 and qref.rank_of(900000, 10) == 8 and qref.rank_of(250000, 8) == 1
    assert qref.rank_of(500000, 5) == 2 and qref.rank_of(900001, 10) == 9
    assert qref.rank_of(990000, 0) == 0
    assert qref.select(np.zeros(0, np.uint32), (500000,)) == dict(n_scored=0, rank=[0], value=[qref.NAN_BITS])


def test_truncated_pool_identity():
    """Truncation to the top 16 bits is monotone: the pooled pick is the top 16 bits of the exact pooled order statistic."""
    pool, every = qref.Pool(), {name: [] for name in qref.REGIONS}
    for seed, (H, W) in enumerate([(9, 13), (31, 17), (64, 5)]):
        disp, gt, mask = qref.make_case(H, W, 40 + seed)
        pool.add(disp, gt, mask)
        for name, k in qref.keys(disp, gt, mask).items():
            every[name].append(k)
    pick = pool.pick(PPM)
    for name in qref.REGIONS:
        exact = qref.select(np.sort(np.concatenate(every[name])), PPM)
        assert pick[name]["n_scored"] == exact["n_scored"] and pick[name]["rank"] == exact["rank"]
        assert pick[name]["value"] == [(v >> 16) << 16 for v in exact["value"]]
    empty = qref.Pool().pick((500000, 990000))
    assert empty["all"] == dict(n_scored=0, rank=[0, 0], value=[qref.NAN_BITS] * 2)


def test_parse_quantiles_and_tags():
    import evaluation as ev
    assert ev.parse_quantiles("50,90,95,99.5") == (500000, 900000, 950000, 995000)
    assert ev.parse_quantiles(" 99 , 50,50 ") == (990000, 500000, 500000)
    assert ev.parse_quantiles("0.0001,100,33.3333") == (1, 1000000, 333333)
    assert ev.parse_quantiles("1,2,3,4,5,6,7,8") == tuple(k * 10000 for k in range(1, 9))
    assert [ev.quantile_tag(q) for q in (500000, 995000, 1, 1000000, 333333)] == ["A50", "A99.5", "A0.0001", "A100", "A33.3333"]
    with pytest.raises(ValueError, match="1 to 8"):
        ev.parse_quantiles("1,2,3,4,5,6,7,8,9")
    with pytest.raises(ValueError, match="1 to 8"):
        ev.parse_quantiles("")
    for bad in ("0", "101", "-5", "nan", "inf", "100.0001"):
        with pytest.raises(ValueError, match="0 < q <= 100"):
            ev.parse_quantiles(bad)
    with pytest.raises(ValueError, match="four decimals"):
        ev.parse_quantiles("99.99999")
    with pytest.raises(ValueError, match="not a number"):
        ev.parse_quantiles("50,abc")


def test_structs_version_and_header():
    import _hipabi
    assert ctypes.sizeof(_hipabi.QuantileRegion) == 104 and ctypes.sizeof(_hipabi.QuantileResult) == 208
    assert _hipabi.MCCNN_ABI_VERSION == 7 and _hipabi.load().mccnn_version() == 7
    assert _hipabi.MCCNN_EVAL_POOL_BYTES == 2 * 65536 * 8 and _hipabi.MCCNN_EVAL_MAX_QUANTILES == 8
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define MCCNN_ABI_VERSION 7\b", text)
    assert "#define MCCNN_EVAL_MAX_QUANTILES 8" in text and "mccnn_quantile_region_t all, nonocc;" in text
    assert re.search(r"#define MCCNN_EVAL_POOL_BYTES \(2 \* 65536 \* 8\)", text)
    assert re.search(r"size_t\s+mccnn_evaluate_quantiles_scratch_bytes\s*\(\s*int H,\s*int W\s*\)", text)
    assert re.search(r"int\s+mccnn_evaluate_quantiles\s*\(\s*const float \*disp,\s*const float \*gt,\s*const uint8_t \*mask", text)
    assert re.search(r"int\s+mccnn_evaluate_quantiles_pooled\s*\(\s*const uint64_t \*pool", text)


def test_refusals_without_a_gpu():
    import _hipabi
    lib = _hipabi.load()
    INV, UNS, SCR = _hipabi.MCCNN_E_INVALID, _hipabi.MCCNN_E_UNSUPPORTED, _hipabi.MCCNN_E_SCRATCH
    assert lib.mccnn_evaluate_quantiles_scratch_bytes(0, 5) == 0 and lib.mccnn_evaluate_quantiles_scratch_bytes(5, -1) == 0
    need = lib.mccnn_evaluate_quantiles_scratch_bytes(4, 5)
    assert need > 0 and need % 8 == 0
    q4 = (ctypes.c_uint32 * 8)(500000, 900000, 950000, 990000, 1, 2, 3, 1000000)
    p = ctypes.c_void_p(4096)        # never dereferenced: the call is refused first
    odd = ctypes.c_void_p(4100)
    big = ctypes.c_size_t(1 << 20)

    def call(disp=p, gt=p, mask=None, H=4, W=5, q=q4, n=4, result=p, pool=None, scratch=p, nbytes=big):
        return lib.mccnn_evaluate_quantiles(disp, gt, mask, H, W, q, n, result, pool, scratch, nbytes, None)

    for kw in (dict(disp=None), dict(gt=None), dict(q=None), dict(scratch=None), dict(result=None, pool=None)):
        assert call(**kw) == INV, kw
        assert b"null pointer" in lib.mccnn_last_error_string()
    for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(n=0), dict(n=9), dict(n=-1)):
        assert call(**kw) == INV, kw
    for bad in (0, 1000001, 2 ** 32 - 1):
        assert call(q=(ctypes.c_uint32 * 2)(500000, bad), n=2) == INV and b"q_ppm[1]" in lib.mccnn_last_error_string()
    for kw in (dict(scratch=odd), dict(result=odd), dict(pool=odd), dict(result=None, pool=odd)):
        assert call(**kw) == INV, kw
        assert b"aligned" in lib.mccnn_last_error_string()
    assert call(nbytes=ctypes.c_size_t(need - 1)) == SCR and call(nbytes=ctypes.c_size_t(0)) == SCR
    assert call(H=65536, W=65536) == UNS and call(H=2 ** 31 - 1, W=2 ** 31 - 1) == UNS

    def pooled(pool=p, q=q4, n=4, result=p):
        return lib.mccnn_evaluate_quantiles_pooled(pool, q, n, result, None)

    for kw in (dict(pool=None), dict(q=None), dict(result=None)):
        assert pooled(**kw) == INV and b"null pointer" in lib.mccnn_last_error_string(), kw
    for kw in (dict(n=0), dict(n=9), dict(q=(ctypes.c_uint32 * 1)(0), n=1), dict(q=(ctypes.c_uint32 * 1)(1000001), n=1),
               dict(pool=odd), dict(result=odd)):
        assert pooled(**kw) == INV, kw


def test_metrics_without_quantiles_keep_their_keys():
    import evaluation as ev
    raw = {r: dict(n_valid=10, n_invalid=1, n_bad=[3, 2], sum_abs=4.5, sum_sq=9.0) for r in ev.REGIONS}
    d = ev.Metrics(raw, (1.0, 2.0)).to_dict()
    assert sorted(d) == ["all", "nonocc", "raw"]
    for r in ev.REGIONS:
        assert sorted(d[r]) == ["avgerr", "bad", "invalid", "rms"]
        assert sorted(d["raw"][r]) == ["n_bad", "n_invalid", "n_valid", "sum_abs", "sum_sq"]
    assert "quantiles" not in ev.mean_of([ev.Metrics(raw, (1.0, 2.0))])["all"]


def test_metrics_with_quantiles():
    import _hipabi
    import evaluation as ev
    res = _hipabi.QuantileResult()
    res.all.n_scored, res.nonocc.n_scored = 9, 0
    for k, (rank, value) in enumerate([(4, 0.5), (8, 3.25)]):
        res.all.rank[k] = rank
        res.all.value[k] = qref.bits_of(value)
        res.nonocc.value[k] = qref.NAN_BITS
    raw = {r: dict(n_valid=10, n_invalid=1, n_bad=[3], sum_abs=4.5, sum_sq=9.0) for r in ev.REGIONS}
    ppm = (500000, 995000)
    m = ev.Metrics(raw, (1.0,), ppm, ev.quantile_raw(bytes(res), ppm))
    d = m.to_dict()
    assert d["all"]["quantiles"] == {"A50": 0.5, "A99.5": 3.25} and d["nonocc"]["quantiles"] == {"A50": None, "A99.5": None}
    assert d["raw"]["all"]["n_scored"] == 9 and d["raw"]["all"]["quantile_rank"] == [4, 8] and "quantile_bits" not in d
    other = ev.Metrics({r: dict(raw[r]) for r in ev.REGIONS}, (1.0,), ppm, ev.quantile_raw(bytes(res), ppm), quantile_bits=16)
    assert other.to_dict()["quantile_bits"] == 16
    mean = ev.mean_of([m, other])
    assert mean["all"]["quantiles"] == {"A50": 0.5, "A99.5": 3.25} and mean["nonocc"]["quantiles"] == {"A50": None, "A99.5": None}
