#!/usr/bin/env python3
"""Generates tests/golden/list_report.json: the evalMCCNN.json and eval.json texts that evaluation.ListReport writes for a
fixed scripted list.  No GPU: the Metrics come from fixed 192- and 208-byte results, the pooled totals from a stub
evaluator.

    python tests/golden/gen_list_report_golden.py

The fixture on record was written by the ListReport of the commit before the report kept one book per view;
tests/test_list_scoring_cpu.py drives the current one through scenarios() below and compares the bytes, so the files of
match.py --evaluate keep theirs - an absent key (an option that is off) included.  Only recorded results are written.
"""
import json
import os
import struct
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "list_report.json")
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
QUANTILES = (500000, 900000)


def _region(n_valid, n_invalid, n_bad, sum_abs, sum_sq):
    return struct.pack("<QQ8Qdd", n_valid, n_invalid, *(list(n_bad) + [0] * (8 - len(n_bad))), sum_abs, sum_sq)


def result_bytes(k):
    """A fixed mccnn_eval_t (192 bytes) that differs with k; k = 0: region nonocc is empty (its figures are None)."""
    nonocc = _region(0, 0, (0, 0, 0, 0), 0.0, 0.0) if k == 0 else _region(800 + k, 7 * k, (90 + k, 50, 20 + k, 3), 301.25 + k / 3.0, 977.5 * k)
    return _region(1000 + 13 * k, 11 + k, (300 + k, 200 - k, 90, 10 + k), 1234.5 / (k + 1), 5678.125 + k) + nonocc


def quantile_bytes(k):
    """A fixed mccnn_eval_quantiles_t (208 bytes); k = 0: region nonocc has no scored pixel (its quantiles are None)."""
    def region(n_scored, ranks, values):
        bits = [struct.unpack("<I", struct.pack("<f", v))[0] for v in values]
        return struct.pack("<Q8Q8I", n_scored, *(list(ranks) + [0] * 6 + bits + [0] * 6))
    nonocc = region(0, (0, 0), (0.0, 0.0)) if k == 0 else region(793 - 6 * k, (397, 714), (0.375 + k, 2.5 * k))
    return region(989 + 12 * k, (495, 890 + k), (0.25 * (k + 1), 3.0625 + k)) + nonocc


def figures(k, names=("mmn", "lrc")):
    """A pair's sparsification entry; k = 0: an empty region."""
    if k == 0:
        return dict(threshold=1.0, n=0, bad_rate=None, auc_optimal=None, auc={n: None for n in names})
    return dict(threshold=1.0, n=1000 + k, bad_rate=0.125 * k, auc_optimal=0.01 * k, auc={n: 0.05 * k + 0.001 * i for i, n in enumerate(names)})


def scenarios(ev, directory):
    """{scenario: {file name: text}} from ev.ListReport; `ev` is the evaluation module under test."""
    class StubEvaluator(object):
        def __init__(self, k, quantiles=None):
            self.thresholds, self.k, self.quantiles = THRESHOLDS, k, quantiles

        def report(self):
            if self.quantiles:
                return ev.Metrics.from_result(result_bytes(self.k), THRESHOLDS, quantile_bytes(self.k), self.quantiles,
                                              ev.POOLED_QUANTILE_BITS)
            return ev.Metrics.from_result(result_bytes(self.k), THRESHOLDS)

    class Describing(StubEvaluator):
        def describe(self):
            return dict(quantiles=[ev.quantile_percent(q) for q in self.quantiles]) if self.quantiles else dict(interpolate=True)

    def metrics(k, quantiles=None):
        if quantiles:
            return ev.Metrics.from_result(result_bytes(k), THRESHOLDS, quantile_bytes(k), quantiles)
        return ev.Metrics.from_result(result_bytes(k), THRESHOLDS)

    out = {}

    def run(scenario, report, calls):
        texts = {}
        for n, call in enumerate(calls):
            kind, index = call[0], call[1]
            if kind == "pair":
                path = os.path.join(directory, "%s_%d_%d.json" % (scenario, n, index))
                report.pair(index, "dir/pair%d/im0.png" % index, call[2], path, **call[3])
                texts["call%d_pair%d_evalMCCNN.json" % (n, index)] = open(path).read()
            else:
                getattr(report, kind)(index, "dir/pair%d/im0.png" % index)
        path = os.path.join(directory, scenario + "_eval.json")
        report.write(path)
        texts["eval.json"] = open(path).read()
        out[scenario] = texts

    # left only: pairs published out of list order, one of them with an empty region, one pair skipped
    run("left_only", ev.ListReport(StubEvaluator(5)),
        [("pair", 2, metrics(2), {}), ("skip", 3), ("pair", 0, metrics(0), {}), ("pair", 1, metrics(1), {})])
    # an evaluator that describes itself (the KITTI one), and a list on which nothing was scored
    run("described", ev.ListReport(Describing(6)), [("pair", 0, metrics(3), {})])
    run("nothing_scored", ev.ListReport(StubEvaluator(0)), [("skip", 1), ("skip", 0)])
    # --confidence: every pair with its sparsification figures, one of them of an empty region
    run("sparsification", ev.ListReport(StubEvaluator(4)),
        [("pair", 0, metrics(1), dict(sparsification=figures(1))), ("pair", 1, metrics(0), dict(sparsification=figures(0))),
         ("pair", 2, metrics(2), dict(sparsification=figures(2)))])
    # --views both: pair 0 scored on both views, pair 1 without right-view ground truth, pair 2 without any; pair 3 is
    # published twice (a repeated pair: the second entry replaces the first)
    run("both", ev.ListReport(StubEvaluator(7), StubEvaluator(8)),
        [("pair", 0, metrics(1), dict(right=dict(metrics=metrics(2), sparsification=None))),
         ("skip_right", 1), ("pair", 1, metrics(3), dict(right=None)),
         ("skip", 2), ("skip_right", 2),
         ("pair", 3, metrics(4), dict(right=dict(metrics=metrics(0), sparsification=None))),
         ("pair", 3, metrics(5), dict(right=dict(metrics=metrics(6), sparsification=None)))])
    run("both_sparsification", ev.ListReport(StubEvaluator(7), StubEvaluator(8)),
        [("pair", 0, metrics(1), dict(sparsification=figures(1), right=dict(metrics=metrics(2), sparsification=figures(3)))),
         ("skip_right", 1), ("pair", 1, metrics(3), dict(sparsification=figures(2))),
         ("pair", 2, metrics(0), dict(sparsification=figures(0), right=dict(metrics=metrics(0), sparsification=figures(0))))])
    run("both_nothing_right", ev.ListReport(StubEvaluator(2), StubEvaluator(0)),
        [("skip_right", 0), ("pair", 0, metrics(1), {}), ("skip", 1), ("skip_right", 1)])
    # --eval_quantiles: the pairs' exact quantiles, the pooled ones at 16 bits, on both views
    q = QUANTILES
    run("quantiles", ev.ListReport(Describing(3, q)),
        [("pair", 0, metrics(0, q), {}), ("pair", 1, metrics(1, q), {}), ("skip", 2)])
    run("quantiles_both", ev.ListReport(Describing(3, q), Describing(0, q)),
        [("pair", 1, metrics(2, q), dict(sparsification=figures(2), right=dict(metrics=metrics(0, q), sparsification=figures(1)))),
         ("pair", 0, metrics(1, q), dict(sparsification=figures(1), right=dict(metrics=metrics(3, q), sparsification=figures(2)))),
         ("skip_right", 2), ("pair", 2, metrics(4, q), dict(sparsification=figures(3)))])
    return out


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "mc-cnn-python_amd", "src"))
    import evaluation
    with tempfile.TemporaryDirectory() as directory:
        out = scenarios(evaluation, directory)
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d scenarios, %d bytes" % (FIXTURE, len(out), os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
