"""The rule of a semi-dense map (include/mccnn.h has the definitions) and its text form.  Host-only: match.py parses
--semi_dense with it before the GPU is pinned; stereo_device re-exports it."""
import math

import numpy as np

MEASURES = ("msm", "mmn", "cur", "lrc")     # stereo_device.CONFIDENCE_MEASURES: the order of the planes


def _f32(x):
    return float(np.float32(x))


class SemiDenseRule(object):
    """Which pixels of a map a semi-dense map keeps: `require_match` (left-right status 0), `thresholds` ({measure: the
    float32 value its plane must reach}) and `speckle` (None or (min_size, max_diff)), applied in that order:
    sparse = speckle_filter(select(map)).  The text form is comma-separated items: `lr`, `<msm|mmn|cur|lrc>:<float>` and
    `speckle:<min_size>[:<max_diff>]` (max_diff defaults to 1.0); at least one item, none repeated.  Floats are rounded
    to float32 once, here."""

    def __init__(self, require_match=False, thresholds=None, speckle=None):
        self.require_match = bool(require_match)
        self.thresholds = {}
        for name, value in dict(thresholds or {}).items():
            if name not in MEASURES:
                raise ValueError("semi-dense rule: unknown confidence measure %r: choose from %s" % (name, ", ".join(MEASURES)))
            value = _f32(value)
            if math.isnan(value):
                raise ValueError("semi-dense rule: the threshold of %s is NaN" % name)
            self.thresholds[name] = value
        self.speckle = None
        if speckle is not None:
            min_size, max_diff = speckle
            if int(min_size) != min_size or not 1 <= int(min_size) <= 0xFFFFFFFF:
                raise ValueError("semi-dense rule: speckle min_size=%r, expected an integer >= 1" % (min_size,))
            max_diff = _f32(max_diff)
            if not max_diff >= 0.0:
                raise ValueError("semi-dense rule: speckle max_diff=%r, expected a value >= 0" % (max_diff,))
            self.speckle = (int(min_size), max_diff)
        if not (self.require_match or self.thresholds or self.speckle):
            raise ValueError("semi-dense rule: empty - name at least one of lr, <measure>:<min>, speckle:<min_size>")

    @classmethod
    def parse(cls, rule):
        """A SemiDenseRule from its text (a SemiDenseRule passes through)."""
        if isinstance(rule, cls):
            return rule
        if not isinstance(rule, str):
            raise ValueError("semi-dense rule: expected a SemiDenseRule or its text, got %r" % (rule,))
        require_match, thresholds, speckle, seen = False, {}, None, set()
        items = [item.strip() for item in rule.split(",")]
        if not any(items):
            raise ValueError("semi-dense rule: empty - name at least one of lr, <measure>:<min>, speckle:<min_size>")
        for item in items:
            head, _, rest = item.partition(":")
            if head in seen:
                raise ValueError("semi-dense rule: %r named twice" % head)
            seen.add(head)
            try:
                if head == "lr" and not rest:
                    require_match = True
                elif head == "speckle" and rest:
                    parts = rest.split(":")
                    if len(parts) > 2:
                        raise ValueError
                    speckle = (int(parts[0]), float(parts[1]) if len(parts) == 2 else 1.0)
                elif head in MEASURES and rest:
                    thresholds[head] = float(rest)
                else:
                    raise KeyError
            except KeyError:
                raise ValueError("semi-dense rule: item %r is none of lr, <%s>:<min>, speckle:<min_size>[:<max_diff>]"
                                 % (item, "|".join(MEASURES)))
            except ValueError:
                raise ValueError("semi-dense rule: item %r does not parse" % item)
        return cls(require_match, thresholds, speckle)

    @property
    def measures(self):
        """The confidence measures the rule reads, in plane order."""
        return tuple(n for n in MEASURES if n in self.thresholds)

    def describe(self):
        """The canonical text: lr, the measures in plane order, speckle; parse(describe()) is the same rule."""
        items = ["lr"] if self.require_match else []
        items += ["%s:%r" % (n, self.thresholds[n]) for n in self.measures]
        if self.speckle:
            items.append("speckle:%d:%r" % self.speckle)
        return ",".join(items)

    def __eq__(self, other):
        return isinstance(other, SemiDenseRule) and self.describe() == other.describe()

    def __hash__(self):
        return hash(self.describe())

    def __repr__(self):
        return "SemiDenseRule(%r)" % self.describe()
