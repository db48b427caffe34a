"""What one matched pair yields, stated once: the disparity map, the confidence planes (--confidence) and the sparse map
(--semi_dense); under views="both" every one of them has one more leading axis (left, right).  With geometry= (--depth,
--point_cloud) the metric outputs follow: the depth plane, the cloud's records and their number - the LEFT view's, without
a leading axis under views="both" too.  The matcher builds the record, the list loops and the scorer pass it on whole; the
fields may be device tensors, pinned host tensors, arrays or the caller's `out=` tensors - whatever travels together.
Imports neither torch nor the GPU library."""
import collections

_VIEW_FIELDS = 3        # map, planes, sparse: the fields with a leading view axis under views="both"


class PairResult(collections.namedtuple("PairResult", "map planes sparse depth points n_points",
                                        defaults=(None, None, None, None, None))):
    __slots__ = ()

    def public(self):
        """What the match entries return: the map alone when nothing else is present, else the present fields in order."""
        if all(t is None for t in self[1:]):
            return self.map
        return tuple(t for t in self if t is not None)

    @classmethod
    def decode(cls, value, planes, sparse, depth=False, points=False):
        """The inverse of public() for a matcher that produces planes / a sparse map / a depth plane / a cloud (booleans:
        its configuration; a cloud is two fields, the records and their number)."""
        if not (planes or sparse or depth or points):
            return cls(value)
        rest = iter(value[1:])
        return cls(value[0], next(rest) if planes else None, next(rest) if sparse else None,
                   next(rest) if depth else None, next(rest) if points else None, next(rest) if points else None)

    def apply(self, fn):
        """fn on every present field, in field order."""
        return PairResult(*(fn(t) if t is not None else None for t in self))

    def view(self, v, both):
        """View v (0 left, 1 right) of a both-views record; a left-only matcher's record is its only view.  The metric
        fields are the left view's: they stay with view 0 and are absent from view 1."""
        if not both:
            return self
        return PairResult(*(t[v] if t is not None else None for t in self[:_VIEW_FIELDS]),
                          *(self[_VIEW_FIELDS:] if v == 0 else ()))
