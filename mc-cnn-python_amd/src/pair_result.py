"""What one matched pair yields, stated once: the disparity map, the confidence planes (--confidence) and the sparse map
(--semi_dense); under views="both" every one of them has one more leading axis (left, right).  The matcher builds the
record, the list loops and the scorer pass it on whole; the fields may be device tensors, pinned host tensors, arrays or
the caller's `out=` tensors - whatever travels together.  Imports neither torch nor the GPU library."""
import collections


class PairResult(collections.namedtuple("PairResult", "map planes sparse", defaults=(None, None))):
    __slots__ = ()

    def public(self):
        """What the match entries return: the map alone when nothing else is present, else the present fields in order."""
        if self.planes is None and self.sparse is None:
            return self.map
        return tuple(t for t in self if t is not None)

    @classmethod
    def decode(cls, value, planes, sparse):
        """The inverse of public() for a matcher that produces planes / a sparse map (two booleans: its configuration)."""
        if not (planes or sparse):
            return cls(value)
        rest = iter(value[1:])
        return cls(value[0], next(rest) if planes else None, next(rest) if sparse else None)

    def apply(self, fn):
        """fn on every present field, in field order."""
        return PairResult(*(fn(t) if t is not None else None for t in self))

    def view(self, v, both):
        """View v (0 left, 1 right) of a both-views record; a left-only matcher's record is its only view."""
        return self.apply(lambda t: t[v]) if both else self
