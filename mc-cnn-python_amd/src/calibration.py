"""What a pair's disparities mean in space: the pinhole intrinsics of the left view, the baseline and the offset of the
principal points - Middlebury 2014's calib.txt, Z = baseline * f / (d + doffs), Z in the unit of `baseline` (mm there).
Imports neither torch nor the GPU library (match.py parses it before the GPU is pinned).  util.parseCalib still reads
the size and ndisp lines: it mirrors the reference."""
import collections
import math
import re

import numpy as np


def _f32(x):
    return float(np.float32(x))


class Calibration(collections.namedtuple("Calibration", "fx fy cx cy baseline doffs", defaults=(0.0,))):
    __slots__ = ()

    def __new__(cls, fx, fy, cx, cy, baseline, doffs=0.0):
        values = tuple(float(v) for v in (fx, fy, cx, cy, baseline, doffs))
        for name, v in zip(cls._fields, values):
            if not math.isfinite(v):
                raise ValueError("Calibration: %s=%r is not finite" % (name, v))
        for name, v in zip(("fx", "fy", "baseline"), (values[0], values[1], values[4])):
            if not v > 0:
                raise ValueError("Calibration: %s=%r, expected a value > 0" % (name, v))
        return super().__new__(cls, *values)

    @classmethod
    def from_middlebury(cls, path):
        """calib.txt read by key, in any line order: cam0=[fx 0 cx; 0 fy cy; 0 0 1], baseline=, doffs= (0 when absent)."""
        keys = {}
        with open(path, "r") as f:
            for line in f:
                k, sep, v = line.partition("=")
                if sep:
                    keys[k.strip()] = v.strip()
        for need in ("cam0", "baseline"):
            if need not in keys:
                raise ValueError("%s: no %s= line" % (path, need))
        try:
            m = [float(t) for t in re.split(r"[\s;,]+", keys["cam0"].strip("[] \t")) if t]
            if len(m) != 9:
                raise ValueError("%d numbers" % len(m))
            return cls(m[0], m[4], m[2], m[5], float(keys["baseline"]), float(keys.get("doffs", 0.0)))
        except ValueError as e:
            raise ValueError("%s: cam0 / baseline / doffs do not parse (%s)" % (path, e))

    @classmethod
    def parse(cls, text):
        """The command-line form "fx,fy,cx,cy,baseline[,doffs]"; a Calibration passes through, and a sequence of the five
        or six numbers is taken as the same list."""
        if isinstance(text, cls):
            return text
        items = list(text) if isinstance(text, (tuple, list)) else [t.strip() for t in str(text).split(",")]
        if len(items) not in (5, 6):
            raise ValueError("expected fx,fy,cx,cy,baseline[,doffs], got %r" % (text,))
        try:
            return cls(*[float(t) for t in items])
        except ValueError as e:
            raise ValueError("expected fx,fy,cx,cy,baseline[,doffs], got %r (%s)" % (text, e))

    def describe(self):
        """The text parse() reads back to the same record."""
        return ",".join(repr(v) for v in self)

    def scalars(self):
        """(fx, fy, cx, cy, fb, doffs) as the kernels take them (include/mccnn.h): float32 values, each rounded once from
        float64 - fb from the float64 product fx * baseline."""
        return (_f32(self.fx), _f32(self.fy), _f32(self.cx), _f32(self.cy), _f32(self.fx * self.baseline), _f32(self.doffs))


def write_ply(path, records, intensity):
    """A cloud as binary little-endian PLY: x y z float32 and intensity uchar per vertex, in the records' order.
    records: [n,4] float32 as the device wrote them (the fourth word is not written); intensity: n values 0 .. 255."""
    records = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 4)
    n = records.shape[0]
    vertex = np.empty(n, dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "u1")]))
    vertex["x"], vertex["y"], vertex["z"] = records[:, 0], records[:, 1], records[:, 2]
    vertex["intensity"] = np.asarray(intensity, dtype=np.uint8).reshape(n)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
              "property float z\nproperty uchar intensity\nend_header\n" % n)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(vertex.tobytes())


def read_ply(path):
    """What write_ply wrote: (xyz float32 [n,3], intensity uint8 [n])."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("%s: not a binary little-endian PLY" % path)
    n = int([ln for ln in lines if ln.startswith("element vertex ")][0].split()[2])
    vertex = np.frombuffer(data[end:], dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "u1")]))
    if vertex.shape[0] != n:
        raise ValueError("%s: %d vertices announced, %d present" % (path, n, vertex.shape[0]))
    return np.stack([vertex["x"], vertex["y"], vertex["z"]], axis=1), vertex["intensity"].copy()


def point_pixels(records):
    """The uint32 pixel indices h * W + w of [n,4] float32 records (their fourth word's bits)."""
    return np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 4)[:, 3].copy().view(np.uint32)
