"""Reader for Praat TextGrid text files, as the Montreal Forced Aligner writes them and reference eval.py:105-126 reads
them through the ``textgrid`` package: ``TextGrid.fromFile(path)``, ``grid.maxTime``, ``grid[tier]`` -> intervals with
``minTime`` / ``maxTime`` / ``mark`` / ``duration()``.

[3P-unverified]: ``textgrid`` is an un-vendored third party that is not available offline; this module restates the
part of its interface the evaluation uses from the file format (Praat manual, "TextGrid file formats") and is tested on
hand-written fixtures (tests/test_textgrid_cpu.py), not against the package.  Times are rounded to 15 decimal places
as that package does on reading.  Both the long form (``xmin = 0``) and the short form (bare values) are read.
"""
import codecs
import re

PRECISION = 15

_TOKEN = re.compile(r'"((?:[^"]|"")*)"|\[\d*\]|(<exists>|<absent>)|([-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?)', re.S)


class Interval:
    def __init__(self, minTime, maxTime, mark):
        self.minTime, self.maxTime, self.mark = minTime, maxTime, mark

    def duration(self):
        return self.maxTime - self.minTime

    def __repr__(self):
        return f"Interval({self.minTime}, {self.maxTime}, {self.mark!r})"


class Point:
    def __init__(self, time, mark):
        self.time, self.mark = time, mark


class Tier:
    """IntervalTier (items are Interval) or, with ``is_point``, a TextTier (items are Point)"""

    def __init__(self, name, minTime, maxTime, items, is_point=False):
        self.name, self.minTime, self.maxTime, self.items, self.is_point = name, minTime, maxTime, items, is_point

    intervals = property(lambda self: self.items)

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)

    def __getitem__(self, i):
        return self.items[i]


class TextGrid:
    def __init__(self, minTime=0.0, maxTime=0.0, tiers=None):
        self.minTime, self.maxTime, self.tiers = minTime, maxTime, list(tiers or [])

    def __len__(self):
        return len(self.tiers)

    def __iter__(self):
        return iter(self.tiers)

    def __getitem__(self, i):
        return self.tiers[i]

    @classmethod
    def fromFile(cls, path):
        with open(path, "rb") as f:
            raw = f.read()
        return cls.fromString(_decode(raw), str(path))

    @classmethod
    def fromString(cls, text, where="<string>"):
        head = re.match(r'\s*File type\s*=\s*"ooTextFile"\s*Object class\s*=\s*"TextGrid"', text)
        if not head:
            raise ValueError(f"{where}: not a Praat TextGrid text file")
        values = []
        for m in _TOKEN.finditer(text, head.end()):
            if m.group(1) is not None:
                values.append(m.group(1).replace('""', '"'))
            elif m.group(2) is not None:
                values.append(m.group(2) == "<exists>")
            elif m.group(3) is not None:
                values.append(round(float(m.group(3)), PRECISION))
        it = iter(values)

        def take(kind):
            try:
                v = next(it)
            except StopIteration:
                raise ValueError(f"{where}: file ends inside a tier") from None
            if kind is float and isinstance(v, float) and not isinstance(v, bool):
                return v
            if kind is int and isinstance(v, float) and v == int(v) and v >= 0:
                return int(v)
            if kind is str and isinstance(v, str):
                return v
            if kind is bool and isinstance(v, bool):
                return v
            raise ValueError(f"{where}: expected {kind.__name__}, found {v!r}")

        grid = cls(take(float), take(float))
        if not take(bool):
            return grid
        for _ in range(take(int)):
            kind, name, lo, hi = take(str), take(str), take(float), take(float)
            n = take(int)
            if kind == "IntervalTier":
                items = [Interval(take(float), take(float), take(str)) for _ in range(n)]
            elif kind == "TextTier":
                items = [Point(take(float), take(str)) for _ in range(n)]
            else:
                raise ValueError(f"{where}: unknown tier class {kind!r}")
            grid.tiers.append(Tier(name, lo, hi, items, kind == "TextTier"))
        return grid


def _decode(raw):
    if raw.startswith(codecs.BOM_UTF16_LE) or raw.startswith(codecs.BOM_UTF16_BE):
        return raw.decode("utf-16")
    if raw.startswith(codecs.BOM_UTF8):
        return raw[len(codecs.BOM_UTF8):].decode("utf-8")
    return raw.decode("utf-8")
