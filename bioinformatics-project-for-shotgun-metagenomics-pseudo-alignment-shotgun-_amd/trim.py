"""Read trimming: the definition in plain Python, the
command line's flags turned into trim specs, and the --trim-report text.

The device pass is pa_reads_trim (csrc/pa_trim.hip); ``trim_read`` below is
the same definition read by read, integers only, and what the tests compare
the device with.
"""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

MAX_ADAPTER = 64
DEFAULT_MIN_OVERLAP = 3
DEFAULT_ERROR_PERMILLE = 100
STAT_NAMES = ("reads", "bases_in", "bases_out", "reads_trimmed", "reads_quality", "bases_quality",
              "reads_adapter", "bases_adapter", "reads_empty")
_ACGT = frozenset(b"ACGT")


class Spec:
    """A trim spec: optional quality cutoffs (raw quality bytes), an optional
    3' adapter, the smallest overlap and the error rate in permille."""

    def __init__(self, quality3: Optional[int] = None, quality5: Optional[int] = None,
                 adapter: Optional[bytes] = None, min_overlap: int = DEFAULT_MIN_OVERLAP,
                 max_error_permille: int = DEFAULT_ERROR_PERMILLE):
        if isinstance(adapter, str):
            adapter = adapter.encode("latin-1")
        for q in (quality3, quality5):
            if q is not None and not 0 <= int(q) <= 255:
                raise ValueError("a trim quality cutoff must be between 0 and 255")
        if adapter is not None:
            if not 1 <= len(adapter) <= MAX_ADAPTER:
                raise ValueError(f"a trim adapter must hold 1 to {MAX_ADAPTER} bases")
            if not set(adapter) <= _ACGT:
                raise ValueError("a trim adapter may hold the letters A, C, G and T only")
        if int(min_overlap) < 1:
            raise ValueError("the trim overlap must be at least 1")
        if not 0 <= int(max_error_permille) <= 500:
            raise ValueError("the trim error rate must be between 0 and 0.5")
        self.quality3 = None if quality3 is None else int(quality3)
        self.quality5 = None if quality5 is None else int(quality5)
        self.adapter = adapter
        self.min_overlap = int(min_overlap)
        self.max_error_permille = int(max_error_permille)

    @property
    def active(self) -> bool:
        return self.quality3 is not None or self.quality5 is not None or self.adapter is not None

    def native(self):
        """The pa_trim_spec of this spec."""
        import pa_native as N
        return N.TrimSpec.make(self.quality3, self.quality5, self.adapter, self.min_overlap, self.max_error_permille)

    def __repr__(self) -> str:
        return (f"trim.Spec(quality3={self.quality3}, quality5={self.quality5}, adapter={self.adapter!r}, "
                f"min_overlap={self.min_overlap}, max_error_permille={self.max_error_permille})")


def quality_bounds(qual: Sequence[int], q3: Optional[int], q5: Optional[int]) -> Tuple[int, int]:
    """(start, cut) of the quality step; both scans run over the original read."""
    n = len(qual)
    cut, start = n, 0
    if q3 is not None:
        s = best = 0
        for i in range(n - 1, -1, -1):
            s += q3 - qual[i]
            if s < 0:
                break
            if s > best:
                best, cut = s, i
    if q5 is not None:
        s = best = 0
        for i in range(n):
            s += q5 - qual[i]
            if s < 0:
                break
            if s > best:
                best, start = s, i + 1
    return start, cut


def adapter_hit(read: bytes, adapter: bytes, min_overlap: int, max_error_permille: int) -> int:
    """The smallest hit p of the adapter in the read, or len(read)."""
    n = len(read)
    for p in range(n):
        ov = min(n - p, len(adapter))
        if ov < min_overlap:
            continue
        allowed = max_error_permille * ov // 1000  # (1000 * mm <= permille * ov, for integers)
        mm = 0
        for j in range(ov):
            if read[p + j] != adapter[j]:  # (a byte outside ACGT equals no adapter byte)
                mm += 1
                if mm > allowed:
                    break
        else:
            return p
    return n


def trim_read(seq: bytes, qual: bytes, spec: Spec) -> Tuple[int, int, int]:
    """(start, end, cut) of one read: it becomes seq[start:end], qual[start:end]."""
    start, cut = quality_bounds(qual, spec.quality3, spec.quality5)
    if start >= cut:
        return 0, 0, 0
    end = cut
    if spec.adapter is not None:
        end = start + adapter_hit(seq[start:cut], spec.adapter, spec.min_overlap, spec.max_error_permille)
    return start, end, cut


def new_stats() -> dict:
    return {n: 0 for n in STAT_NAMES}


def count_read(stats: dict, length: int, start: int, end: int, cut: int) -> None:
    """One read's share of the statistics (sums over reads)."""
    bases_quality = length - (cut - start)
    bases_adapter = cut - end
    stats["reads"] += 1
    stats["bases_in"] += length
    stats["bases_out"] += end - start
    stats["reads_trimmed"] += (end - start) != length
    stats["reads_quality"] += bases_quality != 0
    stats["bases_quality"] += bases_quality
    stats["reads_adapter"] += bases_adapter != 0
    stats["bases_adapter"] += bases_adapter
    stats["reads_empty"] += end == start


def trim_columns(seq: bytes, qual: bytes, off: Sequence[int], spec: Spec):
    """The model over a batch's columns: (seq, qual, off, start, end, stats) of
    the trimmed batch, off a list of len(off) offsets."""
    out_s, out_q, out_off, starts, ends = bytearray(), bytearray(), [0], [], []
    stats = new_stats()
    for r in range(len(off) - 1):
        a, b = int(off[r]), int(off[r + 1])
        s, q = bytes(seq[a:b]), bytes(qual[a:b])
        start, end, cut = trim_read(s, q, spec)
        count_read(stats, b - a, start, end, cut)
        out_s += s[start:end]
        out_q += q[start:end]
        out_off.append(len(out_s))
        starts.append(start)
        ends.append(end)
    return bytes(out_s), bytes(out_q), out_off, starts, ends, stats


def report_text(stats_list: List[dict]) -> str:
    """--trim-report: the nine names behind '#', then one line of values per
    mate file, tab-separated."""
    lines = ["#" + "\t".join(STAT_NAMES)]
    for st in stats_list:
        lines.append("\t".join(str(int(st[n])) for n in STAT_NAMES))
    return "\n".join(lines) + "\n"
