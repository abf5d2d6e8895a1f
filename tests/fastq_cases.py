"""FASTQ test files for the device parser (csrc/pa_fastq.hip) and a CPU model
of the subset it accepts.  Shared by test_fastq_model_host.py (CPU: the model
against the regex grammar, the coverage the GPU tests rely on) and
test_gpu_fastq_grammar.py (GPU: every file against the regex grammar's
outcome).  No GPU is needed to import this module.

The index is built so that every device-parsed byte shows in the summary:
k = 11, a dozen short random genomes, and reads that are mostly one k-mer of
exactly one genome, none of whose 33 one-base neighbours is in the index -- a
wrong, shifted or missing base makes the read unmapped.  Every quality byte is
Q and about half the reads hold one byte Q - 1: with min_read_quality = Q
(mean of the raw bytes < Q drops the read) one wrong quality byte moves
filtered_quality_reads.
"""

from __future__ import annotations

import io
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from test_host import POOL  # the host parser's fuzz pool: one list, so the two cannot drift apart

K = 11
Q = 60                  # raw quality byte of the threshold ('<'); Q - 1 is ';'
WINDOW = 65536          # PA_STREAM_WINDOW of the tests (the library's minimum)
N_GENOMES = 12
GENOME_LEN = 400
KW = dict(min_read_quality=Q)

Record = List[bytes]    # the four lines of a record, without line feeds


def _rng(*seed) -> np.random.Generator:
    return np.random.Generator(np.random.PCG64(list(seed)))


_GENOMES: Optional[List[bytes]] = None
_KMERS: Optional[List[bytes]] = None


def genomes() -> List[bytes]:
    global _GENOMES
    if _GENOMES is None:
        rng = _rng(7)
        _GENOMES = [bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=GENOME_LEN)])
                    for _ in range(N_GENOMES)]
    return _GENOMES


def genomes_fasta() -> str:
    return "".join(f">g{i} sensitive genome\n{g.decode()}\n" for i, g in enumerate(genomes()))


def sensitive_kmers() -> List[bytes]:
    """k-mers held by exactly one genome whose 33 one-base neighbours are all
    absent from the index: a read that is one of them is uniquely mapped, and
    any substitution in it makes it unmapped."""
    global _KMERS
    if _KMERS is None:
        owners: Dict[bytes, set] = {}
        for gi, g in enumerate(genomes()):
            for p in range(len(g) - K + 1):
                owners.setdefault(g[p:p + K], set()).add(gi)
        out = []
        for km, own in owners.items():
            if len(own) != 1:
                continue
            if any(km[:c] + bytes([b]) + km[c + 1:] in owners for c in range(K) for b in b"ACGT" if b != km[c]):
                continue
            out.append(km)
        _KMERS = out
    return _KMERS


def sensitive_records(n: int, seed: int, prefix: str = "r", long_frac: float = 0.15) -> List[Record]:
    """n records: a sensitive k-mer (or, for long_frac of them, a longer piece
    of a genome), qualities Q with one byte Q - 1 in about half of them."""
    rng = _rng(11, seed)
    kmers, gens = sensitive_kmers(), genomes()
    recs = []
    for i in range(n):
        if rng.random() < long_frac:
            g = gens[int(rng.integers(len(gens)))]
            n_b = int(rng.integers(K + 1, 25))
            s = int(rng.integers(0, len(g) - n_b + 1))
            seq = g[s:s + n_b]
        else:
            seq = kmers[int(rng.integers(len(kmers)))]
        qual = bytearray([Q]) * len(seq)
        if rng.random() < 0.5:
            qual[int(rng.integers(len(seq)))] = Q - 1
        recs.append([f"@{prefix}{i}".encode(), seq, b"+", bytes(qual)])
    return recs


def join_records(recs: Sequence[Record], final_lf: bool = True) -> bytes:
    return b"\n".join(b"\n".join(r) for r in recs) + (b"\n" if final_lf and recs else b"")


def record_spans(recs: Sequence[Record]) -> List[Tuple[int, int]]:
    """[start, end) of every record in join_records(recs), the line feed that ends it included."""
    out, at = [], 0
    for r in recs:
        n = sum(len(x) + 1 for x in r)
        out.append((at, at + n))
        at += n
    return out


def decode_text(data: bytes) -> str:
    """What open(path, "rt", encoding="utf-8").read() gives for these bytes
    (universal newlines; UnicodeDecodeError for undecodable bytes)."""
    return io.TextIOWrapper(io.BytesIO(data), encoding="utf-8").read()


# ---- the CPU model ---------------------------------------------------------------

def _graphic(c: int) -> bool:
    return 0x21 <= c <= 0x7E


def in_device_subset(data: bytes) -> Optional[List[Tuple[str, str, str]]]:
    """The subset documented at the top of csrc/pa_fastq.hip, restated: the
    (id, sequence, quality) records of a text inside it, None for any other.
    LF line ends only, exactly four lines per record from byte 0, "@" + an id
    of graphic bytes / space / tab that starts and ends with a graphic byte, a
    non-empty ACGT sequence, a line that is exactly "+", qualities of graphic
    bytes of the sequence's length, at most one final line feed, unique ids,
    at least one record.  (A record longer than a window is a separate matter:
    whether it is parsed on the device depends on where it starts.)"""
    if not data:
        return None
    lines = (data[:-1] if data.endswith(b"\n") else data).split(b"\n")
    if len(lines) % 4:
        return None
    out, seen = [], set()
    for i in range(0, len(lines), 4):
        h, s, p, q = lines[i:i + 4]
        if len(h) < 2 or h[0:1] != b"@" or not _graphic(h[1]) or not _graphic(h[-1]):
            return None
        if not all(_graphic(c) or c in (0x20, 0x09) for c in h[1:]):
            return None
        if not s or s.strip(b"ACGT") or p != b"+" or len(q) != len(s) or not all(_graphic(c) for c in q):
            return None
        rid = h[1:]
        if rid in seen:
            return None
        seen.add(rid)
        out.append((rid.decode("ascii"), s.decode("ascii"), q.decode("ascii")))
    return out


def regex_outcome(data: bytes):
    """The reference grammar's verdict on the bytes of a file: its records as
    (id, sequence, quality), or the exception's type name."""
    import records as R
    c = R.FASTAQRecordContainer()
    try:
        c._parse_regex(decode_text(data))
    except Exception as e:  # noqa: BLE001
        return type(e).__name__
    return [(r.identifier, r["sequence"], r["quality_sequence"]) for r in c]


# ---- differential fuzz -------------------------------------------------------------

# tests/test_host.py's pool (lowercase bases, N and "é" are in it), and what it lacks of the
# ways of being outside the device subset
POOL_EXT = POOL + ["\x7f", "+x"]
PLUS_BYTES = "-.x@!A"   # one-byte "+" lines that are not "+" (fuzz files i % 30 == 9)
FUZZ_SEED = 20
N_FUZZ = 300


def _mutate(rng, text: str) -> str:
    """One edit: a pool string inserted / a character deleted or replaced at a
    random place, or an edit aimed at one line type (a blank or DEL inside a
    quality line, "+x" / "+." / "-" for "+", a lowercase base or N, a blank at
    an edge of an id, "é" in an id), or CRLF line ends throughout."""
    op = int(rng.integers(0, 10))
    if not text:
        return str(rng.choice(POOL_EXT))
    i = int(rng.integers(0, len(text)))
    if op == 0:
        return text[:i] + str(rng.choice(POOL_EXT)) + text[i:]
    if op == 1:
        return text[:i] + text[i + 1:]
    if op == 2:
        return text[:i] + str(rng.choice(POOL_EXT)) + text[i + 1:]
    if op == 3:
        return text.replace("\n", "\r\n")
    lines = text.split("\n")
    n_rec = len(lines) // 4
    if n_rec == 0:
        return text + "\n"
    r = int(rng.integers(n_rec))
    h, s, p, q = lines[4 * r:4 * r + 4]
    if op == 4 and q:
        c = int(rng.integers(len(q)))
        q = q[:c] + str(rng.choice(["\x20", "\x7f"])) + q[c + 1:]
    elif op == 5:
        p = str(rng.choice(["+x", "+.", "+..", "-", "+ ", "+" + h[1:]]))
    elif op == 6 and s:
        c = int(rng.integers(len(s)))
        s = s[:c] + str(rng.choice(["N", s[c].lower(), " "])) + s[c + 1:]
    elif op == 7:
        h = str(rng.choice([h + " ", h + "\t", "@ " + h[1:], "@\t" + h[1:]]))
    elif op == 8:
        c = int(rng.integers(1, len(h) + 1))
        h = h[:c] + "é" + h[c:]
    else:
        return text + str(rng.choice(["\n", " ", "\n\n", "x\n", "\r\n"]))
    lines[4 * r:4 * r + 4] = [h, s, p, q]
    return "\n".join(lines)


def fuzz_case(i: int) -> bytes:
    """File i of the differential fuzz: one to six records with unique ids that
    mostly begin and end with a graphic byte, reads cut from the genomes, then
    zero to two edits (none in every third file); some without the final line
    feed, some with a repeated id, a few with a byte that is not UTF-8.  Every
    thirtieth file is left unedited but for one "+" line, which becomes another
    single byte: the one fault that only k_records' test of that byte catches."""
    rng = _rng(FUZZ_SEED, i)
    kmers, gens = sensitive_kmers(), genomes()
    parts = []
    for r in range(int(rng.integers(1, 7))):
        mid = "".join(rng.choice(list("ab c\t1_:"), size=int(rng.integers(0, 5))))
        rid = f"f{r}{mid}x"
        if rng.random() < 0.03:
            rid = str(rng.choice([" " + rid, rid + " ", rid + "\t"]))
        if rng.random() < 0.7:
            seq = kmers[int(rng.integers(len(kmers)))].decode()
        else:
            g = gens[int(rng.integers(len(gens)))]
            n_b = int(rng.integers(1, 41))
            s = int(rng.integers(0, len(g) - n_b + 1))
            seq = g[s:s + n_b].decode()
        if rng.random() < 0.6:
            qual = [Q] * len(seq)
            if rng.random() < 0.5:
                qual[int(rng.integers(len(seq)))] = Q - 1
        else:
            qual = [int(x) for x in rng.integers(33, 127, size=len(seq))]
        parts.append(f"@{rid}\n{seq}\n+\n{''.join(map(chr, qual))}\n")
    if i % 30 == 9:  # (its own generator: the other files do not depend on this one)
        own = _rng(FUZZ_SEED, i, 1)
        r = int(own.integers(len(parts)))
        parts[r] = parts[r].replace("\n+\n", "\n" + str(own.choice(list(PLUS_BYTES))) + "\n", 1)
    text = "".join(parts)
    if i % 7 == 3:
        text = text[:-1]
    if i % 13 == 5:
        text = text + parts[0]  # a repeated id
    for _ in range(0 if i % 3 == 0 else int(rng.integers(0, 3))):
        text = _mutate(rng, text)
    data = text.encode("utf-8")
    if i % 29 == 17:
        at = int(rng.integers(0, len(data) + 1))
        data = data[:at] + b"\xff" + data[at:]
    return data


# ---- boundary sweep -----------------------------------------------------------------

SWEEP_SEED = 31
SWEEP_BYTES = 150_000   # about 2.3 windows


def _sweep_base() -> List[Record]:
    recs = sensitive_records(6000, SWEEP_SEED)
    spans = record_spans(recs)
    n = next(i for i, (_, e) in enumerate(spans) if e >= SWEEP_BYTES)
    return recs[:n + 1]


_SWEEP: Optional[List[Record]] = None


def sweep_records(pad: int) -> List[Record]:
    """The sweep's records with the first id made `pad` bytes longer, which
    moves every later byte of the file `pad` offsets up."""
    global _SWEEP
    if _SWEEP is None:
        _SWEEP = _sweep_base()
    recs = list(_SWEEP)
    recs[0] = [recs[0][0] + b"p" * pad] + recs[0][1:]
    return recs


def sweep_pads() -> range:
    longest = max(e - s for s, e in record_spans(sweep_records(0)))
    return range(longest + 16)


def sweep_case(pad: int) -> bytes:
    return join_records(sweep_records(pad), final_lf=pad % 2 == 0)


def structure_at(data: bytes, off: int) -> Tuple[int, bool, bool, bool]:
    """What stands at byte `off` of a four-lines-per-record text: (line type
    0..3 = header / sequence / plus / quality, is the line's line feed, is the
    line's first byte, is the line's last byte before the line feed)."""
    t = data.count(b"\n", 0, off) % 4
    lf = data[off:off + 1] == b"\n"
    first = off == 0 or data[off - 1:off] == b"\n"
    last = not lf and (off + 1 == len(data) or data[off + 1:off + 2] == b"\n")
    return t, lf, first and not lf, last


def straddler(recs: Sequence[Record], off: int = WINDOW) -> int:
    """Index of the record with bytes on both sides of offset `off`."""
    for i, (s, e) in enumerate(record_spans(recs)):
        if s < off < e:
            return i
    raise ValueError(f"a record ends exactly at {off}")


# ---- late violations ---------------------------------------------------------------

LATE_SEED = 41
LATE_RECORDS = 6200     # a little over three windows


def _sub(b: bytes, c: int, x: bytes) -> bytes:
    return b[:c] + x + b[c + 1:]


# name -> (the records, the index of the victim) -> the lines that replace the victim's four
VIOLATIONS: Dict[str, Callable[[Sequence[Record], int], List[bytes]]] = {
    "lowercase_base": lambda R, j: [R[j][0], _sub(R[j][1], 4, R[j][1][4:5].lower()), R[j][2], R[j][3]],
    "base_N": lambda R, j: [R[j][0], _sub(R[j][1], 7, b"N"), R[j][2], R[j][3]],
    "blank_in_sequence": lambda R, j: [R[j][0], _sub(R[j][1], 3, b" "), R[j][2], R[j][3]],
    "quality_0x20": lambda R, j: [R[j][0], R[j][1], R[j][2], _sub(R[j][3], 5, b"\x20")],
    "quality_0x7f": lambda R, j: [R[j][0], R[j][1], R[j][2], _sub(R[j][3], 0, b"\x7f")],
    "quality_short": lambda R, j: [R[j][0], R[j][1], R[j][2], R[j][3][:-1]],
    "quality_long": lambda R, j: [R[j][0], R[j][1], R[j][2], R[j][3] + bytes([Q])],
    "plus_id": lambda R, j: [R[j][0], R[j][1], b"+" + R[j][0][1:], R[j][3]],
    "plus_other_byte": lambda R, j: [R[j][0], R[j][1], b"-", R[j][3]],
    "header_without_at": lambda R, j: [R[j][0][1:], R[j][1], R[j][2], R[j][3]],
    "header_at_alone": lambda R, j: [b"@", R[j][1], R[j][2], R[j][3]],
    "id_ends_in_space": lambda R, j: [R[j][0] + b" ", R[j][1], R[j][2], R[j][3]],
    "id_starts_with_tab": lambda R, j: [b"@\t" + R[j][0][1:], R[j][1], R[j][2], R[j][3]],
    "e_acute_in_id": lambda R, j: [R[j][0][:2] + "é".encode() + R[j][0][2:], R[j][1], R[j][2], R[j][3]],
    "cr_before_one_lf": lambda R, j: [R[j][0], R[j][1] + b"\r", R[j][2], R[j][3]],
    "lone_cr_in_id": lambda R, j: [R[j][0][:2] + b"\r" + R[j][0][2:], R[j][1], R[j][2], R[j][3]],
    "blank_line_between_records": lambda R, j: [R[j][0], R[j][1], R[j][2], R[j][3], b""],
    "fifth_garbage_line": lambda R, j: [R[j][0], R[j][1], R[j][2], R[j][3], b"garbage"],
    "id_repeated_from_window_0": lambda R, j: [R[3][0], R[j][1], R[j][2], R[j][3]],
}
PLACEMENTS = ("last_window", "first_boundary")

_LATE: Optional[List[Record]] = None


def late_records() -> List[Record]:
    global _LATE
    if _LATE is None:
        _LATE = sensitive_records(LATE_RECORDS, LATE_SEED, long_frac=0.0)
    return _LATE


def late_case(name: str, placement: str) -> Tuple[bytes, Tuple[int, int]]:
    """A file of more than three windows with one violation: in its last record
    but one (the last window; the garbage line goes after the last record and
    ends the file) or in the record that straddles offset WINDOW.  Returns the
    bytes and [start, end) of the lines that replaced the victim."""
    recs = late_records()
    if placement == "last_window":
        j = len(recs) - (1 if name == "fifth_garbage_line" else 2)
    else:
        j = straddler(recs)
    lines = VIOLATIONS[name](recs, j)
    head = join_records(recs[:j])
    data = head + b"\n".join(lines) + b"\n" + join_records(recs[j + 1:])
    return data, (len(head), len(head) + sum(len(x) + 1 for x in lines))


def clean_case(i: int) -> bytes:
    """A small file inside the subset (its ids differ from every late file's)."""
    return join_records(sensitive_records(120, 5000 + i, prefix="c"))


# ---- extremes ----------------------------------------------------------------------

def _base36(i: int) -> str:
    d = "0123456789abcdefghijklmnopqrstuvwxyz"
    s = ""
    while True:
        s = d[i % 36] + s
        i //= 36
        if not i:
            return s


def dense_case(n: int = 20000) -> bytes:
    """n records of nine to twelve bytes ("@<base36>", one base, "+", one
    quality byte Q or Q - 1): far more than 1024 records in a 64 KiB window.
    Every 23rd record is a sensitive k-mer instead, so a record offset that is
    wrong anywhere in the multi-block scan moves a genome's count."""
    rng = _rng(51)
    kmers = sensitive_kmers()
    base = rng.integers(0, 4, size=n)
    low = rng.random(n) < 0.5
    recs = []
    for i in range(n):
        if i % 23 == 22:
            seq = kmers[int(rng.integers(len(kmers)))]
            qual = bytes([Q]) * K
        else:
            seq = b"ACGT"[base[i]:base[i] + 1]
            qual = bytes([Q - 1 if low[i] else Q])
        recs.append([b"@" + _base36(3 * i).encode(), seq, b"+", qual])  # (ids of one to four bytes)
    return join_records(recs)


def sized_case(size: int, final_lf: bool, seed: int = 61) -> bytes:
    """A text inside the subset of exactly `size` bytes (the first id padded to fit)."""
    recs = sensitive_records(size // 30 + 8, seed, long_frac=0.0)
    spans = record_spans(recs)
    target = size + (0 if final_lf else 1)
    n = max(i for i, (_, e) in enumerate(spans) if e <= target - 1)
    recs = recs[:n + 1]
    pad = target - spans[n][1]
    recs[0] = [recs[0][0] + b"p" * pad] + recs[0][1:]
    data = join_records(recs, final_lf)
    assert len(data) == size
    return data


def threshold_case() -> Tuple[bytes, int]:
    """Three windows of reads whose every quality byte is Q .. Q + 3, except in
    one k-long, uniquely mapped record of the last window: its bytes are all Q
    but one, which is Q - 1.  That read alone is below min_read_quality = Q
    (its sum is Q * k - 1) and its one k-mer alone below min_kmer_quality = Q,
    so a parser whose q_min misses the byte -- it would report Q, and the
    align layer would leave out both thresholds at or below Q -- gives another
    summary.  Returns the bytes and the offset of that byte."""
    recs = [list(r) for r in sensitive_records(LATE_RECORDS, 71, prefix="t", long_frac=0.1)]
    rng = _rng(72)
    for r in recs:
        r[3] = bytes(int(x) for x in rng.integers(Q, Q + 4, size=len(r[3])))
    j = next(i for i in range(len(recs) - 40, len(recs)) if len(recs[i][1]) == K)
    recs[j][3] = _sub(bytes([Q]) * K, 6, bytes([Q - 1]))
    s, _ = record_spans(recs)[j]
    return join_records(recs), s + len(recs[j][0]) + 1 + len(recs[j][1]) + 1 + 2 + 6
