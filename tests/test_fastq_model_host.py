"""CPU checks behind tests/test_gpu_fastq_grammar.py: the model of the
device-parsed subset (fastq_cases.in_device_subset) against the regex grammar
(records.FASTAQRecordContainer._parse_regex, the reference's), and the
properties of the generated files that the GPU tests rely on -- the shares of
accepted and rejected fuzz files, the bytes the boundary sweep puts at a window
edge, where the late violations sit, and that every byte of a record shows in
the summary."""

import numpy as np
import pytest

import fastq_cases as C
import pa_oracle as O

W = C.WINDOW


def _regex(data):
    try:
        return C.regex_outcome(data)
    except UnicodeDecodeError:
        return "UnicodeDecodeError"


def test_model_never_accepts_what_the_regex_parses_differently():
    """tests/test_host.py's 3000 random and mutated FASTQ texts: whenever the
    model accepts, the regex grammar accepts with identical (id, seq, qual)."""
    from test_host import _mutate, _random_fastq
    rng = np.random.Generator(np.random.PCG64(124))
    accepted = 0
    for it in range(3000):
        base = _random_fastq(rng)
        if it % 7 == 3:
            base = base.rstrip("\n")
        if it % 11 == 5:
            base = base + base
        text = base if it % 3 == 0 else _mutate(rng, base)
        data = text.encode("utf-8")
        got = C.in_device_subset(data)
        if got is None:
            continue
        accepted += 1
        assert got == _regex(data), repr(text)
    assert accepted > 300


def test_fuzz_shares_and_agreement():
    """The fuzz files of the GPU test (same seeds): the model agrees with the
    regex on all it accepts, accepts a quarter, rejects a quarter, and the
    rejected ones hold both kinds -- files the regex parses but the device
    subset excludes, and files on which the regex raises.  Some files' only
    fault is a one-byte "+" line that is not "+"."""
    accepted = rejected = subset_only = raises = plus_byte_only = 0
    for i in range(C.N_FUZZ):
        data = C.fuzz_case(i)
        got, want = C.in_device_subset(data), _regex(data)
        if got is not None:
            accepted += 1
            assert got == want, (i, data)
        else:
            rejected += 1
            if isinstance(want, list):
                subset_only += 1
            else:
                raises += 1
            lines = data.split(b"\n")
            mended = [b"+" if n % 4 == 2 and len(x) == 1 else x for n, x in enumerate(lines)]
            if mended != lines and C.in_device_subset(b"\n".join(mended)) is not None:
                plus_byte_only += 1
    assert 4 * accepted >= C.N_FUZZ and 4 * rejected >= C.N_FUZZ, (accepted, rejected)
    assert subset_only >= 20 and raises >= 20, (subset_only, raises)
    assert plus_byte_only >= 5, plus_byte_only


def test_sweep_covers_every_structural_position_at_the_window_edge():
    at_last, at_first = set(), set()  # what stands at W - 1 (the window's last byte) and at W
    final_lf = set()
    for pad in C.sweep_pads():
        data = C.sweep_case(pad)
        assert C.in_device_subset(data) is not None and 2 * W < len(data) < 3 * W
        at_last.add(C.structure_at(data, W - 1))
        at_first.add(C.structure_at(data, W))
        final_lf.add(data.endswith(b"\n"))
    for t in range(4):
        assert (t, True, False, False) in at_last, f"no line feed of line type {t} at offset {W - 1}"
        assert (t, True, False, False) in at_first, f"no line feed of line type {t} at offset {W}"
        assert any(s[0] == t and s[2] for s in at_first), f"no first byte of line type {t} at offset {W}"
        assert any(s[0] == t and s[3] for s in at_first), f"no last byte of line type {t} at offset {W}"
    # a record that ends exactly at W: window 0 leaves nothing to carry
    assert any(C.structure_at(C.sweep_case(p), W - 1) == (3, True, False, False)
               and C.sweep_case(p)[W:W + 1] == b"@" for p in C.sweep_pads())
    assert final_lf == {True, False}


def test_structure_at():
    data = b"@a\nAC\n+\nII\n@b\nG\n+\nI"
    assert C.structure_at(data, 0) == (0, False, True, False)
    assert C.structure_at(data, 1) == (0, False, False, True)
    assert C.structure_at(data, 2) == (0, True, False, False)
    assert C.structure_at(data, 6) == (2, False, True, True)
    assert C.structure_at(data, 10) == (3, True, False, False)
    assert C.structure_at(data, 11) == (0, False, True, False)
    assert C.structure_at(data, len(data) - 1) == (3, False, True, True)


@pytest.mark.parametrize("placement", C.PLACEMENTS)
@pytest.mark.parametrize("name", list(C.VIOLATIONS))
def test_late_violations_are_late_and_outside_the_subset(name, placement):
    clean = C.join_records(C.late_records())
    assert C.in_device_subset(clean) is not None and len(clean) > 3 * W
    data, (s, e) = C.late_case(name, placement)
    assert C.in_device_subset(data) is None
    if placement == "last_window":
        assert s >= (len(data) - 1) // W * W >= 3 * W  # the victim starts in the last window, the fourth
    else:
        assert s < W < e
    # everything before the victim is inside the subset: window 0 has been aligned by then
    assert C.in_device_subset(data[:s]) is not None
    if name == "id_repeated_from_window_0":
        assert data.count(C.late_records()[3][0] + b"\n") == 2 and data.find(C.late_records()[3][0] + b"\n") < W


def test_extreme_cases_are_inside_the_subset():
    assert all(C.in_device_subset(C.clean_case(i)) is not None for i in range(3))
    dense = C.dense_case()
    recs = C.in_device_subset(dense)
    assert recs is not None and len(recs) == 20000
    sizes = sorted({len(b"@%s\n%s\n+\n%s\n" % tuple(x.encode() for x in r)) for r in recs if len(r[1]) == 1})
    assert sizes == [9, 10, 11, 12]
    lf = np.flatnonzero(np.frombuffer(dense, dtype=np.uint8) == 10)
    per_window = np.bincount(lf // W) // 4
    assert per_window[:3].min() > 4 * 1024  # several blocks of the 1024-wide record scan in every full window
    for size, final_lf in [(2 * W, True), (2 * W, False), (3 * W, True), (3 * W, False), (2 * W + 1, True)]:
        data = C.sized_case(size, final_lf)
        assert len(data) == size and data.endswith(b"\n") == final_lf and C.in_device_subset(data) is not None
    data, at = C.threshold_case()
    quals = b"".join(data.split(b"\n")[3::4])
    assert C.in_device_subset(data) is not None and len(data) > 3 * W
    assert data[at] == C.Q - 1 and at >= (len(data) - 1) // W * W and C.structure_at(data, at)[0] == 3
    assert quals.count(bytes([C.Q - 1])) == 1 and min(quals) == C.Q - 1


NAMES = [f"g{i} sensitive genome" for i in range(C.N_GENOMES)]


def _oracle_summary(oix, names, recs, mrq=C.Q, mkq=None, elide_at=None):
    """The summary by the CPU restatement; ``elide_at``: computed as the align
    layer would with q_min = elide_at, every threshold at or below it left out."""
    seq, off = O.concat([r[1] for r in recs])
    qual, _ = O.concat([r[2] for r in recs])
    used = [None if t is not None and elide_at is not None and t <= elide_at else t for t in (mrq, mkq)]
    res = oix.align(seq, qual, off, mrq=used[0], mkq=used[1])
    return O.summary_by_walk(res, names, mrq=mrq, mkq=mkq)


def test_threshold_case_tells_a_parser_that_misses_the_byte():
    """A parser whose q_min misses the one byte Q - 1 reports Q, and the align
    layer then leaves out the thresholds at or below Q.  On the threshold file
    that changes the summary whenever min_read_quality is Q, or
    min_kmer_quality is Q and the read itself is kept: 6 of the 16 pairs.
    With the true q_min = Q - 1, leaving out thresholds changes nothing."""
    Q = C.Q
    oix = O.OracleIndex(C.genomes(), C.K)
    recs = C.regex_outcome(C.threshold_case()[0])
    telling = 0
    for mrq in (None, Q - 1, Q, Q + 1):
        for mkq in (None, Q - 1, Q, Q + 1):
            true = _oracle_summary(oix, NAMES, recs, mrq, mkq)
            assert _oracle_summary(oix, NAMES, recs, mrq, mkq, elide_at=Q - 1) == true, (mrq, mkq)
            missed = _oracle_summary(oix, NAMES, recs, mrq, mkq, elide_at=Q)
            if mrq == Q or (mkq == Q and (mrq is None or mrq < Q)):
                assert missed != true, (mrq, mkq)
                telling += 1
    assert telling == 6
    true = _oracle_summary(oix, NAMES, recs, Q, None)
    assert true["Statistics"]["filtered_quality_reads"] == 1
    assert _oracle_summary(oix, NAMES, recs, None, Q)["Statistics"]["filtered_quality_kmers"] == 1


def test_every_byte_of_the_straddling_record_shows_in_the_summary():
    """On the regex records of a sweep file, with the CPU restatement of the
    align pass: each substitution of a base of the record that straddles the
    first window boundary alters the summary, and so does each quality byte
    moved across the threshold (Q -> Q - 1 in a read whose bytes are all Q;
    + 1 in a read that holds one byte Q - 1, whose sum is then no longer below
    Q times its length).  One record of each kind is checked."""
    oix = O.OracleIndex(C.genomes(), C.K)
    names = NAMES
    seen = set()
    for pad in C.sweep_pads():
        recs_b = C.sweep_records(pad)
        j = C.straddler(recs_b) if C.structure_at(C.sweep_case(pad), W - 1) != (3, True, False, False) else None
        if j is None or len(recs_b[j][1]) != C.K:
            continue
        low = recs_b[j][3].count(bytes([C.Q - 1]))
        if low in seen:
            continue
        seen.add(low)
        recs = C.regex_outcome(C.sweep_case(pad))
        assert recs[j][1] == recs_b[j][1].decode()
        base = _oracle_summary(oix, names, recs)
        assert base["Statistics"]["filtered_quality_reads"] > 0 and base["Statistics"]["unique_mapped_reads"] > 0
        rid, seq, qual = recs[j]
        for c in range(len(seq)):
            for b in "ACGT":
                if b == seq[c]:
                    continue
                if low:  # (a dropped read's bases are not looked at: checked on the read's all-Q twin)
                    changed = recs[:j] + [(rid, seq[:c] + b + seq[c + 1:], chr(C.Q) * len(seq))] + recs[j + 1:]
                    ref = _oracle_summary(oix, names, recs[:j] + [(rid, seq, chr(C.Q) * len(seq))] + recs[j + 1:])
                else:
                    changed, ref = recs[:j] + [(rid, seq[:c] + b + seq[c + 1:], qual)] + recs[j + 1:], base
                assert _oracle_summary(oix, names, changed) != ref, (pad, c, b)
            q = chr(ord(qual[c]) + 1) if low else chr(C.Q - 1)
            changed = recs[:j] + [(rid, seq, qual[:c] + q + qual[c + 1:])] + recs[j + 1:]
            assert _oracle_summary(oix, names, changed) != base, (pad, c)
        if seen == {0, 1}:
            break
    assert seen == {0, 1}
