"""The pileup model of tests/test_gpu_pileup.py against expectations worked out
by hand, so that the yardstick the GPU tests compare with is itself pinned on
the CPU; and the new command-line flags."""

import numpy as np
import pytest

import test_gpu_coverage as TC
import test_gpu_pileup as TP

A, C, G, T = 0, 1, 2, 3


def rows(counts):
    return [c.tolist() for c in counts]


def test_model_forward_substitution_and_base_quality():
    # AACCGGTT, k = 3: ACC is at 1, CCG at 2; the read ACCGCTT (the genome's 1..7 with C for the G
    # at 5) puts both on diagonal 1, and none of its other windows is indexed.
    genomes = ["AACCGGTT", "TTTT"]
    args = (genomes, False, 3, ["ACCGCTT"], ["IIII!II"], [TC.UNIQUE], [0, 1], [0])
    counts, stats = TP.pile(*args)
    want = np.zeros((8, 4), dtype=np.uint32)
    for x, b in ((1, A), (2, C), (3, C), (4, G), (5, C), (6, T), (7, T)):
        want[x, b] = 1
    assert rows(counts) == [want.tolist(), [[0] * 4] * 4]
    assert stats == {"reads_piled": 1, "reads_skipped": 0, "bases_counted": 7}
    assert TP.call(genomes, counts, 1, 1, 0) == [(0, 5, G, C, 1, 1, (0, 1, 0, 0))]
    assert TP.call(genomes, counts, 2, 1, 0) == []
    # '!' is 33: counted at a threshold of 33 (strict <), not at 34
    assert TP.pile(*args, min_base_quality=33)[1]["bases_counted"] == 7
    counts, stats = TP.pile(*args, min_base_quality=34)
    want[5, C] = 0
    assert rows(counts)[0] == want.tolist() and stats["bases_counted"] == 6


def test_model_inconsistent_and_other_types():
    # ACGTTACG, k = 3: ACG first at 0, TAC at 4.  TACG votes 4 - 0 and 0 - 1: two diagonals, skipped.
    # An ambiguous read (listed twice, a p-demoted G*) and an unmapped one add nothing.
    genomes = ["ACGTTACG"]
    counts, stats = TP.pile(genomes, False, 3, ["TACG", "ACGT", "GGGG"], ["IIII"] * 3,
                            [TC.UNIQUE, TC.AMBIGUOUS, 1], [0, 1, 3, 3], [0, 0, 0])
    assert not counts[0].any()
    assert stats == {"reads_piled": 0, "reads_skipped": 1, "bases_counted": 0}


def test_model_both_strands():
    # AAC is held as AACNGTT, k = 2: AA 0, AC 1, GT 4, TT 5.  GTT lies at q = 4, 5, 6 -> x = 2, 1, 0
    # with its bases complemented: C, A, A.  ACAGT votes AC: 1 - 0 and GT: 4 - 3, so s = 1:
    # A at x = 1, C at x = 2, the base on the N dropped, G -> C at x = 2, T -> A at x = 1.
    # The read with an N and a '.' keeps one window (AC) and loses those two bases.
    genomes = ["AAC", ""]
    counts, stats = TP.pile(genomes, True, 2, ["GTT", "ACAGT", "G", "AAC", "NAC."], ["III", "IIIII", "I", "III", "IIII"],
                            [TC.UNIQUE, TC.UNIQUE, 1, TC.UNIQUE, TC.UNIQUE], [0, 1, 2, 2, 3, 4], [0, 0, 0, 0])
    assert rows(counts) == [[[2, 0, 0, 0], [5, 0, 0, 0], [0, 5, 0, 0]], []]
    assert stats == {"reads_piled": 4, "reads_skipped": 0, "bases_counted": 3 + 4 + 3 + 2}
    assert TP.call(genomes, counts, 1, 1, 0) == []


def test_model_calls():
    genomes = ["ACGN", "G", ""]
    counts = [np.array([[3, 1, 0, 0], [0, 2, 2, 0], [0, 0, 5, 0], [1, 1, 1, 1]], dtype=np.uint32),
              np.array([[2, 2, 1, 1]], dtype=np.uint32), np.zeros((0, 4), dtype=np.uint32)]
    assert TP.call(genomes, counts, 1, 1, 0) == [
        (0, 0, A, C, 4, 1, (3, 1, 0, 0)), (0, 1, C, G, 4, 2, (0, 2, 2, 0)),
        (1, 0, G, A, 6, 2, (2, 2, 1, 1)), (1, 0, G, C, 6, 2, (2, 2, 1, 1)), (1, 0, G, T, 6, 1, (2, 2, 1, 1))]
    # 1000 * 2 >= 500 * 4 holds with equality; 501 per mille misses
    assert TP.call(genomes, counts, 4, 2, 500) == [(0, 1, C, G, 4, 2, (0, 2, 2, 0))]
    assert TP.call(genomes, counts, 4, 2, 501) == []
    assert TP.call(genomes, counts, 5, 2, 0) == [(1, 0, G, A, 6, 2, (2, 2, 1, 1)), (1, 0, G, C, 6, 2, (2, 2, 1, 1))]


@pytest.mark.parametrize("both", [False, True], ids=["forward", "both_strands"])
@pytest.mark.parametrize("k", [5, 7])
def test_hand_case_model_equals_hand_written(k, both):
    """The hand-built case of the GPU test: the model (types from the CPU oracle)
    gives the counts written down by hand."""
    genomes, reads, expected, _ = TP.hand_case(k)
    exp, piled = expected(both)
    _, (counts, stats) = TP.hand_model(k, both)
    assert rows(counts) == rows(exp)
    assert stats == {"reads_piled": piled, "reads_skipped": 1, "bases_counted": int(sum(int(e.sum()) for e in exp))}


def test_permille_conversion():
    from kmer import variant_permille
    assert [variant_permille(f) for f in (0, 0.2, 0.0004, 0.0005001, 0.5, 1, 1.0)] == [0, 200, 0, 1, 500, 1000, 1000]
    for bad in (-0.1, 1.01, "0.2", True, None):
        with pytest.raises(ValueError):
            variant_permille(bad)


def test_parse_arguments_accepts_variant_flags():
    import main
    base = ["-t", "dumpalign", "-g", "x.fa", "-k", "21", "--reads", "r.fq"]
    a = main.parse_arguments(base + ["--variants", "v.tsv", "--variant-min-depth", "6", "--variant-min-count", "3",
                                     "--variant-min-fraction", "0.25", "--variant-min-base-quality", "53"])
    assert (a.variants, a.variant_min_depth, a.variant_min_count, a.variant_min_fraction,
            a.variant_min_base_quality) == ("v.tsv", 6, 3, 0.25, 53)
    b = main.parse_arguments(base)
    assert (b.variants, b.variant_min_depth, b.variant_min_count, b.variant_min_fraction,
            b.variant_min_base_quality) == (None, None, None, None, None)
    assert main._has_variants_flag(["--variants=v.tsv"]) and main._has_variants_flag(["--variant-min-d", "3"])
    assert not main._has_variants_flag(base)
    assert main._early_reads_path(base) == "r.fq" and main._early_reads_path(base + ["--variants", "v"]) is None


def test_existing_abbreviations_keep_their_meaning():
    import main
    a = main.parse_arguments(["-t", "dumpalign", "--min-c", "3", "--min-r", "4", "--min-k", "5", "--max", "6", "--cov",
                              "--assign", "a.tsv"])
    assert (a.min_coverage, a.min_read_quality, a.min_kmer_quality, a.max_genomes, a.coverage, a.assignments) == \
        (3, 4, 5, 6, True, "a.tsv")
