"""The coverage model of tests/test_gpu_coverage.py against expectations worked
out by hand, so that the yardstick the GPU tests compare with is itself pinned
on the CPU; and the new command-line flags."""

import test_gpu_coverage as TC


def test_model_forward_read():
    # AACCGGTT, k = 3: CCG is at 2, CGG at 3; the read CCGG puts both on diagonal 2
    genomes = ["AACCGGTT", "TTTT"]
    starts, du, da, ties, rev = TC.cover(genomes, False, 3, ["CCGG"], [TC.UNIQUE], [0, 1], [0])
    assert starts == [2] and (ties, rev) == (0, 0)
    assert [d.tolist() for d in du] == [[0, 0, 1, 1, 1, 1, 0, 0], [0, 0, 0, 0]]
    assert [d.tolist() for d in da] == [[0] * 8, [0] * 4]
    assert TC.summarize(du, genomes, 1) == ([4, 0], [4, 0], [0.5, 0.0])
    assert TC.summarize(du, genomes, 2) == ([0, 0], [4, 0], [0.5, 0.0])


def test_model_tie_overhang_and_demoted_entry():
    # ACGTTACG, k = 3: ACG first at 0 (again at 5), TAC at 4.  The read TACG votes
    # 4 - 0 = 4 and 0 - 1 = -1, once each: the smaller diagonal wins, and the
    # read hangs over the genome's start by one base.  The list holds the genome
    # twice (a p-demoted G*): two placements, one count.
    genomes = ["ACGTTACG"]
    first = TC.first_occurrences(genomes, 3)
    assert first["ACG"] == {0: 0} and first["TAC"] == {0: 4}
    assert TC.place(first, "TACG", 0, 3) == (-1, True)
    starts, du, da, ties, rev = TC.cover(genomes, False, 3, ["TACG"], [TC.AMBIGUOUS], [0, 2], [0, 0])
    assert starts == [-1, -1] and ties == 1
    assert du[0].tolist() == [0] * 8 and da[0].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]


def test_model_both_strands():
    # AAC is held as AACNGTT, k = 2: AA 0, AC 1, GT 4, TT 5.  GTT (the reverse
    # complement) lies at 4 and covers q = 4, 5, 6 -> x = 2, 1, 0.  ACAGT votes AC:
    # 1 - 0 and GT: 4 - 3, so s = 1, q = 1 .. 5: x = 1, 2, the N dropped, x = 2, 1.
    genomes = ["AAC", ""]
    assert TC.regions_of(genomes, True) == ["AACNGTT", ""]
    starts, du, da, ties, rev = TC.cover(genomes, True, 2, ["GTT", "ACAGT", "G"], [TC.UNIQUE, TC.UNIQUE, 1],
                                         [0, 1, 2, 2], [0, 0])
    assert starts == [4, 1] and rev == 1 and ties == 0
    assert du[0].tolist() == [1, 3, 3] and du[1].size == 0 and da[0].tolist() == [0, 0, 0]
    assert TC.summarize(du, genomes, 1) == ([3, 0], [7, 0], [2.3, 0.0])
    assert TC.summarize(du, genomes, 3) == ([2, 0], [7, 0], [2.3, 0.0])


def test_parse_arguments_accepts_coverage_flags():
    import main
    a = main.parse_arguments(["-t", "dumpalign", "-g", "x.fa", "-k", "21", "--reads", "r.fq", "--coverage",
                              "--genomes", "a,b,c", "--min-coverage", "3", "--full-coverage"])
    assert (a.coverage, a.genomes, a.min_coverage, a.full_coverage) == (True, "a,b,c", 3, True)
    b = main.parse_arguments(["-t", "dumpalign", "-g", "x.fa", "-k", "21", "--reads", "r.fq"])
    assert (b.coverage, b.genomes, b.min_coverage, b.full_coverage) == (False, None, None, False)
