"""Genome abundance on the host: the model the GPU tests
compare the device with, pinned against closed forms; the --abundance flag
checks (main.py in a child process, no device needed); the text writer.

The model is plain Python and numpy over the genome texts: a dict from k-mer to
genome set (both strands: over g + "N" + rc(g)), the reference's decision rules
for the mapping type (src/kmer.py:394-480), the compatibility set C(r), a
Counter of classes, and the EM in float64 exactly as section 14 defines it.
Nothing from libpa feeds it.
"""

import collections
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "bioinformatics-project-for-shotgun-metagenomics-pseudo-alignment-shotgun-_amd")
MAIN = os.path.join(PKG, "main.py")
GOLD = os.path.join(REPO, "tests", "golden")
FA, FQ = os.path.join(GOLD, "config1.fa"), os.path.join(GOLD, "config1.fq")

DROPPED, UNMAPPED, UNIQUE, AMBIGUOUS = 0, 1, 2, 3
_COMP = str.maketrans("ACGTN", "TGCAN")


# ---- the model --------------------------------------------------------------------------------

def reverse_complement(s):
    return s.translate(_COMP)[::-1]


def kmer_sets(genomes, both, k):
    """{k-mer: ascending tuple of the genomes holding it}; windows with an N are not indexed."""
    d = {}
    for g, text in enumerate(genomes):
        t = text + "N" + reverse_complement(text) if both and text else text
        for j in range(len(t) - k + 1):
            w = t[j:j + k]
            if "N" not in w:
                d.setdefault(w, set()).add(g)
    return {w: tuple(sorted(s)) for w, s in d.items()}


def classify(kd, k, seq, qual, m=1, p=1, mrq=None, mkq=None, mg=None):
    """(type, C(r) as an ascending tuple, p-demoted) of one read."""
    q = [ord(c) for c in qual]
    if mrq is not None and sum(q) / len(q) < mrq:
        return DROPPED, (), False
    kmers = {}  # Read.kmers: distinct retained k-mers in window order
    for j in range(len(seq) - k + 1):
        if mkq is not None and sum(q[j:j + k]) / k < mkq:
            continue
        s = kd.get(seq[j:j + k])
        if s and not (mg is not None and len(s) > mg):
            kmers[seq[j:j + k]] = s
    if not kmers:
        return UNMAPPED, (), False
    spec, tot = {}, {}
    for s in kmers.values():
        if len(s) == 1:
            spec[s[0]] = spec.get(s[0], 0) + 1
        for g in s:
            tot[g] = tot.get(g, 0) + 1
    mx = max(tot.values())
    cand = tuple(sorted(g for g, c in tot.items() if c == mx))
    unique = None
    if len(spec) == 1:
        unique = next(iter(spec))
    elif len(spec) > 1:
        order = sorted(spec, key=spec.get, reverse=True)  # (stable: the first inserted of equal counts)
        if spec[order[0]] >= spec[order[1]] + m:
            unique = order[0]
    if unique is None:
        return AMBIGUOUS, cand, False
    if p >= 0 and mx - tot[unique] > p:
        return AMBIGUOUS, cand, True
    return UNIQUE, (unique,), False


def classify_all(kd, k, seqs, quals, **ps):
    """(types, sets, demoted flags) of a batch."""
    out = [classify(kd, k, s, q, **ps) for s, q in zip(seqs, quals)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def classes_of(sets):
    """[(C, n_C)] in reported order: lexicographic by genome list, a proper prefix first."""
    return sorted(collections.Counter(c for c in sets if c).items())


def em(classes, lengths, k, max_iterations, tolerance):
    """(theta, abundance, iterations, last delta) -- section 14, float64, the sums in the stated order."""
    G = len(lengths)
    L = np.array([n - k + 1 for n in lengths], dtype=np.float64)
    N = sum(n for _, n in classes)
    if N == 0:
        return np.zeros(G), np.zeros(G), 0, 0.0
    theta = np.full(G, 1.0 / G)

    def rho_of(th):
        return [float(th[g]) / float(L[g]) if L[g] >= 1 else 0.0 for g in range(G)]
    it, delta = 0, 0.0
    while it < max_iterations:
        rho = rho_of(theta)
        new = [0.0] * G
        for C, n in classes:
            d = 0.0
            for g in C:
                d += rho[g]
            if d == 0:
                continue
            for g in C:
                new[g] += float(n) * rho[g] / d
        new = np.array([x / float(N) for x in new])
        delta = float(np.max(np.abs(new - theta)))
        theta = new
        it += 1
        if tolerance > 0 and delta < tolerance:
            break
    rho = rho_of(theta)
    tot = 0.0
    for x in rho:
        tot += x
    ab = np.array([x / tot if tot != 0 else 0.0 for x in rho])
    return theta, ab, it, delta


def abundance_file(names, lengths, types, sets, k, iterations=200, tolerance=1e-9):
    """The --abundance file's text from the model's per-read types and sets."""
    G = len(names)
    classes = classes_of(sets)
    unique, compatible = [0] * G, [0] * G
    for t, c in zip(types, sets):
        if t == UNIQUE:
            unique[c[0]] += 1
        for g in c:
            compatible[g] += 1
    theta, ab, it, delta = em(classes, lengths, k, iterations, tolerance)
    N = sum(n for _, n in classes)
    out = ["#genome\tlength\tunique_reads\tcompatible_reads\testimated_reads\tread_fraction\tabundance\n"]
    for g in range(G):
        out.append("\t".join([names[g], str(lengths[g]), str(unique[g]), str(compatible[g]),
                              format(float(theta[g]) * N, ".9g"), format(float(theta[g]), ".9g"),
                              format(float(ab[g]), ".9g")]) + "\n")
    out.append(f"#iterations\t{it}\tlast_delta\t{format(delta, '.9g')}\tclasses\t{len(classes)}\n")
    return "".join(out)


# ---- the model against closed forms ------------------------------------------------------------

@pytest.mark.parametrize("a, b", [(5, 7), (1, 1000), (3, 0)])
def test_em_unique_evidence_takes_all(a, b):
    """{A}: a, {A, B}: b, equal lengths: with theta_A + theta_B = 1 an iteration is
    theta_B' = theta_B b / (a + b), so theta_B = (1/2) (b / (a + b))^n after n of
    them and theta_A -> 1 whenever a > 0."""
    for n in (1, 7, 200):
        theta, ab, it, delta = em([((0,), a), ((0, 1), b)], [1000, 1000], 31, n, 0)
        want = 0.5 * (b / (a + b)) ** n
        assert it == n and abs(theta[1] - want) <= 1e-12 * max(want, 1e-300) + 1e-300
        assert abs(theta.sum() - 1) < 1e-12 and np.allclose(ab, theta, atol=1e-12)
    theta, _, it, delta = em([((0,), a), ((0, 1), b)], [1000, 1000], 31, 10000, 1e-13)
    if b <= 7:  # (b / (a + b) = 0.999 takes 30 000 iterations: not run)
        assert it < 10000 and abs(theta[0] - 1) < 1e-11


@pytest.mark.parametrize("a, b, c", [(10, 30, 60), (1, 1, 0), (7, 2, 500)])
def test_em_shared_reads_follow_the_unique_ones(a, b, c):
    """{A}: a, {B}: b, {A, B}: c, equal lengths: the fixed point splits c as a : b."""
    theta, ab, it, delta = em([((0,), a), ((0, 1), c), ((1,), b)], [500, 500], 21, 10000, 1e-15)
    assert abs(theta[0] - a / (a + b)) < 1e-9 and abs(theta[1] - b / (a + b)) < 1e-9
    assert np.allclose(ab, theta, atol=1e-12)  # equal lengths: the cell share is the read share
    assert it < 10000 and delta < 1e-15


def test_em_length_normalisation_and_empty():
    # one class {A, B} only, L = 100 and 200: theta_A / theta_B doubles every iteration (the weights are
    # theta / L), and the cell share is theta / L normalised
    for n in (1, 5):
        theta, ab, it, _ = em([((0, 1), 10)], [130, 230], 31, n, 0)
        assert it == n and abs(theta[0] / theta[1] - 2.0 ** n) < 1e-9 and abs(theta.sum() - 1) < 1e-15
        assert abs(ab[0] / ab[1] - 2.0 ** (n + 1)) < 1e-9 and abs(ab.sum() - 1) < 1e-15
    theta, ab, it, delta = em([], [100, 100], 31, 50, 1e-9)
    assert theta.tolist() == [0, 0] and ab.tolist() == [0, 0] and (it, delta) == (0, 0.0)


def test_model_types_and_sets():
    """Three genomes sharing one stretch, two of them a second: the model's C(r) by hand."""
    k = 5
    a, b, c = "AACCGGTTACGTAC", "TTGGACGTACCATG", "GGATCACGTACTCA"  # all three hold ACGTAC
    kd = kmer_sets([a, b, c], False, k)
    assert kd["ACGTA"] == (0, 1, 2) and kd["CGTAC"] == (0, 1, 2)
    t, C, dem = classify(kd, k, "ACGTAC", "IIIIII")
    assert (t, C, dem) == (AMBIGUOUS, (0, 1, 2), False)   # no specific k-mer: the reference's list is empty
    t, C, dem = classify(kd, k, "AACCGG", "IIIIII")
    assert (t, C, dem) == (UNIQUE, (0,), False)
    assert classify(kd, k, "ACGT", "IIII")[0] == UNMAPPED            # shorter than k
    assert classify(kd, k, "AACCGG", "######", mrq=40)[0] == DROPPED
    assert classify(kd, k, "ACNTAC", "IIIIII")[0] == UNMAPPED        # every window holds the N
    assert classify(kd, k, "ACGTAC", "IIIIII", mg=2)[0] == UNMAPPED  # both k-mers are in three genomes
    # both strands: the reverse complement of a specific k-mer maps too
    kb = kmer_sets([a, b, c], True, k)
    assert classify(kb, k, reverse_complement("AACCGG"), "IIIIII")[:2] == (UNIQUE, (0,))
    assert classes_of([(0,), (0, 1), (0,), (), (0, 1, 2), (1,)]) == [((0,), 2), ((0, 1), 1), ((0, 1, 2), 1), ((1,), 1)]


# ---- the text writer ---------------------------------------------------------------------------

def test_abundance_text():
    from kmer import ABUNDANCE_HEADER, abundance_text
    text = abundance_text(["g one", "g2"], [1000, 2000], [3, 0], [5, 2], [0.75, 0.25], [6 / 7, 1 / 7], 7, 12,
                          1.5e-10, 3)
    assert text == (ABUNDANCE_HEADER
                    + "g one\t1000\t3\t5\t5.25\t0.75\t0.857142857\n"
                    + "g2\t2000\t0\t2\t1.75\t0.25\t0.142857143\n"
                    + "#iterations\t12\tlast_delta\t1.5e-10\tclasses\t3\n")
    assert ABUNDANCE_HEADER == ("#genome\tlength\tunique_reads\tcompatible_reads\testimated_reads\tread_fraction"
                                "\tabundance\n")
    assert abundance_text([], [], [], [], [], [], 0, 0, 0.0, 0) == ABUNDANCE_HEADER + \
        "#iterations\t0\tlast_delta\t0\tclasses\t0\n"


# ---- the flag checks ---------------------------------------------------------------------------

def test_parse_arguments_accepts_abundance_flags():
    import main
    base = ["-t", "dumpalign", "-g", "x.fa", "-k", "21", "--reads", "r.fq"]
    a = main.parse_arguments(base + ["--abundance", "a.tsv", "--abundance-iterations", "50",
                                     "--abundance-tolerance", "0"])
    assert (a.abundance, a.abundance_iterations, a.abundance_tolerance) == ("a.tsv", 50, 0.0)
    b = main.parse_arguments(base)
    assert (b.abundance, b.abundance_iterations, b.abundance_tolerance) == (None, None, None)
    assert main._has_abundance_flag(["--abundance=a.tsv"]) and main._has_abundance_flag(["--abundance-it", "3"])
    assert not main._has_abundance_flag(base)
    assert main._early_reads_path(base) == "r.fq" and main._early_reads_path(base + ["--abundance", "a"]) is None


@pytest.mark.parametrize("argv, message", [
    (["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--abundance-iterations", "5"], "need --abundance"),
    (["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--abundance-tolerance", "0.1"], "need --abundance"),
    (["-t", "dumpalign", "-a", "x.aln", "--abundance", "a.tsv"], "only allowed for task 'dumpalign' with --reads"),
    (["-t", "dumpref", "-g", FA, "-k", "21", "--abundance", "a.tsv"], "only allowed for task 'dumpalign'"),
    (["-t", "reference", "-g", FA, "-k", "21", "-r", "x.kdb", "--abundance", "a.tsv"], "only allowed for task"),
    (["-t", "align", "-g", FA, "-k", "21", "--reads", FQ, "-a", "x.aln", "-r", "x.kdb", "--abundance", "a.tsv"],
     "only allowed for task"),
    (["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--abundance", "a.tsv", "--abundance-iterations", "0"],
     "--abundance-iterations must be in 1 .. 10000"),
    (["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--abundance", "a.tsv", "--abundance-iterations",
      "10001"], "--abundance-iterations must be in 1 .. 10000"),
    (["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--abundance", "a.tsv", "--abundance-tolerance=-1"],
     "--abundance-tolerance must be at least 0"),
    (["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--abundance", "a.tsv", "--abundance-tolerance", "nan"],
     "--abundance-tolerance must be at least 0"),
    (["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--abundance", "no_such_dir/a.tsv"], "Error:"),
], ids=["iterations_alone", "tolerance_alone", "alignfile", "dumpref", "reference", "align", "iterations_0",
        "iterations_10001", "tolerance_negative", "tolerance_nan", "unwritable"])
def test_cli_abundance_misuse(argv, message, tmp_path):
    """The flag checks end the process before any device work."""
    r = subprocess.run([sys.executable, MAIN] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=60, cwd=str(tmp_path), env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode != 0 and r.stdout == ""
    err = r.stderr.strip()
    assert err.startswith("Error:") and len(err.splitlines()) == 1 and message in err
