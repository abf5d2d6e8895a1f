"""Bootstrap confidence intervals of the abundance estimate (DESIGN.md section
16) on the host: the model the GPU tests compare the device with, pinned by its
own properties; bootstrap_summary against closed forms; the text writer; the
--abundance-bootstraps / -seed / -confidence flag checks (main.py in a child
process, no device needed); the NULL-handle answer of pa_abundance_bootstrap.

The model is section 16's definition as written: the replicate keys and the
draws in integers (Python ints in ``resample_ints``; ``resample`` is the same
with numpy uint64 and a 32-bit split for the multiply-high, so that 10^5 draws
take milliseconds), the EM test_abundance_host.em over [(C, n*_c)].  Nothing
from libpa feeds it.
"""

import bisect
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import pa_native as N
import test_abundance_host as M

MAIN, FA, FQ = M.MAIN, M.FA, M.FQ

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
COUNTS = [700, 200, 50, 0, 30, 15, 4, 1]  # (the vector section 16's definition was first checked with)


# ---- the model --------------------------------------------------------------------------------

def fmix64(x):
    x &= MASK
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & MASK
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & MASK
    x ^= x >> 33
    return x


def replicate_key(seed, b):
    return fmix64(seed + GOLDEN * (b + 1))


def resample_ints(counts, B, seed):
    """[B][classes] with Python ints, draw by draw."""
    total = sum(counts)
    cum = [0]
    for n in counts:
        cum.append(cum[-1] + n)
    rows = []
    for b in range(B):
        key, row = replicate_key(seed, b), [0] * len(counts)
        for i in range(total):
            r = (fmix64(key + GOLDEN * i) * total) >> 64
            row[bisect.bisect_right(cum, r) - 1] += 1  # the class c with cum[c] <= r < cum[c + 1]
        rows.append(row)
    return rows


def _fmix64_np(x):
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xFF51AFD7ED558CCD)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xC4CEB9FE1A85EC53)
    return x ^ (x >> np.uint64(33))


def _mulhi_np(u, n):
    """floor(u * n / 2^64) for a uint64 array u and an int n < 2^64, from four 32-bit products."""
    s, lo = np.uint64(32), np.uint64(0xFFFFFFFF)
    ul, uh = u & lo, u >> s
    nl, nh = np.uint64(n & 0xFFFFFFFF), np.uint64(n >> 32)
    ll, lh, hl, hh = ul * nl, ul * nh, uh * nl, uh * nh
    mid = (ll >> s) + (lh & lo) + (hl & lo)
    return hh + (lh >> s) + (hl >> s) + (mid >> s)


def resample(counts, B, seed):
    """[B][classes] uint64: resample_ints with numpy (uint64 arithmetic wraps mod 2^64)."""
    counts = [int(n) for n in counts]
    total = sum(counts)
    cum = np.concatenate(([0], np.cumsum(np.array(counts, dtype=np.uint64), dtype=np.uint64))).astype(np.uint64)
    out = np.zeros((B, len(counts)), dtype=np.uint64)
    if total == 0:
        return out
    with np.errstate(over="ignore"):
        steps = np.arange(total, dtype=np.uint64) * np.uint64(GOLDEN)
        for b in range(B):
            r = _mulhi_np(_fmix64_np(np.uint64(replicate_key(seed, b)) + steps), total)
            c = np.searchsorted(cum, r, side="right") - 1
            out[b] = np.bincount(c, minlength=len(counts)).astype(np.uint64)
    return out


def bootstrap(classes, lengths, k, B, seed, iterations, tolerance):
    """(counts [B][classes], theta [B][G], abundance [B][G], iterations [B], last delta [B]):
    every replicate's counts through test_abundance_host.em, with the classes' own N."""
    counts = resample([n for _, n in classes], B, seed)
    G = len(lengths)
    theta, share = np.zeros((B, G)), np.zeros((B, G))
    its, delta = np.zeros(B, dtype=np.int64), np.zeros(B)
    for b in range(B):
        theta[b], share[b], its[b], delta[b] = M.em([(C, int(n)) for (C, _), n in zip(classes, counts[b])],
                                                    lengths, k, iterations, tolerance)
    return counts, theta, share, its, delta


def summary(matrix, confidence):
    """Section 16's (mean, sd, lo, hi) per column, written out once more."""
    c = int(round(1000 * confidence))
    B = len(matrix)
    j = ((1000 - c) * B) // 2000
    out = []
    for g in range(len(matrix[0])):
        col = [float(row[g]) for row in matrix]
        mean = sum(col[1:], col[0]) / B
        sd = math.sqrt(sum((x - mean) ** 2 for x in col) / (B - 1)) if B > 1 else 0.0
        s = sorted(col)
        out.append((mean, sd, s[j], s[B - 1 - j]))
    return out


def bootstrap_file(names, lengths, types, sets, k, B, seed, confidence=0.95, iterations=200, tolerance=1e-9):
    """The --abundance file of a run with --abundance-bootstraps, from the model's per-read types and sets."""
    lines = M.abundance_file(names, lengths, types, sets, k, iterations, tolerance).splitlines()
    _, _, share, _, _ = bootstrap(M.classes_of(sets), lengths, k, B, seed, iterations, tolerance)
    stats = summary(share, confidence)
    out = [lines[0] + "\tabundance_mean\tabundance_sd\tabundance_lo\tabundance_hi"]
    out += [ln + "".join("\t" + format(x, ".9g") for x in st) for ln, st in zip(lines[1:-1], stats)]
    out.append(lines[-1] + f"\tbootstraps\t{B}\tseed\t{seed}\tconfidence\t{format(float(confidence), '.9g')}")
    return "\n".join(out) + "\n"


# ---- the model pinned -------------------------------------------------------------------------

def test_fmix64_and_multiply_high():
    assert fmix64(0) == 0 and fmix64(1) == 0xB456BCFC34C2CB2C  # MurmurHash3's finalizer
    rng = np.random.default_rng(3)
    u = rng.integers(0, 2 ** 64, 200, dtype=np.uint64)
    u[:3] = [0, 2 ** 64 - 1, 2 ** 32]
    for n in (1, 3, 999, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 12345, 2 ** 64 - 1):
        assert _mulhi_np(u, n).tolist() == [(int(x) * n) >> 64 for x in u]
    with np.errstate(over="ignore"):
        assert _fmix64_np(u).tolist() == [fmix64(int(x)) for x in u]


def test_resample_numpy_equals_ints():
    for counts, B, seed in ((COUNTS, 5, 1), ([3], 2, 0), ([1, 0, 0, 2], 4, 2 ** 63 + 5), ([0, 7, 0], 3, 2 ** 64 - 1)):
        assert resample(counts, B, seed).tolist() == resample_ints(counts, B, seed)


def test_resample_properties():
    rows = resample(COUNTS, 200, 1)
    total = sum(COUNTS)
    assert (rows.sum(axis=1) == total).all()          # every replicate holds N draws
    assert not rows[:, 3].any()                       # a class without reads is never drawn
    assert len({tuple(r) for r in rows.tolist()}) == 200
    assert resample(COUNTS, 200, 1).tolist() == rows.tolist()        # the same seed: the same counts
    other = resample(COUNTS, 2, 2)
    assert other[0].tolist() != rows[0].tolist() and other[0].tolist() != other[1].tolist()
    assert resample(COUNTS, 7, 1).tolist() == rows[:7].tolist()      # replicate b does not depend on B
    # the class means: n*_c is Binomial(N, n_c / N); the mean of 200 within 4 standard errors (1.96 at most, measured)
    worst = 0.0
    for c, n in enumerate(COUNTS):
        if n == 0:
            continue
        p = n / total
        se = math.sqrt(total * p * (1 - p) / 200)
        worst = max(worst, abs(float(rows[:, c].mean()) - n) / se)
    print(f"largest |z| of a class mean over 200 replicates: {worst:.2f}")
    assert worst <= 4


def test_resample_tiny():
    assert resample([1], 5, 9).tolist() == [[1]] * 5
    assert resample([0, 1, 0], 3, 9).tolist() == [[0, 1, 0]] * 3
    rows = resample([1, 1, 1], 50, 4)                 # N = 3
    assert (rows.sum(axis=1) == 3).all() and len({tuple(r) for r in rows.tolist()}) > 1
    assert resample([], 3, 1).shape == (3, 0) and not resample([0, 0], 2, 1).any()


def test_bootstrap_model():
    classes = [((0,), 40), ((0, 1), 30), ((1,), 10), ((1, 2), 25), ((2,), 5)]
    lengths = [500, 700, 600]
    counts, theta, share, its, delta = bootstrap(classes, lengths, 21, 6, 3, 40, 0)
    assert counts.tolist() == resample([40, 30, 10, 25, 5], 6, 3).tolist()
    assert its.tolist() == [40] * 6 and np.allclose(theta.sum(axis=1), 1, atol=1e-12)
    assert np.allclose(share.sum(axis=1), 1, atol=1e-12) and len({tuple(r) for r in theta.tolist()}) == 6
    # the replicate whose counts are the sample's own is the point estimate
    t0, s0, _, _ = M.em(classes, lengths, 21, 40, 0)
    t1, s1, _, _ = M.em([(C, n) for C, n in classes], lengths, 21, 40, 0)
    assert t0.tolist() == t1.tolist() and s0.tolist() == s1.tolist()
    _, theta, _, its, delta = bootstrap(classes, lengths, 21, 6, 3, 10000, 1e-9)
    assert (its < 10000).all() and (delta < 1e-9).all()
    empty = bootstrap([], lengths, 21, 2, 1, 10, 0)
    assert empty[0].shape == (2, 0) and not empty[1].any() and not empty[2].any() and empty[3].tolist() == [0, 0]


# ---- bootstrap_summary --------------------------------------------------------------------------

def test_bootstrap_summary_closed_forms():
    from kmer import bootstrap_summary
    assert bootstrap_summary([[0.25, 0.75]], 0.95) == [(0.25, 0.0, 0.25, 0.25), (0.75, 0.0, 0.75, 0.75)]
    m = [[1.0, 10.0], [2.0, 10.0], [3.0, 10.0], [4.0, 10.0], [5.0, 10.0]]
    got = bootstrap_summary(m[::-1], 0.95)            # (the rows' order does not matter to these)
    assert got[0] == (3.0, math.sqrt(2.5), 1.0, 5.0)  # j = (50 * 5) // 2000 = 0
    assert got[1] == (10.0, 0.0, 10.0, 10.0)
    assert bootstrap_summary(m, 0.5)[0][2:] == (2.0, 4.0)            # j = (500 * 5) // 2000 = 1
    assert bootstrap_summary(np.array(m), 0.95) == bootstrap_summary(m, 0.95) == summary(m, 0.95)
    assert bootstrap_summary(np.zeros((4, 0)), 0.9) == []


@pytest.mark.parametrize("B, confidence, j", [(20, 0.9, 1), (20, 0.95, 0), (100, 0.9, 5), (100, 0.95, 2)])
def test_bootstrap_summary_index_rule(B, confidence, j):
    """j = ((1000 - c) * B) // 2000: lo = sorted[j], hi = sorted[B - 1 - j]."""
    from kmer import bootstrap_summary
    rng = np.random.default_rng(B)
    col = rng.permutation(B).astype(np.float64)       # sorted: 0, 1, ..., B - 1
    (mean, sd, lo, hi), = bootstrap_summary(col.reshape(B, 1), confidence)
    assert (lo, hi) == (float(j), float(B - 1 - j))
    assert abs(mean - (B - 1) / 2) < 1e-12 and abs(sd - math.sqrt(B * (B + 1) / 12)) < 1e-9


@pytest.mark.parametrize("bad", [0, 1, 0.0004, 0.9996, -0.5, 1.5, float("nan"), True, "0.9", None])
def test_bootstrap_summary_refuses(bad):
    from kmer import bootstrap_summary, confidence_permille
    with pytest.raises(ValueError):
        bootstrap_summary([[0.5, 0.5]], bad)
    with pytest.raises(ValueError):
        confidence_permille(bad)


def test_confidence_permille_and_matrix_shape():
    from kmer import bootstrap_summary, confidence_permille
    assert [confidence_permille(x) for x in (0.001, 0.0006, 0.95, 0.999, 0.9994)] == [1, 1, 950, 999, 999]
    for bad in ([], [0.5, 0.5], np.zeros((0, 3))):
        with pytest.raises(ValueError):
            bootstrap_summary(bad, 0.95)


# ---- the text writer ----------------------------------------------------------------------------

def test_abundance_text_with_and_without_bootstrap():
    from kmer import ABUNDANCE_HEADER, abundance_text
    args = (["g one", "g2"], [1000, 2000], [3, 0], [5, 2], [0.75, 0.25], [6 / 7, 1 / 7], 7, 12, 1.5e-10, 3)
    plain = abundance_text(*args)
    assert plain == abundance_text(*args, None) == abundance_text(*args, bootstrap=None)
    assert plain == (ABUNDANCE_HEADER
                     + "g one\t1000\t3\t5\t5.25\t0.75\t0.857142857\n"
                     + "g2\t2000\t0\t2\t1.75\t0.25\t0.142857143\n"
                     + "#iterations\t12\tlast_delta\t1.5e-10\tclasses\t3\n")
    stats = [(0.85, 0.0125, 0.8, 0.9), (0.15, 1 / 3, 0.1, 0.2)]
    text = abundance_text(*args, (stats, 100, 2 ** 64 - 1, 0.95))
    assert text == (ABUNDANCE_HEADER[:-1] + "\tabundance_mean\tabundance_sd\tabundance_lo\tabundance_hi\n"
                    + "g one\t1000\t3\t5\t5.25\t0.75\t0.857142857\t0.85\t0.0125\t0.8\t0.9\n"
                    + "g2\t2000\t0\t2\t1.75\t0.25\t0.142857143\t0.15\t0.333333333\t0.1\t0.2\n"
                    + "#iterations\t12\tlast_delta\t1.5e-10\tclasses\t3\tbootstraps\t100\tseed\t18446744073709551615"
                      "\tconfidence\t0.95\n")


def test_text_without_bootstrap_is_the_abundance_models():
    """The writer without the new argument against test_abundance_host.abundance_file, byte for byte."""
    from kmer import abundance_text
    names, lengths, k = ["a", "b c", "d"], [500, 700, 600], 21
    types = [M.UNIQUE] * 3 + [M.AMBIGUOUS] * 4 + [M.UNMAPPED]
    sets = [(0,), (0,), (2,), (0, 1), (0, 1), (1, 2), (0, 1, 2), ()]
    classes = M.classes_of(sets)
    theta, share, it, delta = M.em(classes, lengths, k, 200, 1e-9)
    unique, compatible = [2, 0, 1], [5, 4, 3]
    n = sum(c for _, c in classes)
    assert abundance_text(names, lengths, unique, compatible, theta, share, n, it, delta, len(classes)) == \
        M.abundance_file(names, lengths, types, sets, k)
    # and the model's own file with the columns: the same lines, longer
    boot = bootstrap_file(names, lengths, types, sets, k, 10, 3)
    old = M.abundance_file(names, lengths, types, sets, k).splitlines()
    new = boot.splitlines()
    assert len(new) == len(old) and all(b.startswith(a + "\t") for a, b in zip(old, new))
    assert [b.count("\t") - a.count("\t") for a, b in zip(old, new)] == [4] * (len(old) - 1) + [6]
    _, _, sh, _, _ = bootstrap(classes, lengths, k, 10, 3, 200, 1e-9)
    assert boot == abundance_text(names, lengths, unique, compatible, theta, share, n, it, delta, len(classes),
                                  (summary(sh, 0.95), 10, 3, 0.95))


# ---- the flag checks ----------------------------------------------------------------------------

def test_parse_arguments_accepts_bootstrap_flags():
    import main
    base = ["-t", "dumpalign", "-g", "x.fa", "-k", "21", "--reads", "r.fq"]
    a = main.parse_arguments(base + ["--abundance", "a.tsv", "--abundance-bootstraps", "100", "--abundance-seed",
                                     str(2 ** 64 - 1), "--abundance-confidence", "0.9"])
    assert (a.abundance_bootstraps, a.abundance_seed, a.abundance_confidence) == (100, 2 ** 64 - 1, 0.9)
    b = main.parse_arguments(base + ["--abundance", "a.tsv"])
    assert (b.abundance_bootstraps, b.abundance_seed, b.abundance_confidence) == (None, None, None)
    for flag in ("--abundance-bootstraps", "--abundance-seed", "--abundance-confidence"):
        assert flag in main._ABUNDANCE_FLAGS and main._has_abundance_flag([flag + "=1"])
    assert main._early_reads_path(base + ["--abundance-bootstraps", "5"]) is None
    assert "--abundance-bootstraps B" in main.__doc__ and "--abundance-seed S" in main.__doc__


BASE = ["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ]
NEED = "Error: --abundance-bootstraps, --abundance-seed and --abundance-confidence need --abundance."


@pytest.mark.parametrize("argv, message", [
    (BASE + ["--abundance-bootstraps", "5"], NEED),
    (BASE + ["--abundance-seed", "5"], NEED),
    (BASE + ["--abundance-confidence", "0.9"], NEED),
    (BASE + ["--abundance", "a.tsv", "--abundance-seed", "5"], "need --abundance-bootstraps"),
    (BASE + ["--abundance", "a.tsv", "--abundance-confidence", "0.9"], "need --abundance-bootstraps"),
    (BASE + ["--abundance", "a.tsv", "--abundance-bootstraps", "0"], "--abundance-bootstraps must be in 1 .. 10000"),
    (BASE + ["--abundance", "a.tsv", "--abundance-bootstraps", "10001"],
     "--abundance-bootstraps must be in 1 .. 10000"),
    (BASE + ["--abundance", "a.tsv", "--abundance-bootstraps", "5", "--abundance-seed=-1"],
     "--abundance-seed must be in 0 .. 2^64 - 1"),
    (BASE + ["--abundance", "a.tsv", "--abundance-bootstraps", "5", "--abundance-seed", str(2 ** 64)],
     "--abundance-seed must be in 0 .. 2^64 - 1"),
    (BASE + ["--abundance", "a.tsv", "--abundance-bootstraps", "5", "--abundance-confidence", "0"],
     "--abundance-confidence must be in 0.001 .. 0.999"),
    (BASE + ["--abundance", "a.tsv", "--abundance-bootstraps", "5", "--abundance-confidence", "1"],
     "--abundance-confidence must be in 0.001 .. 0.999"),
    (BASE + ["--abundance", "a.tsv", "--abundance-bootstraps", "5", "--abundance-confidence", "0.9996"],
     "--abundance-confidence must be in 0.001 .. 0.999"),
    (BASE + ["--abundance", "a.tsv", "--abundance-bootstraps", "5", "--abundance-confidence", "nan"],
     "--abundance-confidence must be in 0.001 .. 0.999"),
    (["-t", "dumpalign", "-a", "x.aln", "--abundance", "a.tsv", "--abundance-bootstraps", "5"],
     "only allowed for task 'dumpalign' with --reads"),
], ids=["bootstraps_alone", "seed_alone", "confidence_alone", "seed_without_bootstraps",
        "confidence_without_bootstraps", "bootstraps_0", "bootstraps_10001", "seed_negative", "seed_2_64",
        "confidence_0", "confidence_1", "confidence_rounds_to_1", "confidence_nan", "alignfile"])
def test_cli_bootstrap_misuse(argv, message, tmp_path):
    """The flag checks end the process before any device work."""
    r = subprocess.run([sys.executable, MAIN] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=60, cwd=str(tmp_path), env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode != 0 and r.stdout == ""
    err = r.stderr.strip()
    assert err.startswith("Error:") and len(err.splitlines()) == 1 and message in err


# ---- the C entry point without a device ---------------------------------------------------------

def test_export_and_null_handle():
    assert "pa_abundance_bootstrap" in N.EXPORTS
    st = N.lib().pa_abundance_bootstrap(None, 5, 1, 10, 0.0, None, None, None, None, None, None)
    assert st == N.PA_EINVAL and b"NULL argument" in N.lib().pa_last_error()
