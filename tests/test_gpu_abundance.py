"""Genome abundance on the GPU (pa_align_candidates, pa_abundance_*, Abundance,
PseudoAlignment(abundance=True), main.py --abundance).

The reference has no such code.  The model is tests/test_abundance_host.py's:
plain Python and numpy from the genome texts, nothing of libpa in it; its
mapping types are cross-checked against the CPU oracle's on every batch.
Candidate sets and classes are compared for exact equality, the estimates
within 1e-9 (both are doubles and only the summation order may differ: at most
(entries per genome) x 2^-53 per iteration, far below 1e-12 over 50 iterations
at these sizes; the measured maximum is printed by the test).
"""

import functools
import io

import numpy as np
import pytest

import pa_native as N
import pa_oracle as O
import test_abundance_host as M
import test_gpu_coverage as TC

pytestmark = pytest.mark.gpu

UNIQUE, AMBIGUOUS = M.UNIQUE, M.AMBIGUOUS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X (no CPU fallback exists)")


def params(ps):
    return N.Params.make(ps.get("m", 1), ps.get("p", 1), ps.get("mrq"), ps.get("mkq"), ps.get("mg"))


def model_of(genomes, both, k, seqs, quals, ps, kd=None):
    """(types, sets, demoted) of the model, its types checked against the oracle's."""
    kd = M.kmer_sets(genomes, both, k) if kd is None else kd
    types, sets, dem = M.classify_all(kd, k, seqs, quals, **ps)
    seq, off = O.concat(seqs)
    qual, _ = O.concat(quals)
    o = TC.oracle_lists(genomes, both, k, (seq, qual, off), ps)
    assert o.types.tolist() == types
    for r, (t, c) in enumerate(zip(types, sets)):  # a unique read's list is [g]; an ambiguous one's never empty here
        if t == UNIQUE:
            assert tuple(o.genomes_of(r)) == c
        assert (len(c) >= 1) == (t in (UNIQUE, AMBIGUOUS))
    return types, sets, dem


def sets_of(off, flat):
    return [tuple(int(x) for x in flat[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def classes_list(ab):
    off, gen, cnt = ab.classes()
    return [(c, int(n)) for c, n in zip(sets_of(off, gen), cnt)]


def check_device(index, dev, prm, types, sets):
    """pa_align_candidates read by read, and the classes of a fresh accumulator, order included."""
    t, off, flat = N.align_candidates(index, dev, prm)
    assert t.tolist() == types
    assert sets_of(off, flat) == sets
    ab = N.Abundance(index)
    ab.add(dev, prm)
    want = M.classes_of(sets)
    assert classes_list(ab) == want
    info = ab.info()
    assert [info[n] for n in ("reads_unique", "reads_ambiguous", "reads_unmapped", "reads_dropped")] == \
        [types.count(x) for x in (UNIQUE, AMBIGUOUS, M.UNMAPPED, M.DROPPED)]
    assert (info["n_classes"], info["class_entries"]) == (len(want), sum(len(c) for c, _ in want))
    return ab


# ---- 1. hand-built ---------------------------------------------------------------------------

HAND_PS = dict(m=1, p=1, mrq=50)


@functools.lru_cache(maxsize=None)
def hand_case(k):
    """Three genomes sharing one stretch S3; g0 and g1 share S2, g1 and g2 share S12.
    Returns (genomes, [(name, seq, qual)])."""
    rng = np.random.default_rng(100 + k)
    P = [TC.rand_dna(rng, k + 70) for _ in range(9)]
    S3, S2, S12 = TC.rand_dna(rng, 2 * k + 140), TC.rand_dna(rng, 2 * k + 90), TC.rand_dna(rng, 2 * k + 60)
    g0 = P[0] + S3 + P[1] + S2 + P[2]
    g1 = P[3] + S3 + P[4] + S2 + P[5] + S12
    g2 = P[6] + S3 + P[7] + S12 + P[8]
    a3 = len(P[0])

    def sub(s, i):
        return s[:i] + ("A" if s[i] != "A" else "C") + s[i + 1:]
    reads = [
        ("in3_a", S3[0:k + 40]), ("in3_b", S3[10:k + 55]), ("in3_c", S3[len(S3) - k - 30:]),
        ("in2_a", S2[5:k + 35]), ("in2_b", S2[20:k + 60]),
        ("in12", S12[3:k + 33]),
        ("boundary0", g0[a3 - k - 5:a3 + k + 5]),              # private | shared: unique to g0
        ("boundary2", g2[len(P[6]) + len(S3) - 20:len(P[6]) + len(S3) + k + 10]),
        # 3 k-mers specific to g0, 11 of {g1, g2}; the base between extends neither genome's match
        ("p_demoted", P[0][0:k + 2] + next(b for b in "ACGT" if b not in (P[5][-1], P[7][-1])) + S12[0:k + 10]),
        ("subset", S3[30:k + 35] + S2[40:k + 46]),             # touches all three, the maximum in {g0, g1}
        ("substitution", sub(S3[20:2 * k + 30], k + 4)),
        ("with_n", S2[10:k + 15] + "N" + S2[k + 16:2 * k + 40]),
        ("short", S3[0:k - 1]),
        ("dropped", S3[0:k + 40]),
        ("reverse", M.reverse_complement(S3[5:k + 45])),       # forward index: unmapped; both strands: all three
        ("private1", P[4][3:k + 30]),
    ]
    return [g0, g1, g2], [(n, s, ("#" if n == "dropped" else "I") * len(s)) for n, s in reads]


@pytest.mark.parametrize("both", [False, True], ids=["forward", "both_strands"])
@pytest.mark.parametrize("k", [31, 63, 127])  # (127: four key words, the exact path only)
def test_hand_built(k, both):
    genomes, reads = hand_case(k)
    names, seqs, quals = [r[0] for r in reads], [r[1] for r in reads], [r[2] for r in reads]
    types, sets, dem = model_of(genomes, both, k, seqs, quals, HAND_PS)
    got = dict(zip(names, zip(types, sets, dem)))
    # the corners are what they are named for
    for n in ("in3_a", "in3_b", "in3_c", "substitution"):
        assert got[n] == (AMBIGUOUS, (0, 1, 2), False)
    assert got["in2_a"][:2] == got["in2_b"][:2] == got["with_n"][:2] == (AMBIGUOUS, (0, 1))
    assert got["in12"][:2] == (AMBIGUOUS, (1, 2))
    assert got["boundary0"][:2] == (UNIQUE, (0,)) and got["boundary2"][:2] == (UNIQUE, (2,))
    assert got["p_demoted"] == (AMBIGUOUS, (1, 2), True)
    assert got["subset"] == (AMBIGUOUS, (0, 1), False)
    assert got["short"][0] == M.UNMAPPED and got["dropped"][0] == M.DROPPED
    assert got["reverse"][:2] == ((AMBIGUOUS, (0, 1, 2)) if both else (M.UNMAPPED, ()))
    assert got["private1"][:2] == (UNIQUE, (1,))
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(genomes, k, both_strands=both)
    ab = check_device(index, dev, params(HAND_PS), types, sets)
    for x in (ab, dev, index):
        x.close()


# ---- 2. random strains -----------------------------------------------------------------------

RAND_SEED = 5
RAND_K = 31
RAND_PS = [dict(m=1, p=1), dict(m=0, p=3), dict(m=3, p=0), dict(m=1, p=-1), dict(m=1, p=1, mkq=61),
           dict(m=1, p=1, mg=2), dict(m=1, p=1, mg=0), dict(m=2, p=1, mkq=58, mg=2)]


@functools.lru_cache(maxsize=None)
def rand_strains():
    """12 genomes of about 2 kb: four ancestors, each with a copy mutated at 0.4 %
    and a copy of that copy mutated again (so two strains share what the third lacks)."""
    rng = np.random.default_rng(RAND_SEED)
    genomes = []
    for _ in range(4):
        a = TC.rand_dna(rng, int(rng.integers(1900, 2100)))
        b = TC.mutate(rng, a, 0.004)
        c = TC.mutate(rng, b, 0.004)
        genomes += [a, b, c]
    return genomes


@functools.lru_cache(maxsize=None)
def rand_reads(n=4000):
    """n reads of 100-150 bases with 1 % errors, qualities uniform in 50..74; one
    in twenty is a chimera: a short piece of one strain, then a long piece of a
    strain of another ancestor."""
    rng = np.random.default_rng(RAND_SEED + 1)
    genomes = rand_strains()
    seqs, quals = [], []
    for i in range(n):
        ln = int(rng.integers(100, 151))
        gi = int(rng.integers(0, len(genomes)))
        g = genomes[gi]
        if i % 20 == 19:
            h = genomes[(gi + 3 * int(rng.integers(1, 4))) % len(genomes)]
            cut = int(rng.integers(RAND_K + 1, RAND_K + 8))
            a, b = int(rng.integers(0, len(g) - cut)), int(rng.integers(0, len(h) - ln))
            s = g[a:a + cut] + h[b:b + ln - cut]
        else:
            a = int(rng.integers(0, len(g) - ln + 1))
            s = g[a:a + ln]
        seqs.append(TC.mutate(rng, s, 0.01))
        quals.append(bytes(rng.integers(50, 75, ln, dtype=np.uint8)).decode())
    return seqs, quals


@functools.lru_cache(maxsize=None)
def rand_kd():
    return M.kmer_sets(rand_strains(), False, RAND_K)


@functools.lru_cache(maxsize=None)
def rand_model(i):
    seqs, quals = rand_reads()
    return model_of(rand_strains(), False, RAND_K, seqs, quals, RAND_PS[i], rand_kd())


def test_random_batch_conditions():
    """What the batch must hold, on the model's side, before any device result is looked at."""
    types, sets, dem = rand_model(0)
    assert types.count(AMBIGUOUS) >= 0.2 * len(types)
    assert len({c for c in sets if len(c) >= 2}) >= 3
    assert sum(dem) >= 1
    assert types.count(UNIQUE) >= 0.1 * len(types)


@pytest.mark.parametrize("i", range(len(RAND_PS)), ids=[",".join(f"{a}={b}" for a, b in ps.items()) for ps in RAND_PS])
def test_random_strains(i):
    types, sets, dem = rand_model(i)
    seqs, quals = rand_reads()
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(rand_strains(), RAND_K)
    ab = check_device(index, dev, params(RAND_PS[i]), types, sets)
    for x in (ab, dev, index):
        x.close()


# ---- 3. large sets ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def large_case(G, length, stretch, k, n_reads):
    """G genomes of `length` bases that all hold one stretch; reads from the stretch, from private parts, across."""
    rng = np.random.default_rng(G)
    S = TC.rand_dna(rng, stretch)
    genomes, at = [], []
    for _ in range(G):
        a = int(rng.integers(0, length - stretch + 1))
        body = TC.rand_dna(rng, length - stretch)
        genomes.append(body[:a] + S + body[a:])
        at.append(a)
    seqs = []
    for i in range(n_reads):
        ln = int(rng.integers(k + 3, min(2 * k + 20, length) + 1))
        if i % 3 == 0:   # inside the stretch
            ln = min(ln, stretch)
            a = int(rng.integers(0, stretch - ln + 1))
            seqs.append(S[a:a + ln])
        else:            # anywhere on a genome
            g = genomes[int(rng.integers(0, G))]
            a = int(rng.integers(0, length - ln + 1))
            seqs.append(g[a:a + ln])
    return genomes, seqs, ["I" * len(s) for s in seqs]


@pytest.mark.parametrize("G, length, stretch, k, n_reads", [(300, 500, 200, 31, 90), (2100, 70, 40, 21, 60)],
                         ids=["300_genomes", "2100_genomes"])
def test_large_sets(G, length, stretch, k, n_reads):
    """A set larger than a wave and than a workgroup (300), and larger than what
    the kernels keep in LDS (2100: past the staged ranks and the LDS histogram)."""
    genomes, seqs, quals = large_case(G, length, stretch, k, n_reads)
    ps = dict(m=1, p=1)
    types, sets, dem = model_of(genomes, False, k, seqs, quals, ps)
    assert sum(len(c) == G for c in sets) >= n_reads // 3 and types.count(UNIQUE) >= n_reads // 4
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(genomes, k)
    ab = check_device(index, dev, params(ps), types, sets)
    theta, share, it, delta = ab.estimate(20, 0.0)
    mt, ms, _, _ = M.em(M.classes_of(sets), [len(g) for g in genomes], k, 20, 0.0)
    assert np.max(np.abs(theta - mt)) <= 1e-9 and np.max(np.abs(share - ms)) <= 1e-9
    for x in (ab, dev, index):
        x.close()


# ---- 4. estimates ----------------------------------------------------------------------------

def test_estimates():
    types, sets, _ = rand_model(0)
    genomes = rand_strains()
    lengths = [len(g) for g in genomes]
    classes = M.classes_of(sets)
    seqs, quals = rand_reads()
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(genomes, RAND_K)
    ab = N.Abundance(index)
    ab.add(dev, params(RAND_PS[0]))
    theta, share, it, delta = ab.estimate(50, 0.0)
    mt, ms, mit, mdelta = M.em(classes, lengths, RAND_K, 50, 0.0)
    d_theta, d_share = float(np.max(np.abs(theta - mt))), float(np.max(np.abs(share - ms)))
    print(f"abundance estimate vs numpy EM, 50 iterations: max |d theta| = {d_theta:.3e}, "
          f"max |d abundance| = {d_share:.3e}, delta {delta:.3e} vs {mdelta:.3e}")
    assert it == mit == 50
    assert d_theta <= 1e-9 and d_share <= 1e-9
    assert abs(float(theta.sum()) - 1) <= 1e-12 and abs(float(share.sum()) - 1) <= 1e-12
    assert abs(delta - mdelta) <= 1e-9
    # early stop
    t2, s2, it2, delta2 = ab.estimate(10000, 1e-6)
    _, _, mit2, _ = M.em(classes, lengths, RAND_K, 10000, 1e-6)
    print(f"tolerance 1e-6: {it2} iterations on the device, {mit2} in the model, last delta {delta2:.3e}")
    assert it2 < 10000 and delta2 < 1e-6 and abs(it2 - mit2) <= 1
    # the Python API's defaults are 200 iterations and 1e-9
    assert ab.estimate()[2] <= 200
    for bad in ((0, 0.0), (10001, 0.0), (5, -1e-9), (5, float("nan"))):
        assert N.lib().pa_abundance_estimate(ab.handle, bad[0], bad[1], None, None, None, None, None) == N.PA_EINVAL
    with pytest.raises(ValueError):
        ab.estimate(0)
    with pytest.raises(ValueError):
        ab.estimate(5, -1.0)
    for x in (ab, dev, index):
        x.close()


def test_identical_genomes_keep_equal_estimates():
    genomes = list(rand_strains()) + [rand_strains()[4]]  # genome 12 is genome 4 again
    seqs, quals = rand_reads()
    seqs, quals = list(seqs[:1500]), list(quals[:1500])
    ps = RAND_PS[0]
    types, sets, _ = model_of(genomes, False, RAND_K, seqs, quals, ps)
    assert all((4 in c) == (12 in c) for c in sets) and sum(4 in c for c in sets) >= 50
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(genomes, RAND_K)
    ab = check_device(index, dev, params(ps), types, sets)
    for iters in (1, 50):
        theta, share, _, _ = ab.estimate(iters, 0.0)
        assert theta[4] == theta[12] and share[4] == share[12] and theta[4] > 0
    for x in (ab, dev, index):
        x.close()


# ---- 5. determinism and protocol -------------------------------------------------------------

def bits(arrs):
    return [a.tobytes() for a in arrs[:2]] + list(arrs[2:])


def test_determinism_and_batches():
    seqs, quals = rand_reads()
    seqs, quals = list(seqs[:1800]), list(quals[:1800])
    prm = params(RAND_PS[0])
    index = N.Index(rand_strains(), RAND_K)
    whole, _ = TC.upload(seqs, quals)
    parts = [TC.upload(seqs[a:b], quals[a:b])[0] for a, b in ((0, 500), (500, 1300), (1300, 1800))]
    one, three = N.Abundance(index), N.Abundance(index)
    one.add(whole, prm)
    for p in parts:
        three.add(p, prm)
    ref = classes_list(one)
    assert len(ref) >= 10 and classes_list(three) == ref and three.info() == one.info()
    e1 = bits(one.estimate(60, 0.0))
    assert bits(one.estimate(60, 0.0)) == e1          # the same accumulator twice: the same bits
    assert bits(three.estimate(60, 0.0)) == e1        # the same reads in three batches: the same bits
    assert bits(one.estimate(10000, 1e-7)) == bits(three.estimate(10000, 1e-7))
    # reset
    three.reset()
    assert classes_list(three) == [] and three.info() == dict.fromkeys(one.info(), 0)
    th, sh, it, delta = three.estimate(10, 0.0)       # an empty accumulator: zeros, no iteration
    assert not th.any() and not sh.any() and (it, delta) == (0, 0.0)
    three.add(whole, prm)
    assert classes_list(three) == ref
    for x in [one, three, whole, index] + parts:
        x.close()


def test_assign_off_gives_equal_classes(monkeypatch):
    seqs, quals = rand_reads()
    seqs, quals = list(seqs[:1200]), list(quals[:1200])
    prm = params(RAND_PS[0])
    index = N.Index(rand_strains(), RAND_K)
    dev, _ = TC.upload(seqs, quals)
    ab = N.Abundance(index)
    ab.add(dev, prm)
    ref, cand = classes_list(ab), N.align_candidates(index, dev, prm)
    monkeypatch.setenv("PA_ASSIGN", "0")
    ab.reset()
    ab.add(dev, prm)
    again = N.align_candidates(index, dev, prm)
    assert classes_list(ab) == ref and len(ref) >= 10
    assert all(np.array_equal(a, b) for a, b in zip(cand, again))
    for x in (ab, dev, index):
        x.close()


def test_protocol():
    genomes = rand_strains()
    seqs, quals = rand_reads()
    seqs, quals = list(seqs[:600]), list(quals[:600])
    prm = params(RAND_PS[0])
    index, other = N.Index(genomes, RAND_K), N.Index(genomes, RAND_K)
    dev, _ = TC.upload(seqs, quals)
    b0 = int(index.info().device_bytes)
    res = N.Result(index)
    N.align(index, dev, prm, 0, res)
    before = [np.array(a, copy=True) for a in res.fetch()]
    b1 = int(index.info().device_bytes)
    ab = N.Abundance(index)
    ab.add(dev, prm)
    assert int(index.info().device_bytes) == b1 >= b0  # the accumulator's bytes are not the index's
    assert all(np.array_equal(a, b) for a, b in zip(before, res.fetch()))  # a caller's pa_result untouched
    lib = N.lib()
    # pa_abundance_classes: the sizes always, nothing written when a capacity is too small
    st, off, gen, cnt, nc, ne = ab.classes_call(0, 0)
    assert st == N.PA_EINVAL and nc >= 10 and ne > nc
    assert classes_list(ab) and len(classes_list(ab)) == nc
    for cap_c, cap_e in ((nc - 1, ne), (nc, ne - 1)):
        off = np.full(cap_c + 1, 77, dtype=np.uint64)
        gen = np.full(max(cap_e, 1), 77, dtype=np.uint32)
        cnt = np.full(max(cap_c, 1), 77, dtype=np.uint64)
        a, b = N.U64(0), N.U64(0)
        assert lib.pa_abundance_classes(ab.handle, N._ptr(off), N._ptr(gen), N._ptr(cnt), cap_c, cap_e,
                                        N.ctypes.byref(a), N.ctypes.byref(b), None) == N.PA_EINVAL
        assert (int(a.value), int(b.value)) == (nc, ne)
        assert (off == 77).all() and (gen == 77).all() and (cnt == 77).all()
    st, off, gen, cnt, nc2, ne2 = ab.classes_call(nc, ne)
    assert st == N.PA_OK and (nc2, ne2) == (nc, ne) and int(off[nc]) == ne
    # pa_align_candidates: too small a cap leaves the types, offsets and the total valid
    types, coff, flat = N.align_candidates(index, dev, prm)
    total = int(coff[-1])
    st, t2, off2, sets2, tot2 = N.align_candidates_call(index, dev, prm, 0)
    assert st == N.PA_EINVAL and tot2 == total == flat.size and sets2 is None
    assert t2.tolist() == types.tolist() and off2.tolist() == coff.tolist()
    st, t3, off3, sets3, tot3 = N.align_candidates_call(index, dev, prm, total - 1)
    assert st == N.PA_EINVAL and tot3 == total
    st, t4, off4, sets4, tot4 = N.align_candidates_call(index, dev, prm, total)
    assert st == N.PA_OK and sets4[:total].tolist() == flat.tolist()
    # another index; its own index after a reduce
    assert lib.pa_abundance_add(other.handle, dev.handle, prm, ab.handle, None) == N.PA_EINVAL
    ref = classes_list(ab)
    index.reduce([0, 2, 3, 5])
    with pytest.raises(ValueError):
        ab.add(dev, prm)
    assert classes_list(ab) == ref  # (what it holds stays readable)
    # an empty accumulator and an empty batch
    fresh = N.Abundance(other)
    assert classes_list(fresh) == [] and fresh.info()["n_classes"] == 0
    th, sh, it, delta = fresh.estimate(5, 0.0)
    assert th.shape == (len(genomes),) and not th.any() and not sh.any() and (it, delta) == (0, 0.0)
    for x in (ab, fresh, res, dev, index, other):
        x.close()


# ---- 6. drop-in API and CLI ------------------------------------------------------------------

CLI_CASES, FA, FQ = TC.CLI_CASES, TC.FA, TC.FQ


@functools.lru_cache(maxsize=None)
def config1_text(both=False, iterations=200, tolerance=1e-9):
    gen, reads = TC.config1()
    gs = [g for _, g in gen]
    seqs, quals = [s for s, _ in reads], [q for _, q in reads]
    types, sets, _ = model_of(gs, both, 21, seqs, quals, dict(m=1, p=1))
    return M.abundance_file([n for n, _ in gen], [len(g) for g in gs], types, sets, 21, iterations, tolerance)


def test_cli_abundance(tmp_path):
    from data_file import FASTAFile
    from kmer import KmerReference, PseudoAlignment
    f = str(tmp_path / "a.tsv")
    r = TC.run_cli(["--abundance", f])
    assert r.returncode == 0, r.stderr
    assert r.stdout == CLI_CASES[0]["stdout"]  # stdout: what is pinned without the flag
    text = open(f).read()
    assert text == config1_text()
    ref = KmerReference(21, FASTAFile(FA).container)
    plain = PseudoAlignment(ref)
    for fn in (plain.get_abundance, lambda: plain.write_abundance(io.StringIO())):
        with pytest.raises(ValueError):
            fn()
    pa = PseudoAlignment(ref, abundance=True)
    pa.align_reads_from_file(FQ)
    buf = io.StringIO()
    pa.write_abundance(buf)
    assert buf.getvalue() == text
    a = pa.get_abundance()
    assert [g["genome"] for g in a["genomes"]] == [n for n, _ in TC.config1()[0]]
    assert abs(sum(g["read_fraction"] for g in a["genomes"]) - 1) <= 1e-12
    for bad in ((0, 1e-9), (10001, 1e-9), (5, -1.0), (True, 0.0)):
        with pytest.raises(ValueError):
            pa.get_abundance(*bad)
    assert not any("bundance" in key for key in pa.__getstate__())  # (never part of an .aln file)
    r = TC.run_cli(["--abundance", f, "--abundance-iterations", "7", "--abundance-tolerance", "0"])
    assert r.returncode == 0, r.stderr
    assert open(f).read() == config1_text(False, 7, 0.0) and "#iterations\t7\t" in open(f).read()


def test_cli_abundance_filter_similar(tmp_path):
    """After --filter-similar the file has one line per kept genome, in the index's order."""
    from data_file import FASTAFile
    from kmer import KmerReference
    f = str(tmp_path / "a.tsv")
    flags = ["--filter-similar", "--similarity-threshold", "0.5"]
    r, plain = TC.run_cli(flags + ["--abundance", f]), TC.run_cli(flags)
    assert r.returncode == 0 and plain.returncode == 0, r.stderr + plain.stderr
    assert r.stdout == plain.stdout
    ref = KmerReference(21, FASTAFile(FA).container, filter_similar=True, similarity_threshold=0.5)
    kept = [g.identifier for g in ref.genomes]
    lines = open(f).read().splitlines()
    assert [ln.split("\t")[0] for ln in lines[1:-1]] == kept and 1 <= len(kept) <= 3
    assert lines[0].startswith("#genome\t") and lines[-1].startswith("#iterations\t")
    assert abs(sum(float(ln.split("\t")[5]) for ln in lines[1:-1]) - 1) < 1e-8


def test_cli_abundance_composes(tmp_path):
    f, v, a = str(tmp_path / "a.tsv"), str(tmp_path / "v.tsv"), str(tmp_path / "as.tsv")
    r = TC.run_cli(["--both-strands", "--coverage", "--variants", v, "--assignments", a, "--abundance", f])
    plain = TC.run_cli(["--both-strands", "--coverage", "--variants", str(tmp_path / "v2.tsv"),
                        "--assignments", str(tmp_path / "as2.tsv")])
    assert r.returncode == 0 and plain.returncode == 0, r.stderr + plain.stderr
    assert r.stdout == plain.stdout
    assert open(v).read() == open(str(tmp_path / "v2.tsv")).read()
    assert open(a).read() == open(str(tmp_path / "as2.tsv")).read()
    assert open(f).read() == config1_text(True)
