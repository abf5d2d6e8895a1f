"""Bootstrap replicates of the abundance estimate on the GPU
(pa_abundance_bootstrap, Abundance.bootstrap, get_abundance(bootstraps=...),
main.py --abundance-bootstraps).

The model is tests/test_bootstrap_host.py's: the draws in integers, the EM
test_abundance_host.em.  The resampled counts are compared for exact equality
(section 16 defines them in integers), the estimates within section 14's 1e-9
(the kernel keeps k_em_e's and k_em_m's terms and their order, so the measured
difference, printed by the test, is expected to be 0).
"""

import io

import numpy as np
import pytest

import pa_native as N
import test_abundance_host as M
import test_bootstrap_host as H
import test_gpu_abundance as A
import test_gpu_coverage as TC

pytestmark = pytest.mark.gpu

PS = A.RAND_PS[0]
K = A.RAND_K


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X (no CPU fallback exists)")


@pytest.fixture(scope="module")
def strains():
    """The 12-strain batch (about 4 000 reads, two dozen classes) in one accumulator:
    (accumulator, index, the uploaded batch, the model's classes, the genome lengths)."""
    _, sets, _ = A.rand_model(0)
    seqs, quals = A.rand_reads()
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(A.rand_strains(), K)
    ab = N.Abundance(index)
    ab.add(dev, A.params(PS))
    classes = M.classes_of(sets)
    assert A.classes_list(ab) == classes and 20 <= len(classes) <= 40
    yield ab, index, dev, classes, [len(g) for g in A.rand_strains()]
    for x in (ab, dev, index):
        x.close()


def model_counts(classes, B, seed):
    return H.resample([n for _, n in classes], B, seed).tolist()


# ---- 1. the resampled counts -------------------------------------------------------------------

@pytest.mark.parametrize("lds", ["1", "0"], ids=["lds", "global"])
@pytest.mark.parametrize("seed", [1, 2 ** 63 + 5])
def test_counts(strains, seed, lds, monkeypatch):
    ab, _, _, classes, _ = strains
    monkeypatch.setenv("PA_BOOT_LDS", lds)
    theta, share, its, delta, counts = ab.bootstrap(8, seed, 3, 0.0, counts=True)
    assert counts.dtype == np.uint64 and counts.shape == (8, len(classes))
    assert counts.tolist() == model_counts(classes, 8, seed)
    assert (counts.sum(axis=1) == sum(n for _, n in classes)).all() and its.tolist() == [3] * 8


@pytest.mark.parametrize("lds", ["1", "0"], ids=["lds", "global"])
def test_counts_more_draws_than_threads(strains, lds, monkeypatch):
    """The batch 40 times: N about 1.6 x 10^5, so a thread draws more than once and a replicate takes several blocks."""
    _, index, dev, classes, _ = strains
    ab = N.Abundance(index)
    for _ in range(40):
        ab.add(dev, A.params(PS))
    big = [(C, 40 * n) for C, n in classes]
    assert A.classes_list(ab) == big and sum(n for _, n in big) > 256 * 64 * 2
    monkeypatch.setenv("PA_BOOT_LDS", lds)
    counts = ab.bootstrap(4, 7, 1, 0.0, counts=True)[4]
    assert counts.tolist() == model_counts(big, 4, 7)
    ab.close()


def test_one_read_and_none(strains):
    _, index, _, _, lengths = strains
    types, sets, _ = A.rand_model(0)
    seqs, quals = A.rand_reads()
    r = next(i for i, t in enumerate(types) if t == M.AMBIGUOUS)
    one, _ = TC.upload([seqs[r]], [quals[r]])
    ab = N.Abundance(index)
    G = len(lengths)
    # empty: zeros and no iteration, with and without the counts
    theta, share, its, delta, counts = ab.bootstrap(3, 1, 10, 0.0, counts=True)
    assert theta.shape == share.shape == (3, G) and counts.shape == (3, 0)
    assert not theta.any() and not share.any() and its.tolist() == [0] * 3 and delta.tolist() == [0.0] * 3
    ab.add(one, A.params(PS))
    classes = [(sets[r], 1)]
    assert A.classes_list(ab) == classes
    theta, share, its, delta, counts = ab.bootstrap(5, 9, 10, 0.0, counts=True)
    assert counts.tolist() == [[1]] * 5 and its.tolist() == [10] * 5
    _, mt, ms, _, _ = H.bootstrap(classes, lengths, K, 5, 9, 10, 0.0)
    assert np.max(np.abs(theta - mt)) <= 1e-9 and np.max(np.abs(share - ms)) <= 1e-9
    for x in (ab, one):
        x.close()


# ---- 2. the EM ---------------------------------------------------------------------------------

def test_em_fixed_iterations(strains):
    ab, _, _, classes, lengths = strains
    theta, share, its, delta = ab.bootstrap(6, 1, 50, 0.0)
    _, mt, ms, mit, mdelta = H.bootstrap(classes, lengths, K, 6, 1, 50, 0.0)
    d_theta, d_share = float(np.max(np.abs(theta - mt))), float(np.max(np.abs(share - ms)))
    print(f"bootstrap vs numpy EM, 6 replicates of 50 iterations: max |d theta| = {d_theta:.3e}, "
          f"max |d abundance| = {d_share:.3e}, max |d delta| = {float(np.max(np.abs(delta - mdelta))):.3e}")
    assert its.tolist() == mit.tolist() == [50] * 6
    assert d_theta <= 1e-9 and d_share <= 1e-9
    assert np.max(np.abs(theta.sum(axis=1) - 1)) <= 1e-12 and np.max(np.abs(share.sum(axis=1) - 1)) <= 1e-12
    assert np.max(np.abs(delta - mdelta)) <= 1e-9
    assert len({r.tobytes() for r in theta}) == 6     # six different resamples


def test_em_stops_per_replicate(strains):
    ab, _, _, classes, lengths = strains
    _, mt, _, mit, _ = H.bootstrap(classes, lengths, K, 6, 1, 10000, 1e-6)
    assert len(set(mit.tolist())) >= 3 and max(mit) < 10000   # the model's replicates stop at different iterations
    theta, share, its, delta = ab.bootstrap(6, 1, 10000, 1e-6)
    print(f"tolerance 1e-6: iterations {its.tolist()} on the device, {mit.tolist()} in the model, "
          f"last deltas {delta.tolist()}")
    assert all(abs(int(a) - int(b)) <= 1 for a, b in zip(its, mit))
    assert (delta < 1e-6).all() and (delta > 0).all()
    # the defaults are the point estimate's: 200 iterations, 1e-9
    assert (ab.bootstrap(2)[2] <= 200).all()


@pytest.mark.parametrize("G, length, stretch, k, n_reads", [(300, 500, 200, 31, 90), (2100, 70, 40, 21, 60)],
                         ids=["300_genomes", "2100_genomes"])
def test_more_genomes_than_threads(G, length, stretch, k, n_reads):
    """test_large_sets' shapes: more genomes than the workgroup has threads, classes of G genomes."""
    genomes, seqs, quals = A.large_case(G, length, stretch, k, n_reads)
    _, sets, _ = M.classify_all(M.kmer_sets(genomes, False, k), k, seqs, quals, m=1, p=1)
    classes, lengths = M.classes_of(sets), [len(g) for g in genomes]
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(genomes, k)
    ab = N.Abundance(index)
    ab.add(dev, A.params(dict(m=1, p=1)))
    assert A.classes_list(ab) == classes and max(len(C) for C, _ in classes) == G
    theta, share, its, delta, counts = ab.bootstrap(3, 11, 20, 0.0, counts=True)
    mc, mt, ms, _, mdelta = H.bootstrap(classes, lengths, k, 3, 11, 20, 0.0)
    assert counts.tolist() == mc.tolist() and its.tolist() == [20] * 3
    assert np.max(np.abs(theta - mt)) <= 1e-9 and np.max(np.abs(share - ms)) <= 1e-9
    assert np.max(np.abs(delta - mdelta)) <= 1e-9
    for x in (ab, dev, index):
        x.close()


# ---- 3. invariants -----------------------------------------------------------------------------

def test_absent_and_identical_genomes():
    """Genome 12 is genome 4 again, genome 13 is in no read: theta_b[4] == theta_b[12] and theta_b[13] == 0 in
    every replicate."""
    rng = np.random.default_rng(77)
    genomes = list(A.rand_strains()) + [A.rand_strains()[4], TC.rand_dna(rng, 2000)]
    seqs, quals = A.rand_reads()
    seqs, quals = list(seqs[:1500]), list(quals[:1500])
    _, sets, _ = M.classify_all(M.kmer_sets(genomes, False, K), K, seqs, quals, **PS)
    assert all((4 in c) == (12 in c) for c in sets) and sum(4 in c for c in sets) >= 50
    assert not any(13 in c for c in sets)
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(genomes, K)
    ab = N.Abundance(index)
    ab.add(dev, A.params(PS))
    assert A.classes_list(ab) == M.classes_of(sets)
    for iters in (1, 50):
        theta, share, _, _ = ab.bootstrap(5, 2, iters, 0.0)
        assert (theta[:, 4] == theta[:, 12]).all() and (share[:, 4] == share[:, 12]).all() and (theta[:, 4] > 0).all()
        assert not theta[:, 13].any() and not share[:, 13].any()
    for x in (ab, dev, index):
        x.close()


def boot_bits(out):
    return [np.ascontiguousarray(a).tobytes() for a in out]


def test_determinism_batches_and_an_untouched_accumulator(strains):
    _, index, _, _, _ = strains
    seqs, quals = A.rand_reads()
    seqs, quals = list(seqs[:1800]), list(quals[:1800])
    prm = A.params(PS)
    whole, _ = TC.upload(seqs, quals)
    parts = [TC.upload(seqs[a:b], quals[a:b])[0] for a, b in ((0, 500), (500, 1300), (1300, 1800))]
    one, three = N.Abundance(index), N.Abundance(index)
    one.add(whole, prm)
    for p in parts:
        three.add(p, prm)
    before = ([a.tobytes() for a in one.classes()], A.bits(one.estimate(60, 0.0)), one.info())
    b1 = boot_bits(one.bootstrap(5, 4, 60, 0.0, counts=True))
    assert boot_bits(one.bootstrap(5, 4, 60, 0.0, counts=True)) == b1      # the same call twice: the same bytes
    assert boot_bits(three.bootstrap(5, 4, 60, 0.0, counts=True)) == b1    # the reads in three batches: the same
    assert boot_bits(one.bootstrap(5, 4, 10000, 1e-7)) == boot_bits(three.bootstrap(5, 4, 10000, 1e-7))
    assert boot_bits(one.bootstrap(5, 5, 60, 0.0, counts=True)) != b1      # another seed: other replicates
    # the accumulator and the point estimate are what they were
    assert ([a.tobytes() for a in one.classes()], A.bits(one.estimate(60, 0.0)), one.info()) == before
    for x in [one, three, whole] + parts:
        x.close()


# ---- 4. protocol -------------------------------------------------------------------------------

def test_protocol(strains):
    ab, index, dev, classes, lengths = strains
    lib = N.lib()
    nul = (None,) * 6
    for reps, its, tol in ((0, 5, 0.0), (10001, 5, 0.0), (5, 0, 0.0), (5, 10001, 0.0), (5, 5, -1e-9),
                           (5, 5, float("nan"))):
        assert lib.pa_abundance_bootstrap(ab.handle, reps, 1, its, tol, *nul) == N.PA_EINVAL, (reps, its, tol)
    assert lib.pa_abundance_bootstrap(None, 5, 1, 5, 0.0, *nul) == N.PA_EINVAL
    assert b"NULL argument" in lib.pa_last_error()
    assert lib.pa_abundance_bootstrap(ab.handle, 5, 1, 5, 0.0, *nul) == N.PA_OK     # every output may be NULL
    its = np.zeros(3, dtype=np.uint32)                                               # or only some
    assert lib.pa_abundance_bootstrap(ab.handle, 3, 1, 5, 0.0, None, None, None, N._ptr(its), None, None) == N.PA_OK
    assert its.tolist() == [5, 5, 5]
    assert ab.bootstrap(1)[0].shape == (1, len(lengths)) and ab.bootstrap(10000, iterations=1)[2].shape == (10000,)
    for bad in (dict(replicates=0), dict(replicates=10001), dict(replicates=True), dict(replicates=2.0),
                dict(replicates=3, seed=-1), dict(replicates=3, seed=2 ** 64), dict(replicates=3, iterations=0),
                dict(replicates=3, tolerance=-1.0)):
        with pytest.raises(ValueError):
            ab.bootstrap(**bad)
    # after a reset: an empty accumulator's answer, then the batch's again
    fresh = N.Abundance(index)
    fresh.add(dev, A.params(PS))
    ref = boot_bits(fresh.bootstrap(3, 1, 10, 0.0, counts=True))
    fresh.reset()
    theta, share, it, delta, counts = fresh.bootstrap(3, 1, 10, 0.0, counts=True)
    assert not theta.any() and not share.any() and it.tolist() == [0] * 3 and counts.shape == (3, 0)
    fresh.add(dev, A.params(PS))
    assert boot_bits(fresh.bootstrap(3, 1, 10, 0.0, counts=True)) == ref
    assert ref == boot_bits(ab.bootstrap(3, 1, 10, 0.0, counts=True))
    fresh.close()


# ---- 5. drop-in API and CLI --------------------------------------------------------------------

def config1_model():
    gen, reads = TC.config1()
    gs = [g for _, g in gen]
    types, sets, _ = A.model_of(gs, False, 21, [s for s, _ in reads], [q for _, q in reads], dict(m=1, p=1))
    return [n for n, _ in gen], [len(g) for g in gs], types, sets


def test_cli_and_api(tmp_path):
    from data_file import FASTAFile
    from kmer import ABUNDANCE_BOOTSTRAP_COLUMNS, KmerReference, PseudoAlignment
    names, lengths, types, sets = config1_model()
    want = H.bootstrap_file(names, lengths, types, sets, 21, 20, 3)
    f = str(tmp_path / "a.tsv")
    r = TC.run_cli(["--abundance", f, "--abundance-bootstraps", "20", "--abundance-seed", "3"])
    assert r.returncode == 0, r.stderr
    assert r.stdout == TC.CLI_CASES[0]["stdout"]
    assert open(f).read() == want
    pa = PseudoAlignment(KmerReference(21, FASTAFile(TC.FA).container), abundance=True)
    pa.align_reads_from_file(TC.FQ)
    plain = pa.get_abundance()
    buf = io.StringIO()
    pa.write_abundance(buf, bootstraps=20, seed=3)
    assert buf.getvalue() == want
    buf = io.StringIO()
    pa.write_abundance(buf)
    assert buf.getvalue() == A.config1_text()
    a = pa.get_abundance(bootstraps=20, seed=3)
    assert (a["bootstraps"], a["seed"], a["confidence"]) == (20, 3, 0.95)
    _, _, share, _, _ = H.bootstrap(M.classes_of(sets), lengths, 21, 20, 3, 200, 1e-9)
    for row, old, st in zip(a["genomes"], plain["genomes"], H.summary(share, 0.95)):
        assert {k: v for k, v in row.items() if k not in ABUNDANCE_BOOTSTRAP_COLUMNS} == old
        got = tuple(row[c] for c in ABUNDANCE_BOOTSTRAP_COLUMNS)
        assert max(abs(x - y) for x, y in zip(got, st)) <= 1e-9
        assert row["abundance_lo"] <= row["abundance_mean"] <= row["abundance_hi"] and row["abundance_sd"] >= 0
    assert {k: v for k, v in a.items() if k not in ("genomes", "bootstraps", "seed", "confidence")} == \
        {k: v for k, v in plain.items() if k != "genomes"}
    # without the new arguments: today's dict, whatever ran before
    again = pa.get_abundance()
    assert again == plain and set(again) == {"genomes", "reads", "iterations", "last_delta", "classes"}
    assert set(again["genomes"][0]) == {"genome", "length", "unique_reads", "compatible_reads", "estimated_reads",
                                        "read_fraction", "abundance"}
    narrow = pa.get_abundance(bootstraps=20, seed=3, confidence=0.5)["genomes"]  # (sorted[5] .. sorted[14])
    assert all(n["abundance_lo"] >= w["abundance_lo"] and n["abundance_hi"] <= w["abundance_hi"]
               for n, w in zip(narrow, a["genomes"]))
    for bad in (dict(bootstraps=-1), dict(bootstraps=10001), dict(bootstraps=True), dict(bootstraps=5, seed=-1),
                dict(bootstraps=5, seed=2 ** 64), dict(bootstraps=5, confidence=1.0),
                dict(bootstraps=5, confidence=0.0)):
        with pytest.raises(ValueError):
            pa.get_abundance(**bad)
