"""Paired-end reads on the GPU (pa_align_pairs, N.align_pairs,
PseudoAlignment.align_pairs_from_containers, main.py --reads2; DESIGN.md
section 15).

Every comparison is exact equality with the model of tests/test_pairs_host.py
(plain Python from the section's rules, checked there and again here against
the unchanged CPU oracle): type, list with its order, filtered_kmers,
redundant_kmers, list offsets; with a result the six statistics, unique,
ambiguous and first_key.  Every case runs on a forward and on a both-strand
index, with the combine rules (PA_PAIR_COMBINE unset) and with every pair sent
to the pair-exact kernel (PA_PAIR_COMBINE=0).
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pa_native as N
import test_pairs_host as M

pytestmark = pytest.mark.gpu

MAIN = M.MAIN


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X (no CPU fallback exists)")


@pytest.fixture(params=[None, "0"], ids=["combine", "exact_only"])
def combine(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("PA_PAIR_COMBINE", raising=False)
    else:
        monkeypatch.setenv("PA_PAIR_COMBINE", request.param)
    return request.param is None


def params(ps):
    return N.Params.make(ps.get("m", 1), ps.get("p", 1), ps.get("mrq"), ps.get("mkq"), ps.get("mg"))


def upload(pairs):
    """The two Reads of [(mate1, q1, mate2, q2)]."""
    out = []
    for s, q in ((0, 1), (2, 3)):
        seq, off = N.concat([pr[s] for pr in pairs])
        qual, _ = N.concat([pr[q] for pr in pairs])
        out.append(N.Reads.upload(seq, qual, off))
    return out


def flat(results):
    """(types, qf, hr, list offsets, lists) of the model's results, as the device returns them."""
    off = np.zeros(len(results) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r[1]) for r in results])
    return ([r[0] for r in results], [r[2] for r in results], [r[3] for r in results], off.tolist(),
            [g for r in results for g in r[1]])


def check_pairs(index, m1, m2, prm, results, base=0, combine=True):
    """One align_pairs call with a fresh result against the model; returns exact_pairs."""
    G = index.n_genomes
    res = N.Result(index)
    types, qf, hr, off, lists, exact = N.align_pairs(index, m1, m2, prm, base, res)
    want = flat(results)
    for name, a, b in zip(("types", "filtered_kmers", "redundant_kmers", "list_off", "lists"),
                          (types, qf, hr, off, lists), want):
        a = np.asarray(a).tolist()
        bad = [i for i, (x, y) in enumerate(zip(a, b)) if x != y][:5]
        assert len(a) == len(b) and not bad, (name, len(a), len(b), bad, [a[i] for i in bad], [b[i] for i in bad])
    stats, uq, am, fk = res.fetch()
    ws, wu, wa, wf = M.accumulate(results, G, base)
    assert stats.tolist() == ws
    assert uq.tolist() == wu and am.tolist() == wa
    assert [int(x) for x in fk] == wf
    res.close()
    kept = sum(r[0] != M.DROPPED for r in results)
    if not combine:
        assert exact == kept
    else:
        assert exact <= kept
    return exact


# ---- 1. hand-built ---------------------------------------------------------------------------

@pytest.mark.parametrize("both", [False, True], ids=["forward", "both_strands"])
@pytest.mark.parametrize("k", M.HAND_KS)
def test_hand_built(k, both, combine):
    M.test_hand_built_model(k, both)  # the model's own check, and that every corner is what it is named for
    genomes, _, named = M.hand_case(k)
    pairs = [pr[1:] for pr in named]
    results = M.model_all(M.kmer_sets(genomes, both, k), k, pairs, **M.HAND_PS)
    index = N.Index(genomes, k, both_strands=both)
    m1, m2 = upload(pairs)
    exact = check_pairs(index, m1, m2, params(M.HAND_PS), results, base=77, combine=combine)
    if combine:
        # settled by the rules: a dropped mate, an unmapped mate (three pairs), both unmapped, both ambiguous
        # without a specific k-mer; "shared_kmers", "swapped" and the rest must reach the exact kernel
        assert exact == len(pairs) - 6
    for x in (m1, m2, index):
        x.close()


# ---- 2. random -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rand_world():
    world = {}
    yield world
    for x in world.values():
        for y in x:
            y.close()


def rand_device(world, k, both):
    if ("index", k, both) not in world:
        world[("index", k, both)] = (N.Index(M.rand_genomes(), k, both_strands=both),)
    if ("reads", k) not in world:
        world[("reads", k)] = tuple(upload(M.rand_pairs(k)))
    return world[("index", k, both)][0], world[("reads", k)]


@pytest.mark.parametrize("both", [False, True], ids=["forward", "both_strands"])
@pytest.mark.parametrize("k", sorted(M.RAND_SHAPES))
def test_random_vs_model(k, both, combine, rand_world):
    M.rand_conditions(k, both)
    index, (m1, m2) = rand_device(rand_world, k, both)
    for i, ps in enumerate(M.RAND_PS):
        results, o1, o2 = M.rand_model(k, both, i)
        exact = check_pairs(index, m1, m2, params(ps), results, base=1000 * i, combine=combine)
        if combine:
            # the foreign-mate pairs are settled by the unmapped-mate rule whatever the lane kernels do;
            # the pairs whose two mates each hold specific k-mers must reach the exact kernel
            assert 0 < exact < len(results), (ps, exact)
            both_specific = sum(o1.types[j] != M.DROPPED and o2.types[j] != M.DROPPED
                                and len(o1.genomes_of(j)) >= 1 and len(o2.genomes_of(j)) >= 1
                                for j in range(len(results)))
            assert exact >= both_specific > 0, (ps, exact, both_specific)


# ---- 3. batching and accumulation ------------------------------------------------------------

@pytest.mark.parametrize("both", [False, True], ids=["forward", "both_strands"])
def test_batches_accumulate(both, combine, rand_world):
    k, ps = 31, M.RAND_PS[-1]
    pairs = M.rand_pairs(k)
    results, _, _ = M.rand_model(k, both, len(M.RAND_PS) - 1)
    index, (m1, m2) = rand_device(rand_world, k, both)
    prm = params(ps)
    base = 5000
    one = N.Result(index)
    N.align_pairs(index, m1, m2, prm, base, one)
    acc = N.Result(index)
    cuts = [0, 701, 1402, len(pairs)]
    for a, b in zip(cuts, cuts[1:]):
        p1, p2 = upload(pairs[a:b])
        types, _, _, _, _, _ = N.align_pairs(index, p1, p2, prm, base + a, acc)
        assert types.tolist() == [r[0] for r in results[a:b]]
        p1.close()
        p2.close()
    want = M.accumulate(results, index.n_genomes, base)
    for res in (one, acc):
        stats, uq, am, fk = res.fetch()
        assert (stats.tolist(), uq.tolist(), am.tolist(), [int(x) for x in fk]) == want
    # a call without room for the lists: PA_EINVAL, the total, the types and the offsets valid, acc unchanged
    total = sum(len(r[1]) for r in results)
    assert total > 0
    st, types, _, _, off, _, got_total, _ = N.align_pairs_call(index, m1, m2, prm, 0, base, acc)
    assert st == N.PA_EINVAL
    assert got_total == total
    assert types.tolist() == [r[0] for r in results]
    assert off.tolist() == np.cumsum([0] + [len(r[1]) for r in results]).tolist()
    stats, uq, am, fk = acc.fetch()
    assert (stats.tolist(), uq.tolist(), am.tolist(), [int(x) for x in fk]) == want
    # the counters alone: no per-pair output wanted
    only = N.Result(index)
    N.align_pairs(index, m1, m2, prm, base, only, lists=False)
    stats, uq, am, fk = only.fetch()
    assert (stats.tolist(), uq.tolist(), am.tolist(), [int(x) for x in fk]) == want
    for x in (one, acc, only):
        x.close()


def test_argument_errors(rand_world):
    index, (m1, m2) = rand_device(rand_world, 31, False)
    p1, p2 = upload(M.rand_pairs(31)[:10])
    prm = params({})
    st = N.align_pairs_call(index, m1, p2, prm, 100)[0]
    assert st == N.PA_EINVAL and b"different numbers of reads" in N.lib().pa_last_error()
    for x in (p1, p2):
        x.close()


# ---- 4. Python and CLI -----------------------------------------------------------------------

def file_case(k):
    """hand_case without the pair that holds an N (the FASTQ grammar admits ACGT only)."""
    genomes, names, named = M.hand_case(k)
    return genomes, names, [pr for pr in named if "N" not in pr[1] + pr[3]]


def write_files(tmp_path, k, id_style):
    genomes, names, named = file_case(k)
    fa = tmp_path / "genomes.fa"
    fa.write_text("".join(f">{n}\n{g}\n" for n, g in zip(names, genomes)))
    suffix1, suffix2 = {"slash": ("/1", "/2"), "comment": (" 1:N:0", " 2:N:0")}[id_style]
    r1, r2 = tmp_path / "R1.fq", tmp_path / "R2.fq"
    r1.write_text("".join(f"@{n}{suffix1}\n{s1}\n+\n{q1}\n" for n, s1, q1, _, _ in named))
    r2.write_text("".join(f"@{n}{suffix2}\n{s2}\n+\n{q2}\n" for n, _, _, s2, q2 in named))
    return str(fa), str(r1), str(r2)


def run_main(argv, env=None):
    return subprocess.run([sys.executable, MAIN] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                          timeout=300, env=dict(os.environ, **(env or {})))


@pytest.mark.parametrize("both", [False, True], ids=["forward", "both_strands"])
def test_cli_pairs(tmp_path, both):
    k = 31
    genomes, names, named = file_case(k)
    fa, r1, r2 = write_files(tmp_path, k, "slash")
    results = M.model_all(M.kmer_sets(genomes, both, k), k, [pr[1:] for pr in named], **M.HAND_PS)
    want = M.summary_of(results, names, **M.HAND_PS)
    flags = ["-g", fa, "-k", str(k), "--reads", r1, "--reads2", r2, "--min-read-quality", "50"] + \
        (["--both-strands"] if both else [])
    out = tmp_path / "assignments.tsv"
    r = run_main(["-t", "dumpalign"] + flags + ["--assignments", str(out)])
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    assert got == want
    assert list(got["Summary"]) == list(want["Summary"])  # (the genomes in first-appearance order)
    lines = out.read_text().splitlines()
    assert lines[0].startswith("#")
    word = {M.UNIQUE: "unique", M.AMBIGUOUS: "ambiguous", M.UNMAPPED: "unmapped", M.DROPPED: "filtered"}
    assert len(lines) == 1 + len(named)
    for line, pr, res in zip(lines[1:], named, results):
        cols = line.split("\t")
        assert cols[0] == pr[0] and cols[1] == word[res[0]]
        assert [x for x in "\t".join(cols[2:]).replace(",", "\t").split("\t") if x] == [names[g] for g in res[1]]
    # task align (on a saved reference) writes the pairs' results; dumpalign -a prints the same JSON
    aln, kdb = tmp_path / "x.aln", tmp_path / "x.kdb"
    r = run_main(["-t", "reference", "-g", fa, "-k", str(k), "-r", str(kdb)] + (["--both-strands"] if both else []))
    assert r.returncode == 0, r.stderr
    r = run_main(["-t", "align", "-r", str(kdb), "-a", str(aln)] + flags[4:])
    assert r.returncode == 0, r.stderr
    r = run_main(["-t", "dumpalign", "-a", str(aln)])
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout) == want


def test_cli_pairs_errors(tmp_path):
    k = 31
    fa, r1, r2 = write_files(tmp_path, k, "comment")
    _, _, named = file_case(k)
    short = tmp_path / "short.fq"
    short.write_text("".join(f"@{n} 2:N:0\n{s2}\n+\n{q2}\n" for n, _, _, s2, q2 in named[:-1]))
    r = run_main(["-t", "dumpalign", "-g", fa, "-k", str(k), "--reads", r1, "--reads2", str(short)])
    assert r.returncode != 0 and r.stdout == ""
    assert r.stderr.startswith("Error: ") and "different numbers of records" in r.stderr
    other = tmp_path / "other.fq"
    other.write_text("".join(f"@{'zzz' if i == 3 else n} 2:N:0\n{s2}\n+\n{q2}\n"
                             for i, (n, _, _, s2, q2) in enumerate(named)))
    r = run_main(["-t", "dumpalign", "-g", fa, "-k", str(k), "--reads", r1, "--reads2", str(other)])
    assert r.returncode != 0 and r.stdout == ""
    assert r.stderr.startswith("Error: ") and named[3][0] in r.stderr and "zzz" in r.stderr


def test_python_api(tmp_path):
    from data_file import FASTAFile, FASTAQFile
    from kmer import AddingExistingRead, KmerReference, PseudoAlignment, ReadMappingType
    k = 31
    genomes, names, named = file_case(k)
    fa, r1, r2 = write_files(tmp_path, k, "comment")
    results = M.model_all(M.kmer_sets(genomes, False, k), k, [pr[1:] for pr in named], **M.HAND_PS)
    ref = KmerReference(k, FASTAFile(fa).container)
    c1, c2 = FASTAQFile(r1).container, FASTAQFile(r2).container
    al = PseudoAlignment(ref)
    al.align_pairs_from_containers(c1, c2, min_read_quality=50)
    assert al.get_summary() == M.summary_of(results, names, **M.HAND_PS)
    reads = al.reads
    assert list(reads) == [pr[0] for pr, res in zip(named, results) if res[0] != M.DROPPED]
    for pr, res in zip(named, results):
        if res[0] != M.DROPPED:
            assert set(reads[pr[0]]) == {"mapping_type", "genomes_mapped_to"}
            assert reads[pr[0]]["mapping_type"] == ReadMappingType(res[0])
            assert reads[pr[0]]["genomes_mapped_to"] == [names[g] for g in res[1]]
    with pytest.raises(AddingExistingRead):
        al.align_pairs_from_containers(c1, c2, min_read_quality=50)
    for flag in ("coverage", "pileup", "abundance"):
        with pytest.raises(ValueError):
            PseudoAlignment(ref, **{flag: True}).align_pairs_from_containers(c1, c2)
