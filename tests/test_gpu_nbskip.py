"""lane_walk_150 loads no neighbour word for a read that the bound settles
whatever the words hold (PA_LANE_NBSKIP): with
Xall the live windows that are unindexed genome windows plus the indexed ones
holding a mismatch, and ns the walked specific k-mers, ns >= Xall + max(m, 1).

Reads are built on the host from a k-mer table of the genomes (as
test_gpu_reanchor.py builds its cases): 150-bp stretches of genome 0 -- the
first of its family, so every k-mer of it has its first occurrence there and
the walk runs on it -- with ONE substitution, to a base no member of the
family has there, placed so that ns - Xall is exactly 0, 1, 2, 3 or 4; and the
same across an N run of the genome (the read holds A there), whose windows
are live and unindexed.  For a parameter set with t = max(m, 1) the reads with
ns - Xall = t - 1 lie one below the skip, t at it, t + 1 above it.  The counts
are asserted on the host, by a second, window-by-window computation, before
the GPU runs.

Results equal the CPU oracle's bit for bit (stats, unique, ambiguous, first
keys; nonzero read base; PA_LANE_GRID=1).  The diagnostic library (-DPA_STATS,
libpa_stats.so: __graft_entry__.build makes it) counts the words skipped: in a
child process that loads it, the counter is zero for the reads below, nonzero
for those at and above, and zero throughout under --max-genomes, whose
instantiations keep loading the words.
"""

import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import build_native
import pa_native as N
import pa_oracle as O
import synth

pytestmark = pytest.mark.gpu

K = 31
RLEN = 150
W = RLEN - K + 1
BASE = 777
FAM = 5
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = _i
PARAMS = {"default": dict(), "m0p0": dict(m=0, p=0), "m3": dict(m=3), "pneg": dict(p=-1), "mg2": dict(mg=2)}
DELTAS = (0, 1, 2, 3, 4)
# the substitution's offsets in the read: both ends, the first and last bases that 31 windows hold, the middle
E_ORDER = (0, 149, 30, 119, 31, 118, 1, 148, 15, 134, 45, 104, 60, 89, 75, 7, 142, 22, 127, 37, 112, 52, 97, 67, 82, 70)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X (no CPU fallback exists)")


def make_genomes():
    return synth.family_genomes(10, 30000, seed=311, family_size=FAM, sub_rate=0.01, conserved_len=500,
                                n_rate=2e-4, n_run=8)


# ---- host k-mer table (as in test_gpu_reanchor.py) ------------------------------

def kmer_codes(seq, k=K):
    c = CODE[np.asarray(seq, dtype=np.uint8)]
    n = c.shape[-1] - k + 1
    kc = np.zeros(c.shape[:-1] + (n,), dtype=np.uint64)
    bad = np.zeros(c.shape[:-1] + (n,), dtype=bool)
    for j in range(k):
        cj = c[..., j:j + n]
        bad |= cj == 255
        kc = (kc << np.uint64(2)) | (cj & 3).astype(np.uint64)
    return kc, ~bad


def genome0_windows(gens):
    """Per window position of genome 0: indexed (no N), and specific -- its
    k-mer in no other genome and at no other position of genome 0."""
    kc0, ok0 = kmer_codes(gens[0])
    others = np.unique(np.concatenate([kmer_codes(g)[0][kmer_codes(g)[1]] for g in gens[1:]]))
    i = np.minimum(np.searchsorted(others, kc0), others.size - 1)
    shared = others[i] == kc0
    _, inv, cnt = np.unique(kc0, return_inverse=True, return_counts=True)
    once = cnt[inv] == 1
    return ok0, ok0 & ~shared & once, ok0 & ~once


def engineered_reads(gens):
    """{(delta, across an N run): [(read, start, e)]}, up to 24 per key, the
    substitution offsets e spread over the read."""
    g = gens[0]
    ok, spec, rep = genome0_windows(gens)
    cum = lambda a: np.concatenate([[0], np.cumsum(a.astype(np.int64))])  # noqa: E731
    c_ok, c_spec, c_rep = cum(ok), cum(spec), cum(rep)
    fam = np.stack(gens[:FAM])
    starts = np.arange(len(g) - RLEN + 1)
    nonidx = W - (c_ok[starts + W] - c_ok[starts])
    spec_all = c_spec[starts + W] - c_spec[starts]
    clean = (c_rep[starts + W] - c_rep[starts]) == 0      # (no k-mer that repeats in the genome: the walk's own test)
    out = {}
    rng = np.random.default_rng(7)
    for e in E_ORDER:
        lo, hi = max(0, e - K + 1), min(e, W - 1)
        valid_u = c_ok[starts + hi + 1] - c_ok[starts + lo]
        spec_u = c_spec[starts + hi + 1] - c_spec[starts + lo]
        delta = (spec_all - spec_u) - (nonidx + valid_u)
        base_ok = g[starts + e] != ord("N")
        for d in DELTAS:
            for across in (False, True):
                pick = np.flatnonzero((delta == d) & clean & base_ok & (valid_u >= 1) & ((nonidx > 0) == across))
                rng.shuffle(pick)
                for s in pick[:1]:
                    have = set(fam[:, s + e].tolist())
                    free = [b for b in ACGT.tolist() if b not in have]
                    if not free:
                        continue
                    r = g[s:s + RLEN].copy()
                    r[r == ord("N")] = ord("A")
                    r[e] = free[0]
                    lst = out.setdefault((d, across), [])
                    if len(lst) < 24:
                        lst.append((r, int(s), e))
    return out


def counts_by_window(gens, windows, read, s):
    """(ns, Xall, mismatching bases inside an indexed window) of a read against
    genome 0 at s, window by window (windows: genome0_windows)."""
    g = gens[0]
    ok, spec, _ = windows
    mis = [i for i in range(RLEN) if g[s + i] != ord("N") and read[i] != g[s + i]]
    ns = xall = 0
    for w in range(W):
        has = any(w <= i < w + K for i in mis)
        if not ok[s + w]:
            xall += 1
        elif has:
            xall += 1
        elif spec[s + w]:
            ns += 1
    counted = [i for i in mis if any(ok[s + w] for w in range(max(0, i - K + 1), min(i, W - 1) + 1))]
    return ns, xall, counted


def offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return off


@pytest.fixture(scope="module")
def world():
    gens = make_genomes()
    eng = engineered_reads(gens)
    # the engineered counts, checked before anything runs on the GPU
    windows = genome0_windows(gens)
    for (d, across), lst in eng.items():
        for r, s, e in lst:
            ns, xall, counted = counts_by_window(gens, windows, r, s)
            assert counted == [e] and ns - xall == d, (d, across, s, e, ns, xall, counted)
            assert bool((gens[0][s:s + RLEN] == ord("N")).any()) == across, (d, across, s)
    for d in DELTAS:
        assert len(eng.get((d, False), [])) >= 8, (d, {k: len(v) for k, v in eng.items()})
    for d in (0, 1, 2):
        assert len(eng.get((d, True), [])) >= 2, (d, {k: len(v) for k, v in eng.items()})
    batches = {}
    for (d, across), lst in eng.items():
        reads = [r for r, _, _ in lst]
        batches[f"{'nrun' if across else 'plain'}_d{d}"] = (np.concatenate(reads), offsets([RLEN] * len(reads)))
    nat, _, _ = synth.sample_reads(gens, 2000, RLEN, seed=340, err_rate=0.01)
    reads = [r for lst in eng.values() for r, _, _ in lst] + list(nat)
    batches["all"] = (np.concatenate(reads), offsets([RLEN] * len(reads)))
    return {"gens": gens, "batches": batches, "index": N.Index(gens, K), "oracle": O.OracleIndex(gens, K)}


def full_params(ps):
    return {"m": 1, "p": 1, "mg": None, **PARAMS[ps]}


@pytest.mark.parametrize("ps", list(PARAMS))
def test_results_equal_the_oracle(world, ps, monkeypatch):
    """Every engineered read and 2000 natural ones at 1 % in one batch."""
    monkeypatch.setenv("PA_LANE_GRID", "1")
    s, off = world["batches"]["all"]
    q = np.full(s.size, ord("I"), dtype=np.uint8)
    f = full_params(ps)
    o = world["oracle"].align(s.tobytes(), q.tobytes(), off, m=f["m"], p=f["p"], mrq=None, mkq=None, mg=f["mg"],
                              read_base=BASE, detail=False)
    res = N.Result(world["index"])
    N.align(world["index"], N.Reads.upload(s, q, off), N.Params.make(f["m"], f["p"], None, None, f["mg"]), BASE, res)
    stats, uq, am, fk = res.fetch()
    assert stats.tolist() == o.stats.tolist(), ps
    assert uq.tolist() == o.unique.tolist() and am.tolist() == o.ambiguous.tolist(), ps
    ofk = np.where(o.first_key == np.iinfo(np.uint64).max, N.NO_FIRST_KEY, o.first_key)
    assert fk.tolist() == ofk.tolist(), ps
    if ps in ("default", "pneg"):  # (one substitution off genome 0, ns > Xall: UNIQUE)
        assert int(o.stats[0]) >= sum(len(world["batches"][f"plain_d{d}"][1]) - 1 for d in (1, 2, 3, 4))


# ---- the counter of the diagnostic library --------------------------------------

CHILD = r"""
import json, sys
import numpy as np
import pa_native as N
d = np.load(sys.argv[1])
gens = [d["g%d" % i] for i in range(int(d["ng"]))]
index = N.Index(gens, int(d["k"]))
for ps in json.loads(sys.argv[2]):
    for name in json.loads(sys.argv[3]):
        s, off = d["s_" + name], d["off_" + name]
        q = np.full(s.size, ord("I"), dtype=np.uint8)
        res = N.Result(index)
        sys.stderr.write("[case] %s %s\n" % (ps["name"], name))
        sys.stderr.flush()
        N.align(index, N.Reads.upload(s, q, off), N.Params.make(ps["m"], ps["p"], None, None, ps["mg"]), int(d["base"]), res)
        res.fetch()
"""


def stats_library():
    """libpa_stats.so of this checkout (made by __graft_entry__.build; built
    here only if it is missing or stale)."""
    lib = os.path.join(os.path.dirname(os.path.abspath(build_native.__file__)), "libpa_stats.so")
    want = build_native.source_hash(stats=True)
    try:
        with open(lib + ".sha") as f:
            fresh = os.path.exists(lib) and f.read().strip() == want
    except OSError:
        fresh = False
    return lib if fresh else build_native.build(stats=True)


def test_skipped_word_counter(world, tmp_path):
    names = [n for n in world["batches"] if n != "all"]
    arrays = {"ng": len(world["gens"]), "k": K, "base": BASE}
    for i, g in enumerate(world["gens"]):
        arrays[f"g{i}"] = g
    for n in names:
        arrays["s_" + n], arrays["off_" + n] = world["batches"][n]
    path = str(tmp_path / "cases.npz")
    np.savez(path, **arrays)
    sets = [dict(name=ps, **full_params(ps)) for ps in PARAMS]
    pkg = os.path.dirname(os.path.abspath(build_native.__file__))
    env = dict(os.environ, PA_LIBRARY=stats_library(), PA_LANE_GRID="1", PYTHONNOUSERSITE="1",
               PYTHONPATH=os.pathsep.join([pkg] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    r = subprocess.run([sys.executable, "-c", CHILD, path, json.dumps(sets), json.dumps(names)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    skipped = {}
    case = None
    for line in r.stderr.splitlines():
        m = re.match(r"\[case\] (\S+) (\S+)", line)
        if m:
            case = (m.group(1), m.group(2))
        m = re.search(r"neighbour words skipped .* (\d+)$", line)
        if m and case:
            skipped[case] = skipped.get(case, 0) + int(m.group(1))
    assert len(skipped) == len(sets) * len(names), (len(skipped), r.stderr[-2000:])
    for ps in PARAMS:
        f = full_params(ps)
        t = max(f["m"], 1)
        for n in names:
            d = int(n.rsplit("_d", 1)[1])
            got = skipped[(ps, n)]
            reads = len(world["batches"][n][1]) - 1
            if f["mg"] is not None or d < t:
                assert got == 0, (ps, n, got)
            else:  # (one counted mismatch per read: at most one word each)
                assert 0 < got <= reads, (ps, n, got, reads)
