"""No entry point leaks device buffers when an allocation fails, and a failure
the library tolerates does not change results.

libpa's test hook (csrc/pa_mem.cpp: pa_test_alloc_fail_at / _calls / _live)
makes the nth device allocation from now return out-of-memory without calling
HIP -- a simulated host-side error return, like PA_REDUCE_INJECT; no device
fault is involved.  For every entry point below the call is run once cleanly
(K allocation calls), then once per i = 1..K with allocation i failing, from
fresh handles each time.  Every such run ends in PA_ENOMEM (pa_native raises it
as MemoryError) or, where the allocation is optional by design (the build's
lpos, the Bloom filters, the neighbour words in one piece), in success with the
clean run's results.  After the handles of a run are closed the number of live
device buffers is back where it started; a last clean run shows that no cached
state was poisoned.

Against the commit before the scoped owners (with only the hook added) the
build and the align case failed and the align_reads case ended the process with
a segmentation fault: pa_assign.hip's A_HIP macro handed its `e_` to PA_HIP,
whose own local `e_` shadowed it (`hipError_t e_ = (e_)`), so a failed call could
fall through and the function went on with the buffers it had just freed.
"""

import tempfile

import numpy as np
import pytest

import pa_native as N
import synth

pytestmark = pytest.mark.gpu

K_MER = 31
UNMAPPED, UNIQUE, AMBIGUOUS = 1, 2, 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X (no CPU fallback exists)")


@pytest.fixture(scope="module")
def data():
    gens = synth.family_genomes(6, 3000, seed=11, family_size=3, sub_rate=0.01)
    seq, qual, _ = synth.sample_reads(gens, 300, 150, seed=12, err_rate=0.01)
    seq = np.array(seq, dtype=np.uint8)
    qual = np.array(qual, dtype=np.uint8)
    seq[::3] = synth.reverse_complement(seq[::3])  # every third read: the other strand
    qual[::3] = qual[::3, ::-1]
    off = np.arange(301, dtype=np.uint64) * 150
    kmers = ["".join(map(chr, gens[g][s:s + K_MER])) for g, s in ((0, 5), (2, 100), (3, 700), (5, 2000))]
    kmers = [k for k in kmers if set(k) <= set("ACGT")]
    return {"gens": gens, "seq": seq.reshape(-1), "qual": qual.reshape(-1), "off": off, "kmers": kmers}


def freeze(x):
    """A result as something == compares exactly."""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, dict):
        return tuple(sorted((k, freeze(v)) for k, v in x.items()))
    if isinstance(x, (tuple, list)):
        return tuple(freeze(v) for v in x)
    if hasattr(x, "_fields_"):  # a ctypes structure
        return tuple((f[0], int(getattr(x, f[0]))) for f in x._fields_)
    return x


class Case:
    """prep: fresh handles into h (not under the hook); call: the entry point
    under test; result: what it made, read after the hook is off."""

    def __init__(self, data):
        self.d = data
        self.prm = N.Params.make()

    def index(self, h, prepared=True):
        h["idx"] = N.Index(self.d["gens"], K_MER, device=0)
        if prepared:
            h["idx"].prepare(expected_reads=10 ** 9)

    def reads(self, h):
        h["reads"] = N.Reads.upload(self.d["seq"], self.d["qual"], self.d["off"], device=0)

    def prep(self, h):
        self.index(h)
        self.reads(h)

    def result(self, h):
        return h["out"]


class Build(Case):
    def prep(self, h):
        self.reads(h)

    def call(self, h):
        self.index(h)

    def result(self, h):  # the index as the counter pass sees it
        h["res"] = N.Result(h["idx"])
        N.align(h["idx"], h["reads"], self.prm, 0, h["res"])
        return (h["idx"].info().n_kmers, h["idx"].info().n_multi_classes, h["res"].fetch())


class PrepareCoverage(Case):
    def call(self, h):
        h["idx"].prepare_coverage()

    def result(self, h):
        return N.align_placements(h["idx"], h["reads"], self.prm)


class Align(Case):
    def prep(self, h):
        Case.prep(self, h)
        h["res"] = N.Result(h["idx"])

    def call(self, h):
        N.align(h["idx"], h["reads"], self.prm, 0, h["res"])

    def result(self, h):
        return h["res"].fetch()


class AlignReads(Case):
    def call(self, h):
        h["out"] = N.align_reads(h["idx"], h["reads"], self.prm)


class AlignPlacements(Case):
    def call(self, h):
        h["out"] = N.align_placements(h["idx"], h["reads"], self.prm)


class CoverageAdd(Case):
    def call(self, h):
        h["cov"] = N.Coverage(h["idx"])
        h["cov"].add(h["reads"], self.prm)
        h["out"] = h["cov"].summary(1)


class PileupAdd(Case):
    def call(self, h):
        h["pile"] = N.Pileup(h["idx"])
        h["pile"].add(h["reads"], self.prm)
        h["out"] = (h["pile"].variants(1, 1, 0), h["pile"].stats())


class AbundanceAdd(Case):
    def call(self, h):
        h["ab"] = N.Abundance(h["idx"])
        h["ab"].add(h["reads"], self.prm)
        h["out"] = h["ab"].estimate(50, 0.0)


class AlignCandidates(Case):
    def call(self, h):
        h["out"] = N.align_candidates(h["idx"], h["reads"], self.prm)


class Dumpref(Case):
    def call(self, h):
        G = len(self.d["gens"])
        with tempfile.TemporaryFile() as f:
            out = N.index_dumpref(h["idx"], None, np.arange(G, dtype=np.uint32), ['"g%d"' % g for g in range(G)],
                                  f.fileno(), threads=2)
            f.seek(0)
            h["out"] = (out, f.read())


class Reduce(Case):
    def call(self, h):
        h["idx"].reduce([0, 2, 3, 5])

    def result(self, h):  # (class ids depend on the build's layout, the sets they name do not)
        inf = h["idx"].info()
        cls, size = h["idx"].lookup(self.d["kmers"])
        sets = [tuple(h["idx"].class_genomes(int(c))) if c >= 0 else () for c in cls]
        return (inf.n_kmers, inf.n_genomes, size, sets)


class Positions(Case):
    def call(self, h):
        h["out"] = h["idx"].positions(self.d["kmers"], reverse=True)


CASES = [Build, PrepareCoverage, Align, AlignReads, AlignPlacements, CoverageAdd, PileupAdd, AbundanceAdd,
         AlignCandidates, Dumpref, Reduce, Positions]


def close_all(h):
    for name in ("cov", "pile", "ab", "res", "reads", "idx"):  # accumulators before their index
        if h.get(name) is not None:
            h[name].close()
    h.clear()


def run_once(case, fail_at):
    """(outcome, frozen results or None, allocation calls of the call): outcome
    "ok" or "nomem".  Everything the run made is closed before it returns."""
    h = {}
    try:
        case.prep(h)
        c0 = N.test_alloc_calls()
        N.test_alloc_fail_at(fail_at)
        try:
            case.call(h)
            outcome = "ok"
        except MemoryError:  # PA_ENOMEM; any other status or exception fails the test
            outcome = "nomem"
        finally:
            N.test_alloc_fail_at(0)
        made = N.test_alloc_calls() - c0
        res = freeze(case.result(h)) if outcome == "ok" else None
        return outcome, res, made
    finally:
        N.test_alloc_fail_at(0)
        close_all(h)


def sweep(case):
    live0 = N.test_alloc_live()
    outcome, clean, K = run_once(case, 0)
    assert outcome == "ok"
    assert N.test_alloc_live() == live0, "the clean run leaked"
    assert K >= 1
    n_nomem = 0
    leaks = []
    for i in range(1, K + 1):
        outcome, res, made = run_once(case, i)
        assert made >= i, f"allocation {i} of {K} was never reached: the call is not repeatable"
        if outcome == "ok":
            assert res == clean, f"a tolerated failure of allocation {i} changed the results"
        else:
            n_nomem += 1
        if N.test_alloc_live() != live0:
            leaks.append((i, N.test_alloc_live() - live0))
            live0 = N.test_alloc_live()  # (each leak reported once)
    print(f"{type(case).__name__}: K = {K}, PA_ENOMEM at {n_nomem}, leaks at {leaks}")
    assert not leaks, f"device buffers leaked when allocation i failed: (i, buffers) = {leaks}"
    assert n_nomem >= 1
    outcome, res, _ = run_once(case, 0)
    assert outcome == "ok" and res == clean, "a later clean run differs: cached state was poisoned"
    assert N.test_alloc_live() == live0


def test_reads_of_every_kind(data):
    """The batch holds unique, ambiguous and unmapped reads."""
    case = AlignReads(data)
    h = {}
    try:
        case.prep(h)
        types = N.align_reads(h["idx"], h["reads"], case.prm)[0]
    finally:
        close_all(h)
    for t in (UNMAPPED, UNIQUE, AMBIGUOUS):
        assert (types == t).sum() > 0, t


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_alloc_failure_sweep(data, case):
    sweep(case(data))


def test_alloc_failure_sweep_build_eager_rcnb(data, monkeypatch):
    """The build with the reverse-complement neighbour bits made at once
    (PA_RCNB_EAGER=1): the build-time Bloom filter is alive across build_rcnb."""
    monkeypatch.setenv("PA_RCNB_EAGER", "1")
    sweep(Build(data))
