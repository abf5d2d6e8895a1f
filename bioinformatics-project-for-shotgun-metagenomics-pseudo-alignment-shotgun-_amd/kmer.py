"""K-mer reference and pseudo-alignment, backed by the MI355X engine (libpa.so).

Drop-in for the reference's src/kmer.py: same names, constructor arguments,
attributes, return values and exceptions.  What changes is where the work runs:

* ``KmerReference`` builds a device-resident open-addressing hash table of
  2-bit-packed k-mers and their genome sets (``pa_index_build``) instead of
  ``Dict[str, Dict[Record, Set[int]]]`` (src/kmer.py:113-150).
* ``PseudoAlignment.align_reads_from_container`` ships the reads column-wise to
  HBM and classifies all of them in one kernel pass (``pa_align``,
  src/kmer.py:482-620); only per-genome counters and filter statistics come
  back.  ``PseudoAlignment.reads`` (per-read mapping types and genome lists)
  is materialised on first access by the assign pass (``pa_align_reads``: the
  lane kernels write the reads they settle, the per-read kernel the rest).
* ``KmerReference.kmers`` -- positions included -- is an introspection view
  built on the host on first access; nothing on the align path reads it.
  ``KmerReference.get_summary`` (dumpref) is made on the device instead
  (``pa_index_dumpref``: k-mers in insertion order by a device sort, the JSON
  text streamed by host threads), so it scales to references whose dict the
  reference could not hold.
* ``.kdb`` / ``.aln`` files load through a restricted unpickler that admits
  only the classes such files hold -- this package's, or the reference's
  same-named ones, so files written by the reference load too.

Results (per-genome unique/ambiguous counts, filtered_* counters, the Summary
key order) are bit-exact to the reference; see DESIGN.md for the quirk list
this reproduces.  Known deviations: k above 255 raises PaUnsupported; argument
errors of a batch (TypeError / ValueError / AddingExistingRead) are raised
before any read of the batch is counted rather than at the offending read.
"""

from __future__ import annotations

import gzip
import json
import math
import os
import pickle
import weakref
import tempfile
from collections import defaultdict, namedtuple
from enum import Enum
from typing import Any, Dict, Iterator, List, Optional, Sequence, Set, Tuple, Union

import numpy as np

import constants
import pa_native as N
from lineage import ASSIGNMENTS_TAXON_HEADER, Lineages, LineageTree, lineage_report_rows, lineage_report_text
from records import FASTAQRecordContainer, FASTARecordContainer, Record

IGNORE_AMBIGUOUS_THRESHOLD = 0
M_THRESHOLD = 0
_NO_KEY = int(N.NO_FIRST_KEY)
_DROPPED = 0  # PA_DROPPED

# --assignments: one line per read, read id <TAB> mapping <TAB> genome identifiers joined by ","
ASSIGNMENTS_HEADER = "#read\tmapping\tgenomes\n"
_ASSIGNMENT_WORDS = {0: "filtered", 1: "unmapped", 2: "unique", 3: "ambiguous"}  # PA_DROPPED .. PA_AMBIGUOUSLY_MAPPED


def assignment_line(read_id: str, mapping_type: int, genomes: Sequence[str]) -> str:
    """A line of the assignments file.  ``mapping_type``: a PA_* code (a
    ReadMappingType's value, or 0 for a read dropped by --min-read-quality);
    ``genomes``: genomes_mapped_to in list order (a p-demoted list repeats its
    first genome), written only for unique and ambiguous reads."""
    word = _ASSIGNMENT_WORDS[int(mapping_type)]
    listed = ",".join(genomes) if int(mapping_type) >= 2 else ""
    return f"{read_id}\t{word}\t{listed}\n"


class NotValidatingUniqueMapping(Exception):
    def __init__(self, message: str) -> None:
        super().__init__(message)


class AddingExistingRead(Exception):
    def __init__(self, message: str) -> None:
        super().__init__(message)


class ReadMappingType(Enum):
    UNMAPPED = 1
    UNIQUELY_MAPPED = 2
    AMBIGUOUSLY_MAPPED = 3


class KmerSpecifity(Enum):
    SPECIFIC = 1
    UNSPECIFIC = 2


ReadKmer = namedtuple("ReadKmer", ["specifity", "references"])
ReadMapping = namedtuple("ReadMapping", ["type", "genomes_mapped_to"])


def extract_k_max_value_keys_from_dict(d: Dict[str, int], k: int) -> List[str]:
    if not isinstance(d, dict):
        raise ValueError("Input must be a dictionary.")
    return sorted(d, key=lambda x: d[x], reverse=True)[:k] if d else []


def extract_kmers_from_genome(k: int, genome: str) -> Iterator[Tuple[int, str]]:
    """All (position, k-mer) windows of ``genome`` (src/kmer.py:84-94).

    Host helper kept for API compatibility; the engine extracts windows on
    the GPU (2-bit rolling keys in the build, funnel shifts in the align)."""
    if k > len(genome) or k <= 0:
        return iter([])
    return ((i, genome[i:i + k]) for i in range(len(genome) - k + 1))


def reverse_complement(seq: str) -> str:
    return seq.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def _kmer_positions(genome: str, kmer: str) -> Set[int]:
    out, i = set(), genome.find(kmer)
    while i >= 0:
        out.add(i)
        i = genome.find(kmer, i + 1)
    return out


def _check_align_args(kmer_reference, m, p, mrq, mkq, mg, debug=False) -> Optional[Exception]:
    """The checks of Read.pseudo_align (src/kmer.py:501-510) as an exception, or None."""
    if not (isinstance(kmer_reference, KmerReference) and isinstance(m, int) and isinstance(p, int)
            and (mrq is None or isinstance(mrq, int)) and (mkq is None or isinstance(mkq, int))
            and (mg is None or isinstance(mg, int)) and isinstance(debug, bool)):
        return TypeError(f"Invalid types given to pseudo align: {type(kmer_reference)}, {type(p)}, {type(m)}, "
                         f"{type(debug)}")
    if m < M_THRESHOLD:
        return ValueError(f"m must be bigger than or equal to {M_THRESHOLD}")
    return None


def extsim_filter(index: N.Index, identifiers: Sequence[str], genome_lengths: Sequence[int],
                  similarity_threshold: float) -> Tuple[Set[str], Dict[str, Dict[str, Union[str, int, float]]]]:
    """EXTSIM greedy similar-genome filter (src/kmer.py:152-230) on a device index.

    Per-identifier statistics and pairwise intersections come from the GPU
    (``pa_index_extsim_stats``: distinct k-mers, specific k-mers, and shared
    k-mers of every pair of identifiers, src/kmer.py:152-177); the greedy pass
    is the reference's: genomes sorted ascending by (unique, total, length,
    order), each compared with the kept ones in keep order by the overlap
    coefficient |A & B| / min(|A|, |B|) (0 if min is 0) and dropped on the first
    score strictly above the threshold.  Returns (kept identifiers,
    similarity_info).  Duplicate identifiers form one group, later records
    overwriting the length/order of earlier ones, as in the reference."""
    gid: Dict[str, int] = {}
    group_of = [gid.setdefault(i, len(gid)) for i in identifiers]
    total, uniq, inter = index.extsim_stats(group_of, len(gid))
    stats: Dict[str, Dict[str, int]] = {}
    for order, (ident, glen) in enumerate(zip(identifiers, genome_lengths)):
        a = gid[ident]
        stats[ident] = {"unique_kmers": int(uniq[a]), "total_kmers": int(total[a]), "genome_length": int(glen),
                        "order": order}
    ordered = sorted(stats.items(), key=lambda x: (x[1]["unique_kmers"], x[1]["total_kmers"],
                                                   x[1]["genome_length"], x[1]["order"]))
    kept: List[str] = []
    info: Dict[str, Dict[str, Union[str, int, float]]] = {}
    for ident, st in ordered:
        a = gid[ident]
        similar_to = None
        for kid in kept:
            b = gid[kid]
            min_count = min(int(total[a]), int(total[b]))
            score = (int(inter[a, b]) / min_count) if min_count > 0 else 0
            if score > similarity_threshold:  # overlap coefficient, strict (src/kmer.py:206-208)
                similar_to = (kid, score)
                break
        base = {"unique_kmers": st["unique_kmers"], "total_kmers": st["total_kmers"],
                "genome_length": st["genome_length"]}
        if similar_to is None:
            info[ident] = {"kept": "yes", **base, "similar_to": "NA", "similarity_score": "NA"}
            kept.append(ident)
        else:
            info[ident] = {"kept": "no", **base, "similar_to": similar_to[0], "similarity_score": similar_to[1]}
    return set(kept), info


class _KdbUnpickler(pickle.Unpickler):
    """Loader of .kdb / .aln files (src/kmer.py:265-282, 671-699): only the
    classes such files hold are resolved -- this package's, whose module and
    class names are the reference's own (kmer.KmerReference, records.Record,
    ...), so a file written by the reference resolves to these classes and
    their __setstate__ converts its state.  Anything else is refused."""

    _OWN = {("kmer", n) for n in ("KmerReference", "PseudoAlignment", "ReadMappingType", "KmerSpecifity",
                                  "ReadMapping", "ReadKmer")} | {("records", "Record")}
    _LIB = {("numpy", "ndarray"), ("numpy", "dtype"), ("numpy.core.multiarray", "_reconstruct"),
            ("numpy._core.multiarray", "_reconstruct"), ("numpy.core.multiarray", "scalar"),
            ("numpy._core.multiarray", "scalar"), ("builtins", "set"), ("builtins", "frozenset"),
            ("collections", "defaultdict"), ("collections", "OrderedDict")}

    def find_class(self, module: str, name: str):
        if (module, name) in self._OWN:
            if module == "records":
                import records
                return getattr(records, name)
            return globals()[name]
        if (module, name) in self._LIB:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"{module}.{name} is not a class a .kdb / .aln file holds")


def _load_pickle(path: str):
    with gzip.open(path, "rb") as f:
        return _KdbUnpickler(f).load()


def _write_fd(fd: int, data: bytes) -> None:
    view = memoryview(data)
    while view:
        view = view[os.write(fd, view):]


class KmerReference:
    """Device-resident k-mer reference of a FASTA container (src/kmer.py:109-351)."""

    def __init__(self, k: int, fasta_record_container: FASTARecordContainer, filter_similar: bool = False,
                 similarity_threshold: float = 0.95, device: Optional[int] = None, *,
                 compact_table: bool = False, both_strands: bool = False) -> None:
        """compact_table (not in the reference): the k-mer table at 2 slots per
        genome window (PA_BUILD_COMPACT) -- for a job of few reads per genome
        base, as the CLI's dumpalign / align jobs are (main.create_reference).
        both_strands (not in the reference, whose --reverse-complement flag is
        parsed and never read): reads align against both strands -- a k-mer's
        genomes are its own and its reverse complement's (the merge of
        get_kmer_and_reverse_references), exactly as if every genome g were
        g + "N" + reverse_complement(g) (PA_BUILD_BOTH_STRANDS; about twice the
        device memory).  EXTSIM then compares those k-mer sets.  ``kmers``, the
        position lookups and the dumpref summary stay in forward coordinates."""
        if filter_similar and not (0 <= similarity_threshold <= 1):
            raise ValueError("similarity_threshold must be between 0 and 1")
        if not isinstance(k, int):
            raise TypeError(f"k must be an int, got {type(k)}")
        self.genomes: List[Record] = list(fasta_record_container)
        pg = getattr(fasta_record_container, "packed_genomes", None)
        self._packed = pg(self.genomes) if pg is not None else None  # (the parser's concatenated genomes)
        self._all_genomes: Optional[List[Record]] = None  # before EXTSIM dropped any (k-mer view order)
        self._ref_kmers: Optional[Dict[str, Dict[Record, Set[int]]]] = None  # the dict of a reference-written .kdb
        self.kmer_len: int = k
        self._device = N.default_device() if device is None else int(device)
        self._compact = bool(compact_table)
        self._both_strands = bool(both_strands)
        self._build()
        if filter_similar:
            self._filter_similar_genomes(similarity_threshold)

    # -- device index -------------------------------------------------------

    def _build(self) -> None:
        # the align-side view (tiles, neighbour bits) is made at the first align:
        # an index that EXTSIM then rebuilds from the kept genomes never needs it
        packed, self._packed = getattr(self, "_packed", None), None  # (only for the first build)
        self._index = N.Index(None if packed is not None else [g["genome"] for g in self.genomes], self.kmer_len,
                              device=self._device, defer_tiles=True, packed=packed,
                              compact=getattr(self, "_compact", False),
                              both_strands=getattr(self, "_both_strands", False))
        self._view: Optional[Dict[str, Dict[Record, Set[int]]]] = None

    @property
    def index(self) -> N.Index:
        return self._index

    @property
    def n_kmers(self) -> int:
        """Number of distinct k-mers (== len(self.kmers)).  For a both-strand
        reference it counts the distinct k-mers over both strands, and no longer
        equals len(self.kmers), which stays the forward k-mer database."""
        return self._index.n_kmers

    # -- EXTSIM (src/kmer.py:152-263) --------------------------------------

    def _filter_similar_genomes(self, similarity_threshold: float) -> None:
        keep, info = extsim_filter(self._index, [g.identifier for g in self.genomes],
                                   [len(g["genome"]) for g in self.genomes], similarity_threshold)
        if len(keep) != len({g.identifier for g in self.genomes}):
            sel = [i for i, g in enumerate(self.genomes) if g.identifier in keep]
            # pruning dropped genomes == building from the kept ones: in place,
            # from their codes already on the device (pa_index_reduce); the
            # genome lists change only once that succeeded
            self._index.reduce(sel)
            self._all_genomes = self.genomes
            self.genomes = [self.genomes[i] for i in sel]
            self._view = None
        self.similarity_info = info

    # -- persistence ----------------------------------------------------------

    def __getstate__(self):
        state = {k: v for k, v in self.__dict__.items() if k not in ("_index", "_view", "_packed")}
        return state

    def __setstate__(self, state):
        if "kmers" in state and "_device" not in state:
            # written by the reference (src/kmer.py:265-282): genomes (the kept
            # ones after EXTSIM), kmer_len, its kmers dict, similarity_info.  The
            # device index is built from the genomes; the dict stays the k-mer
            # view, since after EXTSIM its order comes from genomes the file no
            # longer holds.
            self.genomes = list(state["genomes"])
            self.kmer_len = state["kmer_len"]
            self._all_genomes = None
            self._device = N.default_device()
            if "similarity_info" in state:
                self.similarity_info = state["similarity_info"]
            self._both_strands = False  # (the reference looks up forward k-mers only)
            self._build()
            self._ref_kmers = state["kmers"]
            self._view = self._ref_kmers
            return
        self.__dict__.update(state)
        self.__dict__.setdefault("_ref_kmers", None)
        self.__dict__.setdefault("_both_strands", False)  # (a file from before the property: forward)
        self._build()
        if self._ref_kmers is not None:
            self._view = self._ref_kmers

    def save(self, ref_file: str) -> None:
        with gzip.open(ref_file, "wb") as f:
            pickle.dump(self, f)

    @classmethod
    def load(cls, ref_file: str) -> "KmerReference":
        return _load_pickle(ref_file)  # (any object, as pickle.load)

    # -- lookups ----------------------------------------------------------------

    @property
    def kmers(self) -> Dict[str, Dict[Record, Set[int]]]:
        """Introspection view ``{kmer: {Record: positions}}`` in the reference's
        insertion order (built on the host on first access; not used to align)."""
        if self._view is None:
            # After EXTSIM the reference deletes the dropped genomes' entries from
            # the full dict (src/kmer.py:232-245): the remaining k-mers keep the
            # order of the full build, so walk every original genome and keep
            # the kept ones' positions only.
            kept = None if self._all_genomes is None else {id(g) for g in self.genomes}
            view: Dict[str, Dict[Record, Set[int]]] = {}
            for rec in (self.genomes if kept is None else self._all_genomes):
                keep = kept is None or id(rec) in kept
                for pos, km in extract_kmers_from_genome(self.kmer_len, rec["genome"]):
                    if constants.NULL_NUCLEOTIDES_CHAR not in km:
                        entry = view.setdefault(km, {})
                        if keep:
                            entry.setdefault(rec, set()).add(pos)
            self._view = view if kept is None else {km: gs for km, gs in view.items() if gs}
        return self._view

    def _genome_set(self, kmer: str) -> List[int]:
        cls, _ = self._index.lookup([kmer])
        return [] if cls[0] < 0 else self._index.class_genomes(int(cls[0]))

    def _references(self, kmer: str, reverse: bool) -> Dict[Record, Set[int]]:
        """{genome record: positions} of the k-mer (and of its reverse complement)
        from the device index (pa_index_positions): genomes in FASTA order, the
        reverse complement's new genomes after the k-mer's own, as the
        reference's dict merge orders them (src/kmer.py:338-351)."""
        out: Dict[Record, Set[int]] = {}
        for q, g, p in self._index.positions([kmer], reverse).tolist():
            out.setdefault(self.genomes[g], set()).add(p)
        return out

    def _references_many(self, kmers: List[str]) -> List[Dict[Record, Set[int]]]:
        """get_kmer_references of every k-mer of the list: one device scan
        (pa_index_positions over the whole batch), hits split by query."""
        if self._view is not None:
            return [self._view.get(km, {}) for km in kmers]
        out: List[Dict[Record, Set[int]]] = [{} for _ in kmers]
        if kmers:
            for q, g, p in self._index.positions(kmers, False).tolist():
                out[q].setdefault(self.genomes[g], set()).add(p)
        return out

    def get_kmer_references(self, kmer: str) -> Dict[Record, Set[int]]:
        if self._view is not None:
            return self._view.get(kmer, {})
        return self._references(kmer, False)

    def __getitem__(self, kmer: str) -> Optional[Dict[Record, Set[int]]]:
        return self.get_kmer_references(kmer) or None

    def get_kmer_and_reverse_references(self, kmer: str) -> Dict[Record, Set[int]]:
        if self._view is None:
            return self._references(kmer, True)
        result: Dict[Record, Set[int]] = {g: set(p) for g, p in self.get_kmer_references(kmer).items()}
        rev = reverse_complement(kmer)
        if rev != kmer:
            for g, p in self.get_kmer_references(rev).items():
                result.setdefault(g, set()).update(p)
        return result

    # -- dumpref (src/kmer.py:300-329) ---------------------------------------------

    def write_summary(self, fd: int) -> None:
        """``json.dumps(self.get_summary(), indent=4)`` written to file descriptor
        ``fd`` (no final line break): the "Kmers" object streamed from the device
        index by pa_index_dumpref, then Summary (and Similarity) from its counts."""
        if self._ref_kmers is not None:  # a reference-written .kdb: its own dict is the k-mer order
            _write_fd(fd, json.dumps(self._summary_from_view(), indent=4).encode())
            return
        if self._all_genomes is None and not self._both_strands:
            index, genomes, keep, tmp = self._index, self.genomes, None, False
        elif self._all_genomes is None:
            # both strands: the dump is of the forward k-mer database, which the
            # index no longer is (pa_index_dumpref: PA_EUNSUPPORTED) -- dump a
            # forward index of the same genomes
            genomes, keep, tmp = self.genomes, None, True
            index = N.Index([g["genome"] for g in genomes], self.kmer_len, device=self._device, defer_tiles=True)
        else:
            # EXTSIM dropped genomes: the reference deletes their entries from the
            # full dict (src/kmer.py:232-245), so the k-mers keep the full
            # build's order -- dump an index of every original genome, masked
            genomes = self._all_genomes
            index = N.Index([g["genome"] for g in genomes], self.kmer_len, device=self._device, defer_tiles=True)
            kept = {id(g) for g in self.genomes}
            keep = np.fromiter((id(g) in kept for g in genomes), dtype=np.uint8, count=len(genomes))
            tmp = True
        descs: Dict[str, int] = {}
        desc_of = np.empty(len(genomes), dtype=np.uint32)
        for i, g in enumerate(genomes):
            desc_of[i] = descs.setdefault(g["description"], len(descs))
        names = list(descs)
        try:
            _write_fd(fd, b'{\n    "Kmers": ')
            uniq, multi, order, last, _ = N.index_dumpref(index, keep, desc_of, [json.dumps(d) for d in names], fd)
        finally:
            if tmp:
                index.close()
        present = sorted((d for d in range(len(names)) if int(order[d]) != N.NO_ORDER), key=lambda d: int(order[d]))
        summary = {names[d]: {"total_bases": len(genomes[int(last[d])]["genome"]), "unique_kmers": int(uniq[d]),
                              "multi_mapping_kmers": int(multi[d])} for d in present}
        tail: Dict[str, Any] = {"Kmers": 0, "Summary": summary}
        if hasattr(self, "similarity_info"):
            tail["Similarity"] = self.similarity_info
        text = json.dumps(tail, indent=4)
        _write_fd(fd, text[text.index('"Kmers": 0') + len('"Kmers": 0'):].encode())

    def get_summary(self) -> Dict[str, Any]:
        """dumpref summary (src/kmer.py:300-329): {"Kmers", "Summary"[, "Similarity"]}."""
        if self._ref_kmers is not None:
            return self._summary_from_view()
        with tempfile.TemporaryFile() as f:
            self.write_summary(f.fileno())
            f.seek(0)
            return json.loads(f.read())

    def _summary_from_view(self) -> Dict[str, Any]:
        """The same summary from the host view (a reference-written .kdb's dict)."""
        kmers = self.kmers
        details = {km: {g["description"]: sorted(p) for g, p in gs.items()} for km, gs in kmers.items()}
        summary: Dict[str, Dict[str, int]] = defaultdict(
            lambda: {"total_bases": 0, "unique_kmers": 0, "multi_mapping_kmers": 0})
        per_genome: Dict[str, Set[str]] = defaultdict(set)
        for km, gs in kmers.items():
            for g in gs:
                summary[g["description"]]["total_bases"] = len(g["genome"])
                per_genome[g["description"]].add(km)
        for desc, kms in per_genome.items():
            uniq = sum(1 for km in kms if len(kmers[km]) == 1)
            summary[desc]["unique_kmers"] = uniq
            summary[desc]["multi_mapping_kmers"] = len(kms) - uniq
        out = {"Kmers": details, "Summary": dict(summary)}
        if hasattr(self, "similarity_info"):
            out["Similarity"] = self.similarity_info
        return out


class Read:
    """One FASTQ read (src/kmer.py:357-526); pseudo_align runs on the GPU."""

    def __init__(self, fastaq_record: Record) -> None:
        self.identifier = fastaq_record.identifier
        self.mapping = ReadMapping(ReadMappingType.UNMAPPED, [])
        self.__raw_read: str = fastaq_record["sequence"]
        self.__quality_scores: str = fastaq_record["quality_sequence"]
        self.num_quality_filtered_kmers: int = 0
        self.num_redundant_kmers: int = 0
        self._kmers: Dict[str, ReadKmer] = {}
        self._kmer_args = None

    def __str__(self) -> str:
        rows = [f"Mapping: {self.mapping}"]
        for kmer, rk in self.kmers.items():
            rows += [f"k-mer: {kmer}", f"specifity: {rk.specifity}", "Genome References:"]
            rows += [f"\t{ref}" for ref in rk.references]
        return "\n".join(rows)

    __repr__ = __str__

    def mean_quality(self) -> float:
        return sum(map(ord, self.__quality_scores)) / len(self.__quality_scores)

    def kmer_quality(self, start: int, k: int) -> float:
        return sum(map(ord, self.__quality_scores[start:start + k])) / k

    @property
    def kmers(self) -> Dict[str, ReadKmer]:
        """The read's distinct indexed k-mers (src/kmer.py:410-429), from GPU lookups."""
        if self._kmer_args is not None:
            ref, mkq, mg = self._kmer_args
            self._kmer_args = None
            k = ref.kmer_len
            windows = list(extract_kmers_from_genome(k, self.__raw_read))
            cls, size = ref.index.lookup([w for _, w in windows]) if windows else ([], [])
            kept: Dict[str, int] = {}  # included k-mer -> its set size, first inclusion order
            for (start, km), c, s in zip(windows, cls, size):
                if mkq is not None and self.kmer_quality(start, k) < mkq:
                    continue
                if c < 0 or (mg is not None and int(s) > mg):
                    continue
                kept.setdefault(km, int(s))
            # every included k-mer's references from one batched device scan
            names = list(kept)
            for km, refs in zip(names, ref._references_many(names)):
                self._kmers[km] = ReadKmer(KmerSpecifity.SPECIFIC if kept[km] == 1 else KmerSpecifity.UNSPECIFIC, refs)
        return self._kmers

    def _packed(self):
        seq = np.frombuffer(self.__raw_read.encode("ascii", errors="replace"), dtype=np.uint8)
        qual = np.frombuffer(self.__quality_scores.encode("latin-1", errors="replace"), dtype=np.uint8)
        return seq, qual, np.array([0, seq.size], dtype=np.uint64)

    def pseudo_align(self, kmer_reference: KmerReference, m: int = 1, p: int = 1,
                     min_read_quality: Optional[int] = None, min_kmer_quality: Optional[int] = None,
                     max_genomes: Optional[int] = None, debug: bool = False) -> ReadMappingType:
        err = _check_align_args(kmer_reference, m, p, min_read_quality, min_kmer_quality, max_genomes, debug)
        if err is not None:
            raise err
        if min_read_quality is not None and self.mean_quality() < min_read_quality:
            return ReadMappingType.UNMAPPED
        seq, qual, off = self._packed()
        reads = N.Reads.upload(seq, qual, off, device=kmer_reference.index.device)
        prm = N.Params.make(m, p, None, min_kmer_quality, max_genomes)
        types, qf, hr, loff, lists = N.align_detail(kmer_reference.index, reads, prm)
        reads.close()
        self.num_quality_filtered_kmers += int(qf[0])
        self.num_redundant_kmers += int(hr[0])
        self._kmer_args = (kmer_reference, min_kmer_quality, max_genomes)
        t = ReadMappingType(int(types[0]))
        if t != ReadMappingType.UNMAPPED:
            self.mapping = ReadMapping(t, [kmer_reference.genomes[int(g)] for g in lists[loff[0]:loff[1]]])
        if debug:
            print(f"[DEBUG pseudo_align]: self.mapping: {self.mapping.type}, mapped to: {self.mapping}")
        return t


class _Batch:
    """A container batch aligned on the GPU, kept for lazy per-read results.
    ``all_dropped``: every read failed --min-read-quality on the host (no GPU
    pass was needed, see _align_columns)."""

    __slots__ = ("base", "ids", "seq", "qual", "off", "params", "mrq", "entries", "all_dropped", "_dropped",
                 "read_node")

    def __init__(self, base, ids, seq, qual, off, params, mrq, all_dropped=False):
        self.base, self.ids, self.seq, self.qual, self.off, self.params = base, ids, seq, qual, off, params
        self.mrq, self.all_dropped, self.entries, self._dropped = mrq, all_dropped, None, None
        self.read_node = None  # (lineages: every read's node, uint32, N.NO_NODE for none; 4 B per read)

    def load(self) -> None:
        pass

    def dropped(self) -> Optional[np.ndarray]:
        """Reads dropped by --min-read-quality (not in PseudoAlignment.reads), or None if none can be."""
        self.load()
        if self.all_dropped:
            return np.ones(len(self.ids), dtype=bool)
        if self.mrq is None:
            return None
        if self._dropped is None:
            self._dropped = _dropped_mask(self.qual, self.off, self.mrq)
        return self._dropped


    def results(self, index: N.Index):
        """(types, list offsets, lists) per read of the batch, from the device."""
        reads = N.Reads.upload(self.seq, self.qual, self.off, device=index.device)
        try:
            types, _, _, loff, lists = N.align_reads(index, reads, self.params)
        finally:
            reads.close()
        return types, loff, lists


class _PairBatch(_Batch):
    """A batch of pairs (align_pairs_from_containers): the columns of both mates,
    ``ids`` the pair identifiers; its per-pair results come from N.align_pairs."""

    __slots__ = ("seq2", "qual2", "off2")

    def __init__(self, base, ids, mate1, mate2, params, mrq, all_dropped=False):
        super().__init__(base, ids, mate1[0], mate1[1], mate1[2], params, mrq, all_dropped)
        self.seq2, self.qual2, self.off2 = mate2

    def dropped(self) -> Optional[np.ndarray]:
        """Pairs dropped by --min-read-quality: either mate fails it."""
        if self.all_dropped:
            return np.ones(len(self.ids), dtype=bool)
        if self.mrq is None:
            return None
        if self._dropped is None:
            self._dropped = _dropped_mask(self.qual, self.off, self.mrq) | _dropped_mask(self.qual2, self.off2,
                                                                                         self.mrq)
        return self._dropped

    def results(self, index: N.Index):
        m1 = N.Reads.upload(self.seq, self.qual, self.off, device=index.device)
        m2 = N.Reads.upload(self.seq2, self.qual2, self.off2, device=index.device)
        try:
            types, _, _, loff, lists, _ = N.align_pairs(index, m1, m2, self.params)
        finally:
            m1.close()
            m2.close()
        return types, loff, lists


def pair_identifier(id1: str, id2: str) -> str:
    """The identifier of the pair whose mates' FASTQ ids are ``id1`` and ``id2``:
    each id is cut at its first whitespace, a trailing ``/1`` is removed from
    mate 1's and a trailing ``/2`` from mate 2's; the two must then be equal."""
    a = id1.split(None, 1)[0] if id1.strip() else ""
    b = id2.split(None, 1)[0] if id2.strip() else ""
    if a.endswith("/1"):
        a = a[:-2]
    if b.endswith("/2"):
        b = b[:-2]
    if a != b:
        raise ValueError(f"The identifiers of a pair's mates differ: {id1!r} and {id2!r}")
    return a


class _FileBatch(_Batch):
    """A FASTQ file aligned by pa_align_fastq_file: its columns (ids, bases,
    qualities) are parsed from the file only when per-read results or ids are
    asked for."""

    __slots__ = ("path", "n", "trim", "device")

    def __init__(self, base, path, params, mrq, n, trim=None, device=None):
        super().__init__(base, None, None, None, None, params, mrq)
        self.path, self.n, self.trim, self.device = path, n, trim, device

    def load(self) -> None:
        if self.ids is None:
            from data_file import FASTAQFile
            ids, seq, qual, off = _columnar(FASTAQFile(self.path).container)
            if self.trim is not None:  # (the stream aligned the trimmed reads; its statistics are counted already)
                seq, qual, off = _trim_on_device(seq, qual, off, self.trim, None, self.device)
            self.ids, self.seq, self.qual, self.off = ids, seq, qual, off


EXTRACT_MAPPING_WORDS = {"filtered": 0, "unmapped": 1, "unique": 2, "ambiguous": 3}  # (word -> PA_* type value)


def extract_type_mask(mapping) -> int:
    """The pa_extract_spec type_mask of a selection given as --assignments'
    words: a comma-separated string (--extract-mapping) or a sequence of words.
    ValueError for an empty list, an empty word or an unknown one."""
    words = mapping.split(",") if isinstance(mapping, str) else list(mapping)
    if not words:
        raise ValueError("The extract mapping list is empty (choose from unique, ambiguous, unmapped, filtered)")
    mask = 0
    for w in words:
        w = w.strip() if isinstance(w, str) else w
        if w not in EXTRACT_MAPPING_WORDS:
            raise ValueError(f"Unknown extract mapping {w!r} (choose from unique, ambiguous, unmapped, filtered)")
        mask |= 1 << EXTRACT_MAPPING_WORDS[w]
    return mask


def _trim_on_device(seq, qual, off, spec: "N.TrimSpec", stats: Optional["N.TrimStats"], device, keep: bool = False):
    """The columns of a batch trimmed by pa_reads_trim:
    uploaded, trimmed on the device, downloaded.  ``stats`` accumulates.
    ``keep``: the trimmed device batch is returned as a fourth value instead
    of being freed (the caller aligns it and closes it)."""
    reads = N.Reads.upload(seq, qual, off, device=device)
    try:
        out, _, _, _ = reads.trim(spec, stats=stats)
    finally:
        reads.close()
    try:
        cols = out.download()
    except BaseException:
        out.close()
        raise
    if keep:
        return cols + (out,)
    out.close()
    return cols


def _native_trim(spec) -> Optional["N.TrimSpec"]:
    """A trim argument (a trim.Spec, an N.TrimSpec or None) as the N.TrimSpec
    to apply, or None when it trims nothing."""
    if spec is None:
        return None
    if not isinstance(spec, N.TrimSpec):
        if not hasattr(spec, "native"):
            raise ValueError("trim must be a trim.Spec or a pa_native.TrimSpec")
        spec = spec.native()
    return spec if spec.active else None


def _dropped_mask(qual: np.ndarray, off: np.ndarray, mrq) -> np.ndarray:
    """Read.mean_quality() < min_read_quality per read (src/kmer.py:394-399, 587),
    raw ASCII: an exact integer test for an int threshold, the reference's own
    float division (IEEE double, as numpy's) otherwise."""
    off = np.asarray(off, dtype=np.int64)
    lens = np.diff(off)
    n = lens.size
    sums = np.zeros(n, dtype=np.int64)
    if qual.size and n:
        nz = lens > 0
        sums[nz] = np.add.reduceat(qual.astype(np.int64), off[:-1][nz])
    if isinstance(mrq, int):
        return sums < int(mrq) * lens
    with np.errstate(divide="ignore", invalid="ignore"):
        return (sums / lens) < float(mrq)


def _columnar(container) -> Tuple[List[str], np.ndarray, np.ndarray, np.ndarray]:
    if isinstance(container, FASTAQRecordContainer):
        return container.id_sequence(), container.seq, container.qual, container.offsets
    ids, seqs, quals = [], [], []
    for rec in container:
        ids.append(rec.identifier)
        seqs.append(rec["sequence"])
        quals.append(rec["quality_sequence"])
    seq, off = N.concat(seqs)
    qual, _ = N.concat(quals)
    return ids, seq, qual, off


# Depth accumulators of the alignments made with coverage=True.  Device state,
# kept out of the instances' __dict__: an .aln file holds no coverage, and an
# alignment loaded from one has none.
_COVERAGE: "weakref.WeakKeyDictionary[PseudoAlignment, Optional[N.Coverage]]" = weakref.WeakKeyDictionary()


# Base-count accumulators of the alignments made with pileup=True, kept like
# _COVERAGE and for the same reason: [accumulator or None, min_base_quality].
_PILEUP: "weakref.WeakKeyDictionary[PseudoAlignment, list]" = weakref.WeakKeyDictionary()

# Abundance accumulators of the alignments made with abundance=True, kept like
# _COVERAGE and for the same reason.
_ABUNDANCE: "weakref.WeakKeyDictionary[PseudoAlignment, Optional[N.Abundance]]" = weakref.WeakKeyDictionary()

# Lineage state of the alignments made with lineages=..., kept like _COVERAGE and
# for the same reason: [Lineages, tree or None, accumulator or None, reads of
# batches dropped whole on the host].  The tree and the accumulator are made
# with the first batch (or the first report), from the index's genomes.
_LINEAGE: "weakref.WeakKeyDictionary[PseudoAlignment, list]" = weakref.WeakKeyDictionary()

# Containment accumulators of the alignments made with containment=True, kept
# like _COVERAGE and for the same reason: [accumulator or None, reads of batches
# dropped whole on the host].
_CONTAINMENT: "weakref.WeakKeyDictionary[PseudoAlignment, list]" = weakref.WeakKeyDictionary()

# Trim state of the alignments made with trim=..., kept like _COVERAGE (an .aln
# file holds per-read results only): [mate 1's N.TrimSpec or None, mate 2's,
# mate 1's N.TrimStats, mate 2's].
_TRIM: "weakref.WeakKeyDictionary[PseudoAlignment, list]" = weakref.WeakKeyDictionary()

CONTAINMENT_HEADER = ("#genome\tlength\tkmers\tkmers_seen\tcontainment\tidentity\tspecific_kmers\tspecific_seen"
                      "\tspecific_containment\tspecific_hits\tduplication\n")
CONTAINMENT_INFO = ("reads", "reads_dropped", "windows", "windows_retained", "windows_filtered_quality",
                    "windows_filtered_hr", "windows_absent")


def containment_ratios(k, kmers, kmers_seen, specific, specific_seen, hits_specific):
    """(containment, specific_containment, duplication, identity) of one genome or
    node: kmers_seen / kmers, specific_seen / specific, hits_specific /
    specific_seen and containment ** (1 / k), each 0 when its denominator is 0."""
    c = int(kmers_seen) / int(kmers) if int(kmers) else 0.0
    sc = int(specific_seen) / int(specific) if int(specific) else 0.0
    d = int(hits_specific) / int(specific_seen) if int(specific_seen) else 0.0
    return c, sc, d, (c ** (1.0 / k) if k else 0.0)


def containment_text(rows, info) -> str:
    """The --containment file: CONTAINMENT_HEADER, one tab-separated line per row
    of get_containment's "genomes" (floats as format(x, ".9g")) and a last
    comment line with the reads and the windows' counters."""
    def f(x) -> str:
        return format(float(x), ".9g")
    lines = [CONTAINMENT_HEADER]
    for r in rows:
        lines.append("\t".join((str(r["genome"]), str(int(r["length"])), str(int(r["kmers"])),
                                str(int(r["kmers_seen"])), f(r["containment"]), f(r["identity"]),
                                str(int(r["specific_kmers"])), str(int(r["specific_seen"])),
                                f(r["specific_containment"]), str(int(r["specific_hits"])),
                                f(r["duplication"]))) + "\n")
    lines.append(f"#reads\t{int(info['reads'])}\tdropped\t{int(info['reads_dropped'])}"
                 f"\twindows\t{int(info['windows'])}\tretained\t{int(info['windows_retained'])}"
                 f"\tfiltered_quality\t{int(info['windows_filtered_quality'])}"
                 f"\tfiltered_hr\t{int(info['windows_filtered_hr'])}\tabsent\t{int(info['windows_absent'])}\n")
    return "".join(lines)

ABUNDANCE_HEADER = "#genome\tlength\tunique_reads\tcompatible_reads\testimated_reads\tread_fraction\tabundance\n"


ABUNDANCE_BOOTSTRAP_COLUMNS = ("abundance_mean", "abundance_sd", "abundance_lo", "abundance_hi")


def confidence_permille(confidence) -> int:
    """The per-mille integer of a confidence level, round(1000 * confidence),
    converted once as variant_permille converts its fraction, so the quantile
    index below is integer arithmetic.  ValueError outside 1 .. 999."""
    if isinstance(confidence, bool) or not isinstance(confidence, (int, float)) or confidence != confidence:
        raise ValueError("confidence must be a number with round(1000 * confidence) in 1 .. 999")
    c = int(round(1000 * confidence))
    if not 1 <= c <= 999:
        raise ValueError("confidence must be a number with round(1000 * confidence) in 1 .. 999")
    return c


def bootstrap_summary(matrix, confidence):
    """Per genome (column) of a replicates x genomes matrix: (mean, sd, lo, hi).
    mean: the sum over the replicates in replicate order, divided by B; sd: the
    sample standard deviation (ddof = 1; 0 for B = 1); lo and hi: the percentile
    interval, sorted[j] and sorted[B - 1 - j] with j = ((1000 - c) * B) // 2000
    and c = confidence_permille(confidence)."""
    c = confidence_permille(confidence)
    m = np.asarray(matrix, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] < 1:
        raise ValueError("matrix must be replicates x genomes with at least one replicate")
    B = m.shape[0]
    j = ((1000 - c) * B) // 2000
    out = []
    for g in range(m.shape[1]):
        col = [float(x) for x in m[:, g]]
        total = 0.0
        for x in col:
            total += x
        mean = total / B
        ss = 0.0
        for x in col:
            ss += (x - mean) * (x - mean)
        sd = math.sqrt(ss / (B - 1)) if B > 1 else 0.0
        s = sorted(col)
        out.append((mean, sd, s[j], s[B - 1 - j]))
    return out


def abundance_text(names, lengths, unique_reads, compatible_reads, read_fraction, abundance, n_reads, iterations,
                   last_delta, n_classes, bootstrap=None) -> str:
    """The --abundance file: ABUNDANCE_HEADER, one tab-separated line per genome
    (estimated_reads = read_fraction * n_reads; floats as format(x, ".9g")) and a
    last comment line with the EM's iterations, its last delta and the classes.
    With ``bootstrap`` = (per-genome (mean, sd, lo, hi), bootstraps, seed,
    confidence) the header and the lines gain ABUNDANCE_BOOTSTRAP_COLUMNS and the
    last line the three settings."""
    def f(x) -> str:
        return format(float(x), ".9g")
    header, last = ABUNDANCE_HEADER, ""
    if bootstrap is not None:
        summary, bootstraps, seed, confidence = bootstrap
        header = ABUNDANCE_HEADER[:-1] + "".join("\t" + c for c in ABUNDANCE_BOOTSTRAP_COLUMNS) + "\n"
        last = f"\tbootstraps\t{int(bootstraps)}\tseed\t{int(seed)}\tconfidence\t{f(confidence)}"
    lines = [header]
    for g, name in enumerate(names):
        cols = (str(name), str(int(lengths[g])), str(int(unique_reads[g])),
                str(int(compatible_reads[g])), f(float(read_fraction[g]) * n_reads),
                f(read_fraction[g]), f(abundance[g]))
        if bootstrap is not None:
            cols += tuple(f(x) for x in summary[g])
        lines.append("\t".join(cols) + "\n")
    lines.append(f"#iterations\t{int(iterations)}\tlast_delta\t{f(last_delta)}\tclasses\t{int(n_classes)}{last}\n")
    return "".join(lines)


VARIANTS_HEADER = "#genome\tposition\tref\talt\tdepth\talt_count\tA\tC\tG\tT\n"


def variant_permille(min_alt_fraction) -> int:
    """The per-mille integer the device's calling rule uses for a fraction:
    round(1000 * f), converted once, so the rule itself stays integer
    (1000 * alt_count >= permille * depth)."""
    if isinstance(min_alt_fraction, bool) or not isinstance(min_alt_fraction, (int, float)) \
            or not 0 <= min_alt_fraction <= 1:
        raise ValueError("min_alt_fraction must be a number in 0 .. 1")
    return int(round(1000 * min_alt_fraction))


class PseudoAlignment:
    """Pseudo-alignment of reads against a KmerReference (src/kmer.py:532-699).

    ``coverage=True`` (not in the reference, which leaves its EXTCOVERAGE
    extension out): every batch aligned through the host-parsed path is also
    placed on the genomes it maps to, and ``get_coverage`` reports the depth
    and breadth per genome.

    ``pileup=True`` (not in the reference either): the bases of every uniquely
    mapped read of those batches are counted per genome position -- those of
    quality byte >= ``min_base_quality`` when given -- and ``get_variants`` /
    ``write_variants`` report the positions where the sample differs from the
    reference.

    ``abundance=True`` (not in the reference either): every read of those batches
    is counted in its compatibility class, and ``get_abundance`` /
    ``write_abundance`` report an EM estimate of the genomes' shares of the
    sample.

    ``lineages=Lineages(...)`` (not in the reference either): every read of those
    batches gets a node of the genomes' taxonomy tree -- its genome's node, or
    the lowest common ancestor of its compatibility set -- and
    ``get_lineage_report`` / ``write_lineage_report`` report the reads per node
    and clade; ``write_assignments`` gains a ``taxon`` column.

    ``containment=True`` (not in the reference either): every retained window of
    those batches marks its k-mer of the index, and ``get_containment`` /
    ``write_containment`` report, per genome, how many of its distinct k-mers
    the reads hold; with ``lineages`` the lineage report gains the same per
    clade.

    ``trim=spec`` (not in the reference either; a ``trim.Spec``): every read is
    trimmed on the device before anything else sees it -- quality ends, then a
    3' adapter -- and ``reads``, the counters and every accumulator are those of
    the trimmed reads; ``trim2`` is the spec of the second mates of a paired job
    (default: ``trim``); ``get_trim_stats`` reports what was cut (DESIGN.md
    section 22)."""

    def __init__(self, kmer_reference: KmerReference, coverage: bool = False, pileup: bool = False,
                 min_base_quality: Optional[int] = None, abundance: bool = False,
                 lineages: Optional[Lineages] = None, containment: bool = False, trim=None, trim2=None) -> None:
        t1 = _native_trim(trim)
        t2 = t1 if trim2 is None else _native_trim(trim2)
        if t1 is not None or t2 is not None:
            _TRIM[self] = [t1, t2, N.TrimStats(), N.TrimStats()]
        if containment:
            _CONTAINMENT[self] = [None, 0]  # (the accumulator is made with the first batch)
        if lineages is not None:
            if not isinstance(lineages, Lineages):
                raise ValueError("lineages must be a Lineages")
            _LINEAGE[self] = [lineages, None, None, 0]
        if abundance:
            _ABUNDANCE[self] = None  # (the accumulator is made with the first batch)
        if coverage:
            _COVERAGE[self] = None  # (the accumulator is made with the first batch)
        if min_base_quality is not None and (isinstance(min_base_quality, bool)
                                             or not isinstance(min_base_quality, int) or min_base_quality < 0):
            raise ValueError("min_base_quality must be a non-negative integer")
        if pileup:
            _PILEUP[self] = [None, min(min_base_quality or 0, 256)]
        self.kmer_reference: KmerReference = kmer_reference
        self.filtered_quality_reads: int = 0
        self.filtered_quality_kmers: int = 0
        self.filtered_hr_kmers: int = 0
        self.filter_read_quality_flag: bool = False
        self.filter_kmer_quality_flag: bool = False
        self.filter_max_genomes_flag: bool = False
        self._next_index = 0
        self._result: Optional[N.Result] = None
        self._gpu_stats = np.zeros(6, dtype=np.uint64)
        self._batches: List[_Batch] = []
        self._host: List[Tuple[int, str, Dict[str, Any]]] = []  # (index, id, entry) of add_read()
        self._ids: Optional[Set[str]] = None

    # -- bookkeeping ------------------------------------------------------------

    def _known_ids(self) -> Set[str]:
        """Identifiers already in ``reads`` (src/kmer.py:557): reads dropped by
        --min-read-quality never entered it."""
        if self._ids is None:
            ids: Set[str] = set()
            for b in self._batches:
                d = b.dropped()  # (loads a file batch's columns)
                ids.update(b.ids if d is None else (i for i, x in zip(b.ids, d) if not x))
            ids.update(i for _, i, _ in self._host)
            self._ids = ids
        return self._ids

    def _add_ids(self, ids: Sequence[str], dropped: Optional[np.ndarray], unique_batch: bool) -> None:
        """AddingExistingRead for an identifier already aligned -- before or
        earlier in this batch (src/kmer.py:557-558).  ``unique_batch``: the ids
        come from one parsed FASTQ container, which the grammar made unique."""
        if not self._batches and not self._host and unique_batch:
            return
        known = self._known_ids()
        seen: Set[str] = set()
        for i, rid in enumerate(ids):
            if dropped is not None and dropped[i]:
                continue
            if rid in known or (not unique_batch and rid in seen):
                raise AddingExistingRead(f"There already exists a read with identifier: {rid}")
            if not unique_batch:
                seen.add(rid)

    def _trim_stats_of(self, mate: int) -> Optional["N.TrimStats"]:
        t = _TRIM.get(self)
        return None if t is None else t[1 + mate]

    def _trim_spec(self, mate: int = 1) -> Optional["N.TrimSpec"]:
        t = _TRIM.get(self)
        return None if t is None else t[mate - 1]

    def _trimmed(self, seq, qual, off, mate: int = 1):
        """The columns as the rest of the alignment sees them: trimmed on the
        device when mate ``mate`` has a trim spec, else as given."""
        spec = self._trim_spec(mate)
        if spec is None:
            return seq, qual, off
        return _trim_on_device(seq, qual, off, spec, _TRIM[self][1 + mate], self.kmer_reference.index.device)

    def get_trim_stats(self, mate: Optional[int] = None) -> Optional[Dict[str, int]]:
        """What the trim cut off so far (pa_trim_stats as a dict): of mate 1's
        or mate 2's reads, or of both summed (``mate`` None).  None for an
        alignment made without ``trim``."""
        t = _TRIM.get(self)
        if t is None:
            return None
        if mate is not None:
            return t[1 + mate].as_dict()
        a, b = t[2].as_dict(), t[3].as_dict()
        return {k: a[k] + b[k] for k in a}

    def add_read(self, read: Read) -> None:
        self._add_ids([read.identifier], None, False)
        if self._ids is not None:
            self._ids.add(read.identifier)
        entry = {"mapping_type": read.mapping.type,
                 "genomes_mapped_to": [g.identifier for g in read.mapping.genomes_mapped_to]}
        self._host.append((self._next_index, read.identifier, entry))
        self._next_index += 1

    def add_read_from_read_record(self, read_record: Record, m: int = 1, p: int = 1,
                                  min_read_quality: Optional[int] = None, min_kmer_quality: Optional[int] = None,
                                  max_genomes: Optional[int] = None) -> None:
        ids = [read_record.identifier]
        seq, off = N.concat([read_record["sequence"]])
        qual = np.frombuffer(read_record["quality_sequence"].encode("latin-1", errors="replace"), dtype=np.uint8)
        self._align_columns(ids, seq, qual, off, m, p, min_read_quality, min_kmer_quality, max_genomes)

    def align_reads_from_container(self, reads_container: FASTAQRecordContainer, m: int = 1, p: int = 1,
                                   min_read_quality: Optional[int] = None, min_kmer_quality: Optional[int] = None,
                                   max_genomes: Optional[int] = None) -> None:
        ids, seq, qual, off = _columnar(reads_container)
        self._align_columns(ids, seq, qual, off, m, p, min_read_quality, min_kmer_quality, max_genomes,
                            unique_batch=isinstance(reads_container, FASTAQRecordContainer))

    def align_reads_from_file(self, reads_file: str, m: int = 1, p: int = 1, min_read_quality: Optional[int] = None,
                              min_kmer_quality: Optional[int] = None, max_genomes: Optional[int] = None, *,
                              prefetch: Optional["N.FastqPrefetch"] = None) -> None:
        """FASTAQFile(reads_file).container + align_reads_from_container as one
        device pass (pa_align_fastq_file: the file is parsed on the GPU and
        aligned in windows while the host reads the next).  Per-read results
        (``reads``) parse the file again when asked for.  A file outside the
        device-parsed subset of the grammar, a duplicate id, arguments the
        reference rejects, or reads already added take the exact path.
        ``prefetch``: the same file already on its way to the device
        (N.FastqPrefetch, started before the index build); consumed here."""
        from data_file import FASTAQFile
        # (a coverage job takes the host-parsed path: the placements need the read columns)
        fresh = (not self._batches and not self._host and self._result is None and self not in _COVERAGE
                 and self not in _PILEUP and self not in _ABUNDANCE and self not in _LINEAGE
                 and self not in _CONTAINMENT)
        err = _check_align_args(self.kmer_reference, m, p, min_read_quality, min_kmer_quality, max_genomes)
        n = None
        if fresh and err is None and os.environ.get("PA_STREAM", "1") != "0":
            FASTAQFile.check_extension(reads_file)
            ref = self.kmer_reference
            result = N.Result(ref.index)
            prm = N.Params.make(m, p, min_read_quality, min_kmer_quality, max_genomes)
            if prefetch is not None and prefetch.device == ref.index.device:
                n = N.align_fastq_prefetched(ref.index, prefetch, prm, self._next_index, result,
                                             trim=self._trim_spec(), trim_stats=self._trim_stats_of(1))
            else:
                n = N.align_fastq_file(ref.index, reads_file, prm, self._next_index, result,
                                       trim=self._trim_spec(), trim_stats=self._trim_stats_of(1))
            if n is None:
                result.close()
        if prefetch is not None:
            prefetch.close()
        if n is None:
            self.align_reads_from_container(FASTAQFile(reads_file).container, m, p, min_read_quality,
                                            min_kmer_quality, max_genomes)
            return
        self._adopt_streamed(result, reads_file, prm, n, min_read_quality, min_kmer_quality, max_genomes)

    def extract_reads_from_file(self, reads_file: str, out_file: str, mapping: Sequence[str] = ("unique", "ambiguous"),
                                genomes: Optional[Sequence[str]] = None, invert: bool = False, m: int = 1, p: int = 1,
                                min_read_quality: Optional[int] = None, min_kmer_quality: Optional[int] = None,
                                max_genomes: Optional[int] = None, *, host_parsed: bool = False) -> Dict[str, Any]:
        """align_reads_from_file, with the selected reads written to ``out_file``
        as FASTQ records in file order.  ``mapping``: the
        read types to select, of "unique", "ambiguous", "unmapped" and
        "filtered"; ``genomes``: identifiers that restrict the mapped reads to
        those whose genomes_mapped_to holds one of them (None: no
        restriction); ``invert``: everything else instead.  Returns the
        statistics (records, selected, bytes, selected_by_type).  The records
        are gathered on the device from the device-parsed file where
        align_reads_from_file would stream it; otherwise, and for a file
        outside that subset of the grammar, the exact parser's records are
        selected by N.reads_select and written by the host (``host_parsed``:
        at once, for a job that needs the host-parsed records anyway)."""
        from data_file import FASTAQFile
        type_mask = extract_type_mask(mapping)
        ref = self.kmer_reference
        keep = None
        if genomes is not None:
            names = [g.identifier for g in ref.genomes]
            unknown = [x for x in genomes if x not in set(names)]
            if unknown:
                raise ValueError(f"unknown genome identifier: {unknown[0]}")
            wanted = set(genomes)
            keep = np.fromiter((name in wanted for name in names), dtype=np.uint8, count=len(names))
        spec = N.ExtractSpec.make(type_mask, keep, invert)
        fresh = (not self._batches and not self._host and self._result is None and self not in _COVERAGE
                 and self not in _PILEUP and self not in _ABUNDANCE and self not in _LINEAGE
                 and self not in _CONTAINMENT)
        err = _check_align_args(ref, m, p, min_read_quality, min_kmer_quality, max_genomes)
        with open(out_file, "wb") as fh:
            if fresh and err is None and not host_parsed and os.environ.get("PA_STREAM", "1") != "0":
                FASTAQFile.check_extension(reads_file)
                result = N.Result(ref.index)
                prm = N.Params.make(m, p, min_read_quality, min_kmer_quality, max_genomes)
                n, stats = N.extract_fastq_file(ref.index, reads_file, prm, spec, fh.fileno(), self._next_index, result,
                                                trim=self._trim_spec(), trim_stats=self._trim_stats_of(1))
                if n is not None:
                    self._adopt_streamed(result, reads_file, prm, n, min_read_quality, min_kmer_quality, max_genomes)
                    return stats
                result.close()
                fh.truncate(0)  # (a late window refused: what the earlier ones wrote goes)
                fh.seek(0)
            # the exact path: a parse error leaves the (truncated) file empty
            container = FASTAQFile(reads_file).container
            self.align_reads_from_container(container, m, p, min_read_quality, min_kmer_quality, max_genomes)
            ids, seq, qual, off = _columnar(container)
            n = len(ids)
            batch = self._batches[-1] if n else None
            if n == 0:
                sel = np.zeros(0, dtype=bool)
                types = np.zeros(0, dtype=np.uint8)
            elif batch.all_dropped:  # (no device pass was made: every read is PA_DROPPED)
                types = np.zeros(n, dtype=np.uint8)
                sel = np.full(n, bool(type_mask & 1) != bool(invert))
            else:
                # (the selection is decided on the reads as aligned -- trimmed, when a trim is set;
                # the records written below are the file's own)
                reads = N.Reads.upload(batch.seq, batch.qual, batch.off, device=ref.index.device)
                try:
                    sel = N.reads_select(ref.index, reads, batch.params, spec)
                    types = None
                    if sel.any():  # (the statistics' types: the batch's own per-read results)
                        types, _, _, _, _ = N.align_reads(ref.index, reads, batch.params)
                finally:
                    reads.close()
            stats = {"records": n, "selected": int(sel.sum()), "bytes": 0,
                     "selected_by_type": {name: 0 for name in N.EXTRACT_TYPE_NAMES}}
            off = np.asarray(off, dtype=np.int64)
            chunks: List[bytes] = []
            held = 0
            for i in np.flatnonzero(sel):
                a, b = int(off[i]), int(off[i + 1])
                rec = b"@" + ids[i].encode("utf-8") + b"\n" + seq[a:b].tobytes() + b"\n+\n" + qual[a:b].tobytes() + b"\n"
                chunks.append(rec)
                held += len(rec)
                stats["bytes"] += len(rec)
                stats["selected_by_type"][N.EXTRACT_TYPE_NAMES[int(types[i])]] += 1
                if held >= (8 << 20):
                    fh.write(b"".join(chunks))
                    chunks, held = [], 0
            fh.write(b"".join(chunks))
        return stats

    def _adopt_streamed(self, result, reads_file, prm, n, mrq, mkq, mg) -> None:
        """The bookkeeping of a file the device-parsed stream aligned into ``result``."""
        if mrq is not None:
            self.filter_read_quality_flag = True
        if mkq is not None:
            self.filter_kmer_quality_flag = True
        if mg is not None:
            self.filter_max_genomes_flag = True
        self._result = result
        stats, _, _, _ = result.fetch()
        self._gpu_stats = stats
        self.filtered_quality_reads += int(stats[3])
        self.filtered_quality_kmers += int(stats[4])
        self.filtered_hr_kmers += int(stats[5])
        self._batches.append(_FileBatch(self._next_index, reads_file, prm, mrq, n, self._trim_spec(),
                                        self.kmer_reference.index.device))
        self._next_index += n
        self._streamed_records = n  # (diagnostics: the device-parsed path was taken)

    def _align_columns(self, ids, seq, qual, off, m, p, mrq, mkq, mg, unique_batch=False) -> None:
        n = len(ids)
        if n == 0:
            return
        trimmed = None  # (the trimmed batch on the device: aligned below as it is, not uploaded again)
        if self._trim_spec() is not None:
            seq, qual, off, trimmed = _trim_on_device(seq, qual, off, self._trim_spec(), self._trim_stats_of(1),
                                                      self.kmer_reference.index.device, keep=True)
        try:  # (all below sees the trimmed reads)
            self._align_trimmed_columns(ids, seq, qual, off, m, p, mrq, mkq, mg, unique_batch, trimmed)
        finally:
            if trimmed is not None:
                trimmed.close()

    def _align_trimmed_columns(self, ids, seq, qual, off, m, p, mrq, mkq, mg, unique_batch, on_device) -> None:
        """_align_columns after its trim (the columns as given when none is set).
        ``on_device``: the same columns as a device batch already, or None."""
        n = len(ids)
        if mrq is not None:
            self.filter_read_quality_flag = True
        if mkq is not None:
            self.filter_kmer_quality_flag = True
        if mg is not None:
            self.filter_max_genomes_flag = True
        err = _check_align_args(self.kmer_reference, m, p, mrq, mkq, mg)
        all_dropped = False
        if err is not None:
            # the reference checks the arguments (Read.pseudo_align) only for
            # reads that pass --min-read-quality (src/kmer.py:587-592): a batch
            # whose every read is dropped by it is only counted
            if mrq is None or isinstance(mrq, bool) or not isinstance(mrq, (int, float)):
                raise err
            if not _dropped_mask(qual, off, mrq).all():
                raise err
            all_dropped = True
        dropped = _dropped_mask(qual, off, mrq) if (mrq is not None and (self._batches or self._host
                                                                          or not unique_batch)) else None
        self._add_ids(ids, np.ones(n, dtype=bool) if all_dropped else dropped, unique_batch)
        ref = self.kmer_reference
        prm = None
        read_node = None
        if all_dropped:
            self.filtered_quality_reads += n
            if self in _LINEAGE:
                _LINEAGE[self][3] += n
                read_node = np.full(n, N.NO_NODE, dtype=np.uint32)
            if self in _CONTAINMENT:
                _CONTAINMENT[self][1] += n
        else:
            if self._result is None:
                self._result = N.Result(ref.index)
            prm = N.Params.make(m, p, mrq, mkq, mg)
            # the align-side view this batch repays (the neighbour bits only
            # past their break-even in reads per genome base; pa_index_prepare_ex)
            ref.index.prepare(expected_reads=n)
            reads = on_device if on_device is not None else N.Reads.upload(seq, qual, off, device=ref.index.device)
            N.align(ref.index, reads, prm, self._next_index, self._result)
            stats, _, _, _ = self._result.fetch()
            if self in _COVERAGE:
                self._coverage().add(reads, prm)
            if self in _PILEUP:
                self._pileup().add(reads, prm, _PILEUP[self][1])
            if self in _ABUNDANCE:
                self._abundance().add(reads, prm)
            if self in _LINEAGE:
                read_node = self._lineage().add(reads, prm)
            if self in _CONTAINMENT:
                self._containment().add(reads, prm)
            reads.close()
            delta = stats - self._gpu_stats
            self._gpu_stats = stats
            self.filtered_quality_reads += int(delta[3])
            self.filtered_quality_kmers += int(delta[4])
            self.filtered_hr_kmers += int(delta[5])
        b = _Batch(self._next_index, ids, seq, qual, off, prm, mrq, all_dropped)
        b._dropped = dropped
        b.read_node = read_node
        self._batches.append(b)
        if self._ids is not None:
            d = b.dropped()
            self._ids.update(ids if d is None else (i for i, x in zip(ids, d) if not x))
        self._next_index += n

    def align_pairs_from_containers(self, reads1, reads2, m: int = 1, p: int = 1,
                                    min_read_quality: Optional[int] = None, min_kmer_quality: Optional[int] = None,
                                    max_genomes: Optional[int] = None) -> None:
        """Paired-end reads: record i of ``reads1`` and record i of ``reads2`` are
        the two ends of one fragment, classified as one by the k-mers of both
        mates together.  ``reads``, the counters and
        ``write_assignments`` hold one entry per pair, under pair_identifier of
        the mates' ids.  The mates are taken as given: nothing is reverse-
        complemented here, so paired data wants a both-strand reference."""
        if self in _COVERAGE or self in _PILEUP or self in _ABUNDANCE:
            raise ValueError("pairs are not supported with coverage, pileup or abundance: those accumulators take reads")
        if self in _LINEAGE:
            raise ValueError("pairs are not supported with lineages: that accumulator takes reads")
        if self in _CONTAINMENT:
            raise ValueError("pairs are not supported with containment: that accumulator takes reads")
        ids1, seq1, qual1, off1 = _columnar(reads1)
        ids2, seq2, qual2, off2 = _columnar(reads2)
        if len(ids1) != len(ids2):
            raise ValueError(f"The two read files of a paired job hold different numbers of records: "
                             f"{len(ids1)} and {len(ids2)}")
        n = len(ids1)
        if n == 0:
            return
        ids = [pair_identifier(a, b) for a, b in zip(ids1, ids2)]
        seq1, qual1, off1 = self._trimmed(seq1, qual1, off1, 1)  # (each mate by its own spec)
        seq2, qual2, off2 = self._trimmed(seq2, qual2, off2, 2)
        mrq, mkq, mg = min_read_quality, min_kmer_quality, max_genomes
        if mrq is not None:
            self.filter_read_quality_flag = True
        if mkq is not None:
            self.filter_kmer_quality_flag = True
        if mg is not None:
            self.filter_max_genomes_flag = True
        err = _check_align_args(self.kmer_reference, m, p, mrq, mkq, mg)
        dropped = None
        if mrq is not None and not isinstance(mrq, bool) and isinstance(mrq, (int, float)):
            dropped = _dropped_mask(qual1, off1, mrq) | _dropped_mask(qual2, off2, mrq)
        all_dropped = False
        if err is not None:  # (as _align_columns: the arguments are checked only for what passes the read filter)
            if dropped is None or not dropped.all():
                raise err
            all_dropped = True
        self._add_ids(ids, dropped, False)  # (two mates' ids can collapse to one pair id: checked within the batch)
        ref = self.kmer_reference
        prm = None
        if all_dropped:
            self.filtered_quality_reads += n
        else:
            if self._result is None:
                self._result = N.Result(ref.index)
            prm = N.Params.make(m, p, mrq, mkq, mg)
            ref.index.prepare(expected_reads=2 * n)
            m1 = N.Reads.upload(seq1, qual1, off1, device=ref.index.device)
            m2 = N.Reads.upload(seq2, qual2, off2, device=ref.index.device)
            try:
                N.align_pairs(ref.index, m1, m2, prm, self._next_index, self._result, lists=False)
            finally:
                m1.close()
                m2.close()
            stats, _, _, _ = self._result.fetch()
            delta = stats - self._gpu_stats
            self._gpu_stats = stats
            self.filtered_quality_reads += int(delta[3])
            self.filtered_quality_kmers += int(delta[4])
            self.filtered_hr_kmers += int(delta[5])
        b = _PairBatch(self._next_index, ids, (seq1, qual1, off1), (seq2, qual2, off2), prm, mrq, all_dropped)
        b._dropped = dropped
        self._batches.append(b)
        if self._ids is not None:
            self._ids.update(ids if dropped is None else (i for i, x in zip(ids, dropped) if not x))
        self._next_index += n

    # -- results ----------------------------------------------------------------

    @property
    def reads(self) -> Dict[str, Dict[str, Any]]:
        """``{read id: {"mapping_type", "genomes_mapped_to"}}`` in insertion order;
        reads dropped by --min-read-quality are absent (src/kmer.py:587-589)."""
        ref = self.kmer_reference
        items: List[Tuple[int, str, Dict[str, Any]]] = list(self._host)
        for b in self._batches:
            if b.all_dropped:
                continue
            if b.entries is None:
                b.load()
                types, loff, lists = b.results(ref.index)
                names = [g.identifier for g in ref.genomes]
                ent = []
                for i, t in enumerate(types):
                    if t == _DROPPED:  # filtered by --min-read-quality: not a read of the alignment
                        continue
                    gl = [names[int(g)] for g in lists[loff[i]:loff[i + 1]]]
                    ent.append((b.base + i, b.ids[i], {"mapping_type": ReadMappingType(int(t)),
                                                       "genomes_mapped_to": gl}))
                b.entries = ent
            items.extend(b.entries)
        items.sort(key=lambda x: x[0])
        return {rid: e for _, rid, e in items}

    def write_assignments(self, fh) -> None:
        """Read -> genome as text: the header ``#read<TAB>mapping<TAB>genomes``, then one
        line per read in the order the reads were added (assignment_line).
        Reads dropped by --min-read-quality are written as ``filtered``, so a
        FASTQ file gives as many lines as it has records.  Written batch by
        batch from the device's per-read arrays; the ``reads`` dict is not built.
        An alignment made with ``lineages`` writes a fourth column ``taxon``
        (ASSIGNMENTS_TAXON_HEADER): the path of the read's node, empty for a read
        without one."""
        ref = self.kmer_reference
        names = [g.identifier for g in ref.genomes]
        # lineages: a fourth column, the path of the read's node (empty: none, or a read of add_read())
        paths = self._lineage_tree().paths if self in _LINEAGE else None

        def line(rid, mapping_type, genomes, node=N.NO_NODE) -> str:
            text = assignment_line(rid, mapping_type, genomes)
            if paths is None:
                return text
            return text[:-1] + "\t" + (paths[int(node)] if int(node) != N.NO_NODE else "") + "\n"

        def node_of(b, i):
            return N.NO_NODE if b.read_node is None else b.read_node[i]
        fh.write(ASSIGNMENTS_HEADER if paths is None else ASSIGNMENTS_TAXON_HEADER)
        parts: List[Tuple[int, Any]] = [(b.base, b) for b in self._batches] + [(i, (rid, e)) for i, rid, e in self._host]
        parts.sort(key=lambda x: x[0])
        for _, part in parts:
            if isinstance(part, tuple):  # a read of add_read()
                rid, e = part
                fh.write(line(rid, int(e["mapping_type"].value), e["genomes_mapped_to"]))
                continue
            b = part
            b.load()
            if b.all_dropped:
                fh.writelines(line(rid, _DROPPED, ()) for rid in b.ids)
                continue
            types, loff, lists = b.results(ref.index)
            loff = loff.astype(np.int64)
            fh.writelines(line(rid, int(types[i]), [names[int(g)] for g in lists[loff[i]:loff[i + 1]]], node_of(b, i))
                          for i, rid in enumerate(b.ids))

    def get_summary(self) -> Dict[str, Dict[str, Union[int, Dict[str, int]]]]:
        stats = self._gpu_stats.astype(np.int64)
        summary: Dict[str, Union[int, Dict[str, int]]] = {
            "unique_mapped_reads": int(stats[0]),
            "ambiguous_mapped_reads": int(stats[1]),
            "unmapped_reads": int(stats[2]),
        }
        if self.filter_read_quality_flag:
            summary["filtered_quality_reads"] = self.filtered_quality_reads
        if self.filter_kmer_quality_flag:
            summary["filtered_quality_kmers"] = self.filtered_quality_kmers
        if self.filter_max_genomes_flag:
            summary["filtered_hr_kmers"] = self.filtered_hr_kmers
        counts: Dict[str, List[int]] = {}
        first: Dict[str, int] = {}
        if self._result is not None:
            _, uq, am, fk = self._result.fetch()
            for g in np.flatnonzero(fk != N.NO_FIRST_KEY):
                name = self.kmer_reference.genomes[int(g)].identifier
                c = counts.setdefault(name, [0, 0])
                c[0] += int(uq[g])
                c[1] += int(am[g])
                first[name] = min(first.get(name, _NO_KEY), int(fk[g]))
        for idx, _, e in self._host:
            t = e["mapping_type"]
            if t == ReadMappingType.UNMAPPED:
                summary["unmapped_reads"] += 1
                continue
            col = 0 if t == ReadMappingType.UNIQUELY_MAPPED else 1
            summary["unique_mapped_reads" if col == 0 else "ambiguous_mapped_reads"] += 1
            for pos, name in enumerate(e["genomes_mapped_to"]):
                counts.setdefault(name, [0, 0])[col] += 1
                first[name] = min(first.get(name, _NO_KEY), (idx << 20) | pos)
        genome_mapping = {name: {"unique_reads": counts[name][0], "ambiguous_reads": counts[name][1]}
                          for name in sorted(first, key=first.get)}
        return {"Statistics": summary, "Summary": genome_mapping}

    def _coverage(self) -> "N.Coverage":
        cov = _COVERAGE[self]
        if cov is None:
            cov = _COVERAGE[self] = N.Coverage(self.kmer_reference.index)
        return cov

    def get_coverage(self, genomes: Optional[Sequence[str]] = None, min_coverage: int = 1,
                     full: bool = False) -> Dict[str, Dict[str, Any]]:
        """``{"Coverage": {identifier: {"covered_bases_unique", "covered_bases_ambiguous",
        "mean_coverage_unique", "mean_coverage_ambiguous"}}}`` for the genomes
        named in ``genomes`` (None: all), in FASTA order, genomes no read covers
        included; covered = positions at least ``min_coverage`` reads deep, mean =
        summed depth / genome length, rounded to one decimal.  ``full`` adds
        ``"Details": {identifier: {"unique_cov": [...], "ambiguous_cov": [...]}}``,
        the depth at every position.  ValueError for an alignment made without
        ``coverage=True`` (or loaded from a file) and for an unknown identifier."""
        if self not in _COVERAGE:
            raise ValueError("this alignment was made without coverage=True")
        if isinstance(min_coverage, bool) or not isinstance(min_coverage, int) or min_coverage < 1:
            raise ValueError("min_coverage must be an integer of at least 1")
        names = [g.identifier for g in self.kmer_reference.genomes]
        if genomes is not None:
            known = set(names)
            unknown = [x for x in genomes if x not in known]
            if unknown:
                raise ValueError(f"unknown genome identifier: {unknown[0]}")
            wanted = set(genomes)
        cov = self._coverage()
        cu, ca, su, sa = cov.summary(min_coverage)
        out: Dict[str, Dict[str, Any]] = {"Coverage": {}}
        if full:
            out["Details"] = {}
        for g, name in enumerate(names):
            if genomes is not None and name not in wanted:
                continue
            n = cov.lengths[g]
            out["Coverage"][name] = {
                "covered_bases_unique": int(cu[g]),
                "covered_bases_ambiguous": int(ca[g]),
                "mean_coverage_unique": round(int(su[g]) / n, 1) if n else 0.0,
                "mean_coverage_ambiguous": round(int(sa[g]) / n, 1) if n else 0.0,
            }
            if full:
                du, da = cov.depth(g)
                out["Details"][name] = {"unique_cov": [int(x) for x in du], "ambiguous_cov": [int(x) for x in da]}
        return out

    def _pileup(self) -> "N.Pileup":
        slot = _PILEUP[self]
        if slot[0] is None:
            slot[0] = N.Pileup(self.kmer_reference.index)
        return slot[0]

    def _variant_records(self, min_depth, min_alt_count, min_alt_fraction):
        if self not in _PILEUP:
            raise ValueError("this alignment was made without pileup=True")
        for v, name in ((min_depth, "min_depth"), (min_alt_count, "min_alt_count")):
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v < 2 ** 32:
                raise ValueError(f"{name} must be an integer of at least 1")
        return self._pileup().variants(min_depth, min_alt_count, variant_permille(min_alt_fraction))

    def get_variants(self, min_depth: int = 4, min_alt_count: int = 2,
                     min_alt_fraction: float = 0.2) -> List[Dict[str, Any]]:
        """The positions where the uniquely mapped reads differ from the reference:
        one ``{"genome", "position", "ref", "alt", "depth", "alt_count", "A", "C",
        "G", "T"}`` per (position, alternative base) with depth >= ``min_depth``,
        alt_count >= ``min_alt_count`` and alt_count / depth >= ``min_alt_fraction``,
        ordered by genome (FASTA order), position (0-based, forward) and base.
        The fraction becomes the integer round(1000 * min_alt_fraction) once
        (variant_permille) and the device compares 1000 * alt_count with it times
        depth.  ValueError for an alignment made without ``pileup=True`` (or
        loaded from a file)."""
        names = [g.identifier for g in self.kmer_reference.genomes]
        out = []
        for v in self._variant_records(min_depth, min_alt_count, min_alt_fraction):
            a = [int(x) for x in v["acgt"]]
            out.append({"genome": names[int(v["genome"])], "position": int(v["position"]),
                        "ref": "ACGT"[int(v["ref"])], "alt": "ACGT"[int(v["alt"])], "depth": int(v["depth"]),
                        "alt_count": int(v["alt_count"]), "A": a[0], "C": a[1], "G": a[2], "T": a[3]})
        return out

    def write_variants(self, fh, min_depth: int = 4, min_alt_count: int = 2, min_alt_fraction: float = 0.2) -> None:
        """get_variants as text: VARIANTS_HEADER, then one tab-separated line per record."""
        fh.write(VARIANTS_HEADER)
        fh.writelines("\t".join(str(v[c]) for c in ("genome", "position", "ref", "alt", "depth", "alt_count",
                                                    "A", "C", "G", "T")) + "\n"
                      for v in self.get_variants(min_depth, min_alt_count, min_alt_fraction))

    def _abundance(self) -> "N.Abundance":
        ab = _ABUNDANCE[self]
        if ab is None:
            ab = _ABUNDANCE[self] = N.Abundance(self.kmer_reference.index)
        return ab

    def get_abundance(self, iterations: int = 200, tolerance: float = 1e-9, bootstraps: int = 0, seed: int = 1,
                      confidence: float = 0.95) -> Dict[str, Any]:
        """The EM estimate over the reads' compatibility classes (DESIGN.md section
        14): ``{"genomes": [{"genome", "length", "unique_reads", "compatible_reads",
        "estimated_reads", "read_fraction", "abundance"}, ...], "reads", "iterations",
        "last_delta", "classes"}``, one entry per genome of the index in FASTA
        order.  compatible_reads counts the reads whose class holds the genome,
        estimated_reads = read_fraction * reads.  With ``bootstraps`` > 0 (at most
        10000) that many bootstrap replicates of the estimate are run under
        ``seed``: every genome gains "abundance_mean",
        "abundance_sd", "abundance_lo" and "abundance_hi" (bootstrap_summary of the
        replicates' abundances at ``confidence``) and the dict "bootstraps", "seed"
        and "confidence".  ValueError for an alignment made without
        ``abundance=True`` (or loaded from a file), iterations outside 1 .. 10000,
        a negative tolerance, bootstraps outside 0 .. 10000, a seed outside
        0 .. 2^64 - 1 and a confidence bootstrap_summary refuses."""
        return self._abundance_estimates(iterations, tolerance, bootstraps, seed, confidence)[0]

    def _abundance_estimates(self, iterations, tolerance, bootstraps, seed, confidence):
        """(get_abundance's dict, the replicates x genomes abundance matrix or None)."""
        if self not in _ABUNDANCE:
            raise ValueError("this alignment was made without abundance=True")
        if isinstance(iterations, bool) or not isinstance(iterations, int) or not 1 <= iterations <= 10000:
            raise ValueError("iterations must be an integer in 1 .. 10000")
        if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float)) or not tolerance >= 0:
            raise ValueError("tolerance must be a number that is not negative")
        if isinstance(bootstraps, bool) or not isinstance(bootstraps, int) or not 0 <= bootstraps <= 10000:
            raise ValueError("bootstraps must be an integer in 0 .. 10000")
        if bootstraps:
            if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed <= 2 ** 64 - 1:
                raise ValueError("seed must be an integer in 0 .. 2^64 - 1")
            confidence_permille(confidence)
        ab = self._abundance()
        names = [g.identifier for g in self.kmer_reference.genomes]
        G = len(names)
        off, gen, cnt = ab.classes()
        compatible = np.zeros(G, dtype=np.uint64)
        np.add.at(compatible, gen, np.repeat(cnt, np.diff(off).astype(np.int64)))
        unique = self._result.fetch()[1] if self._result is not None else np.zeros(G, dtype=np.uint64)
        theta, share, done, delta = ab.estimate(iterations, float(tolerance))
        n_reads = int(cnt.sum())
        out = {"genomes": [{"genome": names[g], "length": ab.lengths[g], "unique_reads": int(unique[g]),
                            "compatible_reads": int(compatible[g]), "estimated_reads": float(theta[g]) * n_reads,
                            "read_fraction": float(theta[g]), "abundance": float(share[g])} for g in range(G)],
               "reads": n_reads, "iterations": done, "last_delta": delta, "classes": int(cnt.size)}
        shares = None
        if bootstraps:
            shares = ab.bootstrap(bootstraps, seed, iterations, float(tolerance))[1]
            for row, stats in zip(out["genomes"], bootstrap_summary(shares, confidence)):
                row.update(zip(ABUNDANCE_BOOTSTRAP_COLUMNS, stats))
            out.update(bootstraps=bootstraps, seed=seed, confidence=float(confidence))
        return out, shares

    def write_abundance(self, fh, iterations: int = 200, tolerance: float = 1e-9, bootstraps: int = 0, seed: int = 1,
                        confidence: float = 0.95) -> None:
        """get_abundance as text (abundance_text)."""
        a = self.get_abundance(iterations, tolerance, bootstraps, seed, confidence)
        rows = a["genomes"]
        boot = None
        if bootstraps:
            boot = ([tuple(r[c] for c in ABUNDANCE_BOOTSTRAP_COLUMNS) for r in rows], a["bootstraps"], a["seed"],
                    a["confidence"])
        fh.write(abundance_text([r["genome"] for r in rows], [r["length"] for r in rows],
                                [r["unique_reads"] for r in rows], [r["compatible_reads"] for r in rows],
                                [r["read_fraction"] for r in rows], [r["abundance"] for r in rows], a["reads"],
                                a["iterations"], a["last_delta"], a["classes"], boot))

    def _lineage_tree(self) -> LineageTree:
        slot = _LINEAGE[self]
        if slot[1] is None:
            slot[1] = slot[0].tree([g.identifier for g in self.kmer_reference.genomes])
        return slot[1]

    def _lineage(self) -> "N.Lineage":
        slot = _LINEAGE[self]
        if slot[2] is None:
            tree = self._lineage_tree()
            slot[2] = N.Lineage(self.kmer_reference.index, tree.parent, tree.genome_node)
        return slot[2]

    def get_lineage_report(self, iterations: int = 200, tolerance: float = 1e-9, bootstraps: int = 0, seed: int = 1,
                           confidence: float = 0.95) -> Dict[str, Any]:
        """The reads rolled up the lineage tree: ``{"rows":
        [{"node", "taxon", "depth", "genomes", "reads_clade", "reads_direct",
        "clade_share"}, ...], "reads", "classified", "unmapped", "dropped",
        "nodes"}``, one row per node in preorder (children in node order).  An
        alignment that also has ``abundance=True`` gains per row "read_fraction"
        and "abundance" -- the genomes' estimates summed over the subtree in
        ascending genome index -- and "iterations", "last_delta" and "classes";
        with ``bootstraps`` the four ABUNDANCE_BOOTSTRAP_COLUMNS per row, from
        bootstrap_summary of the replicates x nodes matrix rolled up the same way.
        The arguments are get_abundance's and are read only with abundance.
        ValueError for an alignment made without ``lineages``."""
        if self not in _LINEAGE:
            raise ValueError("this alignment was made without lineages")
        tree = self._lineage_tree()
        direct, clade, info = self._lineage().counts()
        rows = lineage_report_rows(tree, direct, clade)
        if self in _CONTAINMENT:  # (section 21: the clades' k-mers, after every other column)
            _, _, ck, cs = self._containment().nodes(self._lineage())
            for r in rows:
                v = r["node"]
                r["kmers_clade"], r["kmers_seen_clade"] = int(ck[v]), int(cs[v])
                r["kmer_containment"] = int(cs[v]) / int(ck[v]) if int(ck[v]) else 0.0
        dropped = info["reads_dropped"] + _LINEAGE[self][3]
        out: Dict[str, Any] = {"rows": rows, "classified": int(clade[0]), "unmapped": info["reads_unmapped"],
                               "dropped": dropped, "nodes": tree.n_nodes}
        out["reads"] = out["classified"] + out["unmapped"] + dropped
        if self in _ABUNDANCE:
            a, shares = self._abundance_estimates(iterations, tolerance, bootstraps, seed, confidence)
            theta = tree.roll_up([g["read_fraction"] for g in a["genomes"]])
            share = tree.roll_up([g["abundance"] for g in a["genomes"]])
            for r in rows:
                r["read_fraction"], r["abundance"] = theta[r["node"]], share[r["node"]]
            out.update(iterations=a["iterations"], last_delta=a["last_delta"], classes=a["classes"])
            if shares is not None:
                rolled = np.array([tree.roll_up(rep) for rep in shares], dtype=np.float64).reshape(len(shares), -1)
                summary = bootstrap_summary(rolled, confidence)
                for r in rows:
                    r.update(zip(ABUNDANCE_BOOTSTRAP_COLUMNS, summary[r["node"]]))
                out.update(bootstraps=a["bootstraps"], seed=a["seed"], confidence=a["confidence"])
        return out

    def write_lineage_report(self, fh, iterations: int = 200, tolerance: float = 1e-9, bootstraps: int = 0,
                             seed: int = 1, confidence: float = 0.95) -> None:
        """get_lineage_report as text (lineage.lineage_report_text)."""
        rep = self.get_lineage_report(iterations, tolerance, bootstraps, seed, confidence)
        ab = None
        if "iterations" in rep:
            boot = (rep["bootstraps"], rep["seed"], rep["confidence"]) if "bootstraps" in rep else None
            ab = (rep["iterations"], rep["last_delta"], rep["classes"], boot)
        fh.write(lineage_report_text(rep["rows"], rep["reads"], rep["unmapped"], rep["dropped"], ab,
                                     containment=self in _CONTAINMENT))

    def _containment(self) -> "N.Containment":
        slot = _CONTAINMENT[self]
        if slot[0] is None:
            slot[0] = N.Containment(self.kmer_reference.index)
        return slot[0]

    def get_containment(self, genomes: Optional[Sequence[str]] = None) -> Dict[str, Any]:
        """The distinct k-mers of every genome the reads hold (DESIGN.md section
        21): ``{"genomes": [{"genome", "length", "kmers", "kmers_seen",
        "containment", "identity", "specific_kmers", "specific_seen",
        "specific_containment", "specific_hits", "duplication"}, ...], "info":
        {CONTAINMENT_INFO}}`` for the genomes named in ``genomes`` (None: all),
        in FASTA order.  ValueError for an alignment made without
        ``containment=True`` (or loaded from a file) and for an unknown
        identifier."""
        if self not in _CONTAINMENT:
            raise ValueError("this alignment was made without containment=True")
        ref = self.kmer_reference
        names = [g.identifier for g in ref.genomes]
        wanted = None
        if genomes is not None:
            known = set(names)
            unknown = [x for x in genomes if x not in known]
            if unknown:
                raise ValueError(f"unknown genome identifier: {unknown[0]}")
            wanted = set(genomes)
        c, info = self._containment().counts()
        info["reads"] += _CONTAINMENT[self][1]
        info["reads_dropped"] += _CONTAINMENT[self][1]
        k = int(ref.kmer_len)
        lengths = self._containment().lengths
        rows = []
        for g, name in enumerate(names):
            if wanted is not None and name not in wanted:
                continue
            cont, scont, dup, ident = containment_ratios(k, c["kmers"][g], c["kmers_seen"][g], c["specific"][g],
                                                         c["specific_seen"][g], c["hits_specific"][g])
            rows.append({"genome": name, "length": lengths[g], "kmers": int(c["kmers"][g]),
                         "kmers_seen": int(c["kmers_seen"][g]), "containment": cont, "identity": ident,
                         "specific_kmers": int(c["specific"][g]), "specific_seen": int(c["specific_seen"][g]),
                         "specific_containment": scont, "specific_hits": int(c["hits_specific"][g]),
                         "duplication": dup})
        return {"genomes": rows, "info": info}

    def write_containment(self, fh, genomes: Optional[Sequence[str]] = None) -> None:
        """get_containment as text (containment_text)."""
        rep = self.get_containment(genomes)
        fh.write(containment_text(rep["genomes"], rep["info"]))

    def get_reads_by_mapping_type(self, mapping_type: ReadMappingType) -> List[str]:
        return [rid for rid, d in self.reads.items() if d["mapping_type"] == mapping_type]

    def export_summary_to_json(self, json_file: str) -> None:
        with open(json_file, "w") as f:
            json.dump(self.get_summary(), f, indent=4)

    def __repr__(self) -> str:
        return json.dumps(self.get_summary(), indent=4)

    # -- persistence: per-read results are materialised, device state dropped ----

    def __getstate__(self):
        reads = self.reads
        state = {k: v for k, v in self.__dict__.items() if k not in ("_result", "_batches", "_host", "_ids")}
        state["_host"] = [(i, rid, e) for i, (rid, e) in enumerate(reads.items())]
        state["_next_index"] = len(reads)
        state["_gpu_stats"] = np.zeros(6, dtype=np.uint64)
        return state

    def __setstate__(self, state):
        if "reads" in state and "_host" not in state:
            # written by the reference (src/kmer.py:536-548, 659-699): its reads
            # dict becomes the host entries, in the same order
            reads = state.pop("reads")
            state["_host"] = [(i, rid, e) for i, (rid, e) in enumerate(reads.items())]
            state["_next_index"] = len(reads)
            state["_gpu_stats"] = np.zeros(6, dtype=np.uint64)
        self.__dict__.update(state)
        self._result = None
        self._batches = []
        self._ids = None

    def save(self, align_file: str) -> None:
        with gzip.open(align_file, "wb") as f:
            pickle.dump(self, f)

    @classmethod
    def load(cls, align_file: str) -> "PseudoAlignment":
        return _load_pickle(align_file)  # (any object, as pickle.load)
