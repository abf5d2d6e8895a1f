"""Lineages: the genomes' places in a taxonomy tree, and the lineage report
(DESIGN.md section 17).  Plain Python: the per-read reduction and the counts
are the device's (pa_native.Lineage); this module builds the tree the device
is given and writes what comes back.
"""

from __future__ import annotations

from typing import Dict, List, Mapping, Optional, Sequence, Tuple

ROOT_NAME = "root"
LINEAGE_HEADER_COLUMNS = ("#taxon", "depth", "genomes", "reads_clade", "reads_direct", "clade_share")
LINEAGE_ABUNDANCE_COLUMNS = ("read_fraction", "abundance")
LINEAGE_KMER_COLUMNS = ("kmers_clade", "kmers_seen_clade", "kmer_containment")
ASSIGNMENTS_TAXON_HEADER = "#read\tmapping\tgenomes\ttaxon\n"


def parse_lineage_line(line: str) -> Optional[Tuple[str, List[str]]]:
    """(identifier, [names root -> leaf]) of one line ``identifier<TAB>name;name;...``,
    None for a blank line or a ``#`` line.  An identifier alone, or one with
    nothing after its tab, has the empty lineage.  ValueError for an empty
    identifier and for an empty name between ``;``."""
    text = line.rstrip("\r\n")
    if not text.strip() or text.lstrip().startswith("#"):
        return None
    ident, tab, rest = text.partition("\t")
    ident = ident.strip()
    if not ident:
        raise ValueError(f"lineage line without an identifier: {text!r}")
    if not tab or not rest.strip():
        return ident, []
    names = [n.strip() for n in rest.split(";")]
    if any(not n for n in names):
        raise ValueError(f"empty name in the lineage of {ident!r}: {rest.strip()!r}")
    return ident, names


class LineageTree:
    """The tree of one index: nodes 0 .. n - 1, node 0 the root, parent[i] < i.
    ``names[v]``: the node's own name; ``genome_node[g]``: genome g's node;
    ``order``: the nodes in depth-first preorder, children in ascending id."""

    def __init__(self, parent: List[int], names: List[str], genome_node: List[int]) -> None:
        self.parent, self.names, self.genome_node = parent, names, genome_node
        n = len(parent)
        self.depth = [0] * n
        kids: List[List[int]] = [[] for _ in range(n)]
        for v in range(1, n):
            self.depth[v] = self.depth[parent[v]] + 1
            kids[parent[v]].append(v)
        self.order: List[int] = []
        stack = [0]
        while stack:
            v = stack.pop()
            self.order.append(v)
            stack.extend(reversed(kids[v]))
        self.genomes_below = [0] * n
        for g in genome_node:
            self.genomes_below[g] += 1
        for v in range(n - 1, 0, -1):
            self.genomes_below[parent[v]] += self.genomes_below[v]
        self._paths: Optional[List[str]] = None

    @property
    def n_nodes(self) -> int:
        return len(self.parent)

    @property
    def paths(self) -> List[str]:
        """Per node the names below the root joined by ``;``; the root: ``root``."""
        if self._paths is None:
            p = [ROOT_NAME] * self.n_nodes
            for v in range(1, self.n_nodes):
                p[v] = self.names[v] if self.parent[v] == 0 else p[self.parent[v]] + ";" + self.names[v]
            self._paths = p
        return self._paths

    def roll_up(self, per_genome: Sequence[float]) -> List[float]:
        """Per node the sum of the genomes' values over its subtree, added in
        ascending genome index, in double."""
        out = [0.0] * self.n_nodes
        for g, node in enumerate(self.genome_node):
            x = float(per_genome[g])
            v = node
            while True:
                out[v] += x
                if v == 0:
                    break
                v = self.parent[v]
        return out


class Lineages:
    """{genome identifier: [names root -> leaf]}.  ``tree(identifiers)`` makes
    the tree of an index: a node is a pair (parent, name), created walking the
    index's genomes in index order and each lineage root -> leaf, so the ids
    ascend from parents to children; every genome gets a node of its own, named
    by its identifier, below the last node of its lineage.  Identifiers the
    index does not hold are ignored; an index genome without a lineage is a
    ValueError."""

    def __init__(self, mapping: Mapping[str, Sequence[str]]) -> None:
        self._m: Dict[str, List[str]] = {}
        for ident, names in mapping.items():
            if isinstance(names, str):
                raise ValueError(f"the lineage of {ident!r} must be a sequence of names, not a string")
            names = [str(n).strip() for n in names]
            if any(not n for n in names):
                raise ValueError(f"empty name in the lineage of {ident!r}")
            self._m[str(ident)] = names

    @classmethod
    def from_file(cls, path: str) -> "Lineages":
        m: Dict[str, List[str]] = {}
        with open(path) as fh:
            for line in fh:
                rec = parse_lineage_line(line)
                if rec is None:
                    continue
                if rec[0] in m:
                    raise ValueError(f"duplicate identifier in lineage file '{path}': {rec[0]}")
                m[rec[0]] = rec[1]
        return cls(m)

    def __contains__(self, ident: str) -> bool:
        return ident in self._m

    def __getitem__(self, ident: str) -> List[str]:
        return list(self._m[ident])

    def __len__(self) -> int:
        return len(self._m)

    def tree(self, identifiers: Sequence[str]) -> LineageTree:
        parent, names, genome_node = [0], [ROOT_NAME], []
        by_pair: Dict[Tuple[int, str], int] = {}
        for ident in identifiers:
            if ident not in self._m:
                raise ValueError(f"no lineage for genome '{ident}'")
            v = 0
            for name in self._m[ident]:
                key = (v, name)
                if key not in by_pair:
                    by_pair[key] = len(parent)
                    parent.append(v)
                    names.append(name)
                v = by_pair[key]
            genome_node.append(len(parent))  # (its own node: never shared, not even with a taxon of that name)
            parent.append(v)
            names.append(ident)
        return LineageTree(parent, names, genome_node)


def _f(x) -> str:
    return format(float(x), ".9g")


def lineage_report_rows(tree: LineageTree, direct: Sequence[int], clade: Sequence[int]) -> List[dict]:
    """One row per node in preorder: taxon, depth, genomes, reads_clade,
    reads_direct, clade_share (reads_clade / classified; 0 when nothing is)."""
    classified = int(clade[0]) if tree.n_nodes else 0
    paths = tree.paths
    return [{"node": v, "taxon": paths[v], "depth": tree.depth[v], "genomes": tree.genomes_below[v],
             "reads_clade": int(clade[v]), "reads_direct": int(direct[v]),
             "clade_share": int(clade[v]) / classified if classified else 0.0} for v in tree.order]


def lineage_report_text(rows: Sequence[dict], reads: int, unmapped: int, dropped: int, abundance=None,
                        containment: bool = False) -> str:
    """The --lineage-report file: the header, one tab-separated line per row
    (lineage_report_rows; floats as format(x, ".9g")) and a last comment line
    with the reads, the classified, unmapped and dropped ones and the nodes.
    ``abundance`` = (iterations, last_delta, classes, bootstrap) when the rows
    hold "read_fraction" and "abundance": those columns are added and the EM's
    settings appended to the last line as abundance_text appends them;
    bootstrap = None or (bootstraps, seed, confidence) when the rows also hold
    the four bootstrap columns.  ``containment``: the rows also hold
    LINEAGE_KMER_COLUMNS, written after every other column."""
    from kmer import ABUNDANCE_BOOTSTRAP_COLUMNS
    cols = list(LINEAGE_HEADER_COLUMNS)
    extra: List[str] = []
    last = ""
    if abundance is not None:
        iterations, last_delta, classes, bootstrap = abundance
        extra = list(LINEAGE_ABUNDANCE_COLUMNS)
        last = f"\titerations\t{int(iterations)}\tlast_delta\t{_f(last_delta)}\tclasses\t{int(classes)}"
        if bootstrap is not None:
            extra += list(ABUNDANCE_BOOTSTRAP_COLUMNS)
            last += f"\tbootstraps\t{int(bootstrap[0])}\tseed\t{int(bootstrap[1])}\tconfidence\t{_f(bootstrap[2])}"
    kmers = list(LINEAGE_KMER_COLUMNS) if containment else []
    lines = ["\t".join(cols + extra + kmers) + "\n"]
    classified = 0
    for r in rows:
        if r["depth"] == 0:
            classified = int(r["reads_clade"])
        out = [str(r["taxon"]), str(int(r["depth"])), str(int(r["genomes"])), str(int(r["reads_clade"])),
               str(int(r["reads_direct"])), _f(r["clade_share"])]
        out += [_f(r[c]) for c in extra]
        if containment:
            out += [str(int(r["kmers_clade"])), str(int(r["kmers_seen_clade"])), _f(r["kmer_containment"])]
        lines.append("\t".join(out) + "\n")
    lines.append(f"#reads\t{int(reads)}\tclassified\t{classified}\tunmapped\t{int(unmapped)}\tdropped\t{int(dropped)}"
                 f"\tnodes\t{len(rows)}{last}\n")
    return "".join(lines)


__all__ = ["Lineages", "LineageTree", "parse_lineage_line", "lineage_report_rows", "lineage_report_text",
           "ROOT_NAME", "LINEAGE_HEADER_COLUMNS", "LINEAGE_ABUNDANCE_COLUMNS", "LINEAGE_KMER_COLUMNS", "ASSIGNMENTS_TAXON_HEADER"]
