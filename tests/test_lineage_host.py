"""Lineages on the host: the model the GPU tests compare
the device with, pinned against cases worked out by hand; the lineage file's
parser and the tree it makes; the report's text; the --lineages flag checks
(main.py in a child process, no device needed); the tree's host code
(csrc/pa_tree.h) as a program of its own under AddressSanitizer and UBSan.

The model is plain Python and does not use the preorder trick: a node set's
lowest common ancestor is the last node of the common prefix of the members'
root paths.  Types and sets come from test_abundance_host's model.  Nothing
from libpa feeds it.
"""

import collections
import os
import re
import shutil
import subprocess
import sys

import pytest

import test_abundance_host as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "bioinformatics-project-for-shotgun-metagenomics-pseudo-alignment-shotgun-_amd")
MAIN = os.path.join(PKG, "main.py")
GOLD = os.path.join(REPO, "tests", "golden")
FA, FQ = os.path.join(GOLD, "config1.fa"), os.path.join(GOLD, "config1.fq")

NO_NODE = 0xFFFFFFFF


# ---- the model --------------------------------------------------------------------------------

def root_path(parent, v):
    """[root, ..., v]"""
    path = [v]
    while v != 0:
        v = parent[v]
        path.append(v)
    return path[::-1]


def lca(parent, nodes):
    """The lowest common ancestor of a non-empty node collection: the end of the root paths' common prefix."""
    paths = [root_path(parent, v) for v in nodes]
    v = 0
    for level in zip(*paths):
        if any(x != level[0] for x in level):
            break
        v = level[0]
    return v


def node_of(parent, genome_node, t, C):
    """node(r) of a read of type t and compatibility set C."""
    if t not in (M.UNIQUE, M.AMBIGUOUS) or not C:
        return NO_NODE
    return lca(parent, [genome_node[g] for g in C])


def nodes_of(parent, genome_node, types, sets):
    return [node_of(parent, genome_node, t, C) for t, C in zip(types, sets)]


def counts_of(parent, nodes):
    """(direct, clade) of a batch's per-read nodes."""
    n = len(parent)
    direct, clade = [0] * n, [0] * n
    for v in nodes:
        if v != NO_NODE:
            direct[v] += 1
            for a in root_path(parent, v):
                clade[a] += 1
    return direct, clade


def preorder(parent):
    kids = collections.defaultdict(list)
    for v in range(1, len(parent)):
        kids[parent[v]].append(v)
    out = []

    def walk(v):
        out.append(v)
        for c in kids[v]:
            walk(c)
    walk(0)
    return out


def model_tree(identifiers, lineages):
    """(parent, names, genome_node) as section 17 numbers them: the index's genomes in
    order, each lineage root -> leaf, a node per new (parent, name), then the genome's own."""
    parent, names, genome_node, seen = [0], ["root"], [], {}
    for ident in identifiers:
        v = 0
        for name in lineages[ident]:
            if (v, name) not in seen:
                seen[(v, name)] = len(parent)
                parent.append(v)
                names.append(name)
            v = seen[(v, name)]
        genome_node.append(len(parent))
        parent.append(v)
        names.append(ident)
    return parent, names, genome_node


def f9(x):
    return format(float(x), ".9g")


def report_text(parent, names, genome_node, nodes, unmapped, dropped, per_genome=None, last=""):
    """The --lineage-report file from the model's per-read nodes; per_genome: columns of
    per-genome values, each summed over every node's subtree in ascending genome index."""
    direct, clade = counts_of(parent, nodes)
    cols = ["#taxon", "depth", "genomes", "reads_clade", "reads_direct", "clade_share"]
    out = []
    for v in preorder(parent):
        path = root_path(parent, v)
        below = [g for g, gv in enumerate(genome_node) if v in root_path(parent, gv)]
        row = ["root" if v == 0 else ";".join(names[a] for a in path[1:]), str(len(path) - 1), str(len(below)),
               str(clade[v]), str(direct[v]), f9(clade[v] / clade[0] if clade[0] else 0.0)]
        for _, values in per_genome or []:
            s = 0.0
            for g in below:
                s += float(values[g])
            row.append(f9(s))
        out.append("\t".join(row) + "\n")
    head = "\t".join(cols + [c for c, _ in per_genome or []]) + "\n"
    tail = (f"#reads\t{len(nodes)}\tclassified\t{clade[0]}\tunmapped\t{unmapped}\tdropped\t{dropped}"
            f"\tnodes\t{len(parent)}{last}\n")
    return head + "".join(out) + tail


# ---- the model by hand ------------------------------------------------------------------------

#        0
#      /   \
#     1     2          genomes: g0 -> 3, g1 -> 4, g2 -> 4 (shared), g3 -> 1 (internal), g4 -> 5, g5 -> 0 (the root)
#    / \     \
#   3   4     5
HAND_PARENT = [0, 0, 0, 1, 1, 2]
HAND_GENOME_NODE = [3, 4, 4, 1, 5, 0]


@pytest.mark.parametrize("C, want", [
    ((0, 1), 1),        # two siblings: their parent
    ((0, 3), 1),        # a node and its own ancestor: the ancestor
    ((1, 2), 4),        # genomes sharing a node: that node
    ((3,), 1),          # a set of one, on an internal node
    ((1,), 4),          # a set of one, on a leaf
    ((0, 4), 0),        # across the root's children: the root
    ((0, 1, 2, 3), 1),
    ((4, 5), 0),        # a genome on the root
    ((), NO_NODE),      # the empty set
], ids=["siblings", "ancestor", "shared_node", "internal_single", "leaf_single", "root", "clade", "root_genome",
        "empty"])
def test_model_lca_by_hand(C, want):
    t = M.UNIQUE if len(C) == 1 else M.AMBIGUOUS
    assert node_of(HAND_PARENT, HAND_GENOME_NODE, t, C) == want


def test_model_types_and_counts_by_hand():
    assert node_of(HAND_PARENT, HAND_GENOME_NODE, M.UNMAPPED, ()) == NO_NODE
    assert node_of(HAND_PARENT, HAND_GENOME_NODE, M.DROPPED, ()) == NO_NODE
    nodes = [3, 3, 1, 4, 0, NO_NODE, 5]
    direct, clade = counts_of(HAND_PARENT, nodes)
    assert direct == [1, 1, 0, 2, 1, 1] and clade == [6, 4, 1, 2, 1, 1]
    assert preorder(HAND_PARENT) == [0, 1, 3, 4, 2, 5]
    assert root_path(HAND_PARENT, 5) == [0, 2, 5] and root_path(HAND_PARENT, 0) == [0]


def test_model_nodes_from_classify_all():
    """Types and sets from test_abundance_host's model (its three genomes sharing ACGTAC), nodes from this one."""
    k = 5
    a, b, c = "AACCGGTTACGTAC", "TTGGACGTACCATG", "GGATCACGTACTCA"
    kd = M.kmer_sets([a, b, c], False, k)
    seqs = ["ACGTAC", "AACCGG", "ACGT", "AACCGG", "TTGGAC"]
    quals = ["IIIIII", "IIIIII", "IIII", "######", "IIIIII"]
    types, sets, _ = M.classify_all(kd, k, seqs, quals, mrq=40)
    assert types == [M.AMBIGUOUS, M.UNIQUE, M.UNMAPPED, M.DROPPED, M.UNIQUE]
    assert sets == [(0, 1, 2), (0,), (), (), (1,)]
    parent, genome_node = [0, 0, 1, 1, 0], [2, 3, 4]     # a species of g0 and g1; g2 off the root
    nodes = nodes_of(parent, genome_node, types, sets)
    assert nodes == [0, 2, NO_NODE, NO_NODE, 3]
    assert node_of(parent, genome_node, M.AMBIGUOUS, (0, 1)) == 1
    assert counts_of(parent, nodes) == ([1, 0, 1, 1, 0], [3, 2, 1, 1, 0])


# ---- the lineage file and the tree --------------------------------------------------------------

def test_lineages_tree_ids():
    from lineage import Lineages
    lin = {"gB": ["Bacteria", "Esch", "coli"], "gA": ["Bacteria", "Esch", "coli"], "gC": ["Bacteria", "Salm"],
           "gD": [], "gX": ["Archaea"], "unused": ["Bacteria", "Other"]}
    ids = ["gA", "gB", "gC", "gD", "gX"]
    tree = Lineages(lin).tree(ids)
    parent, names, genome_node = model_tree(ids, lin)
    assert (tree.parent, tree.names, tree.genome_node) == (parent, names, genome_node)
    assert names == ["root", "Bacteria", "Esch", "coli", "gA", "gB", "Salm", "gC", "gD", "Archaea", "gX"]
    assert parent == [0, 0, 1, 2, 3, 3, 1, 6, 0, 0, 9]
    assert all(parent[i] < i for i in range(1, len(parent))) and parent[0] == 0
    assert genome_node == [4, 5, 7, 8, 10]          # every genome a node of its own; gD hangs off the root
    assert "Other" not in names                        # a lineage of a genome the index lacks makes no node
    assert tree.order == preorder(parent)
    assert tree.paths[5] == "Bacteria;Esch;coli;gB" and tree.paths[0] == "root" and tree.paths[8] == "gD"
    assert tree.depth == [0, 1, 2, 3, 4, 4, 2, 3, 1, 1, 2]
    assert tree.genomes_below == [5, 3, 2, 2, 1, 1, 1, 1, 1, 1, 1]
    # the order of the index's genomes gives the ids
    other = Lineages(lin).tree(["gX", "gA"])
    assert other.names == ["root", "Archaea", "gX", "Bacteria", "Esch", "coli", "gA"]
    # a genome named like a taxon under the same parent still gets its own node
    twin = Lineages({"coli": ["Esch"], "g2": ["Esch", "coli"]}).tree(["coli", "g2"])
    assert twin.names == ["root", "Esch", "coli", "coli", "g2"] and twin.parent == [0, 0, 1, 1, 3]
    assert twin.roll_up([0.25, 0.5]) == [0.75, 0.75, 0.25, 0.5, 0.5]


def test_lineage_file(tmp_path):
    from lineage import Lineages, parse_lineage_line
    assert parse_lineage_line("g1\tA;B;C\n") == ("g1", ["A", "B", "C"])
    assert parse_lineage_line("g one\t A ; B b\r\n") == ("g one", ["A", "B b"])
    assert parse_lineage_line("g1\n") == ("g1", []) and parse_lineage_line("g1\t\n") == ("g1", [])
    assert parse_lineage_line("\n") is None and parse_lineage_line("   \n") is None
    assert parse_lineage_line("# a comment\tx;y\n") is None
    for bad in ("g1\tA;;B\n", "g1\tA;B;\n", "g1\t;A\n", "\tA;B\n"):
        with pytest.raises(ValueError):
            parse_lineage_line(bad)
    p = tmp_path / "lin.tsv"
    p.write_text("# genome\tlineage\n\ng1\tBacteria;Esch\ng2\tBacteria;Esch\nextra\tArchaea;X\ng3\n")
    lin = Lineages.from_file(str(p))
    assert len(lin) == 4 and "extra" in lin and lin["g3"] == [] and lin["g1"] == ["Bacteria", "Esch"]
    tree = lin.tree(["g1", "g2", "g3"])                    # (extra: ignored, so one file serves --filter-similar runs)
    assert tree.names == ["root", "Bacteria", "Esch", "g1", "g2", "g3"] and tree.parent == [0, 0, 1, 2, 2, 0]
    with pytest.raises(ValueError, match="no lineage for genome 'g4'"):
        lin.tree(["g1", "g4"])
    p.write_text("g1\tA\ng2\tB\ng1\tA\n")
    with pytest.raises(ValueError, match="duplicate identifier"):
        Lineages.from_file(str(p))
    p.write_text("g1\tA;;B\n")
    with pytest.raises(ValueError, match="empty name"):
        Lineages.from_file(str(p))
    with pytest.raises(ValueError):
        Lineages({"g1": ["A", ""]})
    with pytest.raises(ValueError):
        Lineages({"g1": "A;B"})


# ---- the report's text ---------------------------------------------------------------------------

REPORT_LIN = {"gA": ["Esch", "coli"], "gB": ["Esch", "coli"], "gC": ["Esch"], "gD": []}
REPORT_IDS = ["gA", "gB", "gC", "gD"]
# nodes: 0 root, 1 Esch, 2 coli, 3 gA, 4 gB, 5 gC, 6 gD
REPORT_NODES = [3, 3, 2, 2, 2, 1, 5, 0, NO_NODE, NO_NODE, NO_NODE]   # 8 classified, 2 unmapped, 1 dropped


def _report_rows():
    from lineage import Lineages, lineage_report_rows
    tree = Lineages(REPORT_LIN).tree(REPORT_IDS)
    direct, clade = counts_of(tree.parent, REPORT_NODES)
    return tree, lineage_report_rows(tree, direct, clade)


def test_report_text_plain():
    from lineage import lineage_report_text
    tree, rows = _report_rows()
    text = lineage_report_text(rows, 11, 2, 1)
    assert text == ("#taxon\tdepth\tgenomes\treads_clade\treads_direct\tclade_share\n"
                    "root\t0\t4\t8\t1\t1\n"
                    "Esch\t1\t3\t7\t1\t0.875\n"
                    "Esch;coli\t2\t2\t5\t3\t0.625\n"
                    "Esch;coli;gA\t3\t1\t2\t2\t0.25\n"
                    "Esch;coli;gB\t3\t1\t0\t0\t0\n"
                    "Esch;gC\t2\t1\t1\t1\t0.125\n"
                    "gD\t1\t1\t0\t0\t0\n"
                    "#reads\t11\tclassified\t8\tunmapped\t2\tdropped\t1\tnodes\t7\n")
    parent, names, genome_node = model_tree(REPORT_IDS, REPORT_LIN)
    assert text == report_text(parent, names, genome_node, REPORT_NODES, 2, 1)
    # nothing classified: every share is 0
    from lineage import lineage_report_rows
    empty = lineage_report_text(lineage_report_rows(tree, [0] * 7, [0] * 7), 3, 2, 1)
    assert empty.splitlines()[1] == "root\t0\t4\t0\t0\t0" and empty.endswith(
        "#reads\t3\tclassified\t0\tunmapped\t2\tdropped\t1\tnodes\t7\n")


def test_report_text_with_abundance_and_bootstraps():
    from kmer import bootstrap_summary
    from lineage import lineage_report_text
    tree, rows = _report_rows()
    theta, share = [0.5, 0.125, 0.25, 0.125], [0.25, 0.25, 0.375, 0.125]
    rt, rs = tree.roll_up(theta), tree.roll_up(share)
    assert rt == [1.0, 0.875, 0.625, 0.5, 0.125, 0.25, 0.125]
    for r in rows:
        r["read_fraction"], r["abundance"] = rt[r["node"]], rs[r["node"]]
    text = lineage_report_text(rows, 11, 2, 1, (12, 1.5e-10, 3, None))
    assert text == ("#taxon\tdepth\tgenomes\treads_clade\treads_direct\tclade_share\tread_fraction\tabundance\n"
                    "root\t0\t4\t8\t1\t1\t1\t1\n"
                    "Esch\t1\t3\t7\t1\t0.875\t0.875\t0.875\n"
                    "Esch;coli\t2\t2\t5\t3\t0.625\t0.625\t0.5\n"
                    "Esch;coli;gA\t3\t1\t2\t2\t0.25\t0.5\t0.25\n"
                    "Esch;coli;gB\t3\t1\t0\t0\t0\t0.125\t0.25\n"
                    "Esch;gC\t2\t1\t1\t1\t0.125\t0.25\t0.375\n"
                    "gD\t1\t1\t0\t0\t0\t0.125\t0.125\n"
                    "#reads\t11\tclassified\t8\tunmapped\t2\tdropped\t1\tnodes\t7"
                    "\titerations\t12\tlast_delta\t1.5e-10\tclasses\t3\n")
    # two replicates of the genomes' abundances, rolled up replicate by replicate, then summarised per node
    reps = [[0.25, 0.25, 0.375, 0.125], [0.5, 0.0, 0.25, 0.25]]
    rolled = [tree.roll_up(r) for r in reps]
    assert rolled[1] == [1.0, 0.75, 0.5, 0.5, 0.0, 0.25, 0.25]
    summary = bootstrap_summary(rolled, 0.9)
    for r in rows:
        r.update(zip(("abundance_mean", "abundance_sd", "abundance_lo", "abundance_hi"), summary[r["node"]]))
    text = lineage_report_text(rows, 11, 2, 1, (12, 1.5e-10, 3, (2, 7, 0.9)))
    lines = text.splitlines()
    assert lines[0] == ("#taxon\tdepth\tgenomes\treads_clade\treads_direct\tclade_share\tread_fraction\tabundance"
                        "\tabundance_mean\tabundance_sd\tabundance_lo\tabundance_hi")
    # coli: replicates 0.5 and 0.5; gB: 0.25 and 0 (mean 0.125, sd = sqrt(2 * 0.125^2) = 0.176776695)
    assert lines[3] == "Esch;coli\t2\t2\t5\t3\t0.625\t0.625\t0.5\t0.5\t0\t0.5\t0.5"
    assert lines[5] == "Esch;coli;gB\t3\t1\t0\t0\t0\t0.125\t0.25\t0.125\t0.176776695\t0\t0.25"
    assert lines[1] == "root\t0\t4\t8\t1\t1\t1\t1\t1\t0\t1\t1"
    assert lines[-1] == ("#reads\t11\tclassified\t8\tunmapped\t2\tdropped\t1\tnodes\t7\titerations\t12\tlast_delta"
                         "\t1.5e-10\tclasses\t3\tbootstraps\t2\tseed\t7\tconfidence\t0.9")


# ---- the binding table and the header -------------------------------------------------------------

def test_binding_and_header_constants():
    import pa_native as N
    for name in ("pa_lineage_create", "pa_lineage_reset", "pa_lineage_add", "pa_lineage_counts", "pa_lineage_lca",
                 "pa_lineage_free"):
        assert name in N.EXPORTS and hasattr(N.lib(), name)
    text = open(os.path.join(REPO, "include", "pa.h")).read()
    m = re.search(r"#define PA_LINEAGE_LDS_NODES (\d+)", text)
    assert m and int(m.group(1)) == N.LINEAGE_LDS_NODES
    m = re.search(r"#define PA_NO_NODE 0x([0-9A-Fa-f]+)u", text)
    assert m and int(m.group(1), 16) == N.NO_NODE == NO_NODE
    assert N.ctypes.sizeof(N.LineageInfo) == 40
    import build_native
    assert "pa_lineage.hip" in build_native.SOURCES and "pa_tree.h" in build_native.HEADERS


def test_tree_host_code_under_sanitizers(tmp_path):
    """csrc/pa_tree.h (validation, preorder, climb, clade sums) against brute force, as a stand-alone program."""
    import build_native
    exe = str(tmp_path / "tree_main")
    cxx = shutil.which(build_native._hipcc())
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", f"-I{build_native.CSRC}",
           os.path.join(REPO, "tests", "host", "tree_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout
    assert "tree ok" in r.stdout


# ---- the flag checks ----------------------------------------------------------------------------

def test_parse_arguments_accepts_lineage_flags():
    import main
    base = ["-t", "dumpalign", "-g", "x.fa", "-k", "21", "--reads", "r.fq"]
    a = main.parse_arguments(base + ["--lineages", "l.tsv", "--lineage-report", "rep.tsv"])
    assert (a.lineages, a.lineage_report) == ("l.tsv", "rep.tsv")
    a = main.parse_arguments(base + ["--lineages=l.tsv", "--lineage-r", "rep.tsv"])
    assert (a.lineages, a.lineage_report) == ("l.tsv", "rep.tsv")
    b = main.parse_arguments(base)
    assert (b.lineages, b.lineage_report) == (None, None)
    # no abbreviation that worked before became ambiguous
    c = main.parse_arguments(["--ta", "dumpalign", "-g", "x.fa", "-k", "21", "--reads", "r.fq", "--c"])
    assert c.task == "dumpalign" and c.coverage is True
    assert main._has_lineage_flag(["--lineages=l.tsv"]) and main._has_lineage_flag(["--lineage-rep", "x"])
    assert main._has_lineage_flag(["--l", "x"]) and not main._has_lineage_flag(base)
    # a lineage job takes the host-parsed path: no early prefetch of the reads file
    assert main._early_reads_path(base) == "r.fq"
    assert main._early_reads_path(base + ["--lineages", "l.tsv", "--lineage-report", "r.tsv"]) is None


def _lineage_files(tmp_path):
    good = tmp_path / "good.tsv"
    good.write_text("x\tA;B\n")
    dup = tmp_path / "dup.tsv"
    dup.write_text("x\tA\nx\tB\n")
    empty = tmp_path / "empty.tsv"
    empty.write_text("x\tA;;B\n")
    return str(good), str(dup), str(empty)


MISUSE = [
    (lambda g, d, e: ["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--lineage-report", "r.tsv"],
     "--lineage-report needs --lineages"),
    (lambda g, d, e: ["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--lineages", g],
     "--lineages needs --lineage-report"),
    (lambda g, d, e: ["-t", "dumpalign", "-a", "x.aln", "--lineages", g, "--lineage-report", "r.tsv"],
     "only allowed for task 'dumpalign' with --reads"),
    (lambda g, d, e: ["-t", "dumpref", "-g", FA, "-k", "21", "--lineages", g, "--lineage-report", "r.tsv"],
     "only allowed for task 'dumpalign'"),
    (lambda g, d, e: ["-t", "reference", "-g", FA, "-k", "21", "-r", "x.kdb", "--lineages", g, "--lineage-report",
                      "r.tsv"], "only allowed for task"),
    (lambda g, d, e: ["-t", "align", "-g", FA, "-k", "21", "--reads", FQ, "-a", "x.aln", "-r", "x.kdb", "--lineages",
                      g, "--lineage-report", "r.tsv"], "only allowed for task"),
    (lambda g, d, e: ["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--reads2", FQ, "--lineages", g,
                      "--lineage-report", "r.tsv"], "--reads2 cannot be combined with --lineages"),
    (lambda g, d, e: ["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--lineages", "no_such.tsv",
                      "--lineage-report", "r.tsv"], "does not exist"),
    (lambda g, d, e: ["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--lineages", g, "--lineage-report",
                      "no_such_dir/r.tsv"], "Error:"),
    (lambda g, d, e: ["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--lineages", d, "--lineage-report",
                      "r.tsv"], "duplicate identifier"),
    (lambda g, d, e: ["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--lineages", e, "--assignments",
                      "a.tsv"], "empty name"),
]


@pytest.mark.parametrize("make, message", MISUSE,
                         ids=["report_alone", "lineages_alone", "alignfile", "dumpref", "reference", "align", "reads2",
                              "unreadable", "unwritable", "duplicate", "empty_name"])
def test_cli_lineage_misuse(make, message, tmp_path):
    """The flag checks and the lineage file's parser end the process before any device work."""
    argv = make(*_lineage_files(tmp_path))
    r = subprocess.run([sys.executable, MAIN] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=60, cwd=str(tmp_path), env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode != 0 and r.stdout == ""
    err = r.stderr.strip()
    assert err.startswith("Error:") and len(err.splitlines()) == 1 and message in err
