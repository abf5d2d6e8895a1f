"""--assignments on the host: the flag checks and their messages, the line
format, and the early-prefetch guess that must stand back for the flag.  No
device call is made: every command below ends in its flag check."""

import os
import stat
import subprocess
import sys

import pytest

from conftest import GOLDEN, PKG

MAIN = os.path.join(PKG, "main.py")
FA = os.path.join(GOLDEN, "config1.fa")
FQ = os.path.join(GOLDEN, "config1.fq")
ONLY = "Error: --assignments is only allowed for task 'dumpalign' with --reads."


def run_main(argv, cwd):
    return subprocess.run([sys.executable, MAIN] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                          timeout=120, cwd=str(cwd))


@pytest.mark.parametrize("argv", [
    ["-t", "dumpalign", "-a", "x.aln", "--assignments", "out.tsv"],
    ["-t", "dumpref", "-g", FA, "-k", "21", "--assignments", "out.tsv"],
    ["-t", "reference", "-g", FA, "-k", "21", "-r", "x.kdb", "--assignments", "out.tsv"],
    ["-t", "align", "-g", FA, "-k", "21", "--reads", FQ, "-a", "x.aln", "-r", "x.kdb", "--assignments=out.tsv"],
], ids=["no_reads", "dumpref", "reference", "align"])
def test_flag_on_the_wrong_job(argv, tmp_path):
    r = run_main(argv, tmp_path)
    assert r.returncode != 0 and r.stdout == ""
    assert r.stderr.strip() == ONLY
    assert not os.path.exists(tmp_path / "out.tsv")


def test_unwritable_file(tmp_path):
    if os.geteuid() == 0:
        # (root writes anywhere: a directory that does not exist is unwritable for everyone)
        target = str(tmp_path / "missing" / "out.tsv")
        want = f"Error: Directory '{os.path.dirname(target)}' is not writable to create Assignments output file '{target}'."
    else:
        target = str(tmp_path / "out.tsv")
        open(target, "w").close()
        os.chmod(target, stat.S_IRUSR)
        want = f"Error: Assignments output file '{target}' is not writable."
    r = run_main(["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--assignments", target], tmp_path)
    assert r.returncode != 0 and r.stdout == ""
    assert r.stderr.strip() == want


def test_parse_arguments():
    import main
    a = main.parse_arguments(["-t", "dumpalign", "-g", "x.fa", "-k", "21", "--reads", "r.fq", "--assignments", "o.tsv"])
    assert a.assignments == "o.tsv"
    b = main.parse_arguments(["-t", "dumpalign", "-g", "x.fa", "-k", "21", "--reads", "r.fq"])
    assert b.assignments is None


def test_assignment_line():
    import kmer
    assert kmer.ASSIGNMENTS_HEADER == "#read\tmapping\tgenomes\n"
    assert kmer.assignment_line("r1", 2, ["gA"]) == "r1\tunique\tgA\n"
    assert kmer.assignment_line("r2", 3, []) == "r2\tambiguous\t\n"
    assert kmer.assignment_line("r3", 3, ["gA", "gB", "gA"]) == "r3\tambiguous\tgA,gB,gA\n"  # (a p-demoted list)
    assert kmer.assignment_line("r4", 1, []) == "r4\tunmapped\t\n"
    assert kmer.assignment_line("r5", 0, []) == "r5\tfiltered\t\n"
    # the list is written for unique and ambiguous reads only
    assert kmer.assignment_line("r6", 1, ["gA"]) == "r6\tunmapped\t\n"
    assert kmer.assignment_line("r7", 0, ["gA"]) == "r7\tfiltered\t\n"
    assert kmer.assignment_line("r8", kmer.ReadMappingType.UNIQUELY_MAPPED.value, ("g",)) == "r8\tunique\tg\n"


@pytest.mark.parametrize("flag", [["--assignments", "o.tsv"], ["--assignments=o.tsv"], ["--assign", "o.tsv"],
                                  ["--assi=o.tsv"]], ids=["spaced", "equals", "prefix", "prefix_equals"])
def test_early_prefetch_stands_back(flag, monkeypatch):
    import main
    for v in ("PA_GPUS", "PA_STREAM", "PA_PREFETCH"):
        monkeypatch.delenv(v, raising=False)
    base = ["-t", "dumpalign", "-g", "x.fa", "-k", "21", "--reads", "r.fq"]
    assert main._early_reads_path(base) == "r.fq"
    assert main._early_reads_path(base + flag) is None
    assert main._early_reads_path(flag + base) is None
