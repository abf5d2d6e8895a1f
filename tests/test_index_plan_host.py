"""The index build's sizing plan (csrc/pa_index_plan.h) and the ownership list
of an index's align-side view (release_align_view, csrc/pa_internal.h) on the
CPU: tests/host/index_plan_main.cpp checks hand-derived capacities, Bloom and
neighbour-word choices at sizes no GPU test reaches (C5: 8 G windows in
288 GB) and the release against a malloc-backed allocator, built with
AddressSanitizer and UBSan as a program of its own (no GPU, no HIP runtime,
nothing loaded into Python)."""

import os
import shutil
import subprocess

import build_native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_index_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "index_plan_main")
    hipcc = shutil.which(build_native._hipcc())
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    cmd = [hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           f"-I{build_native.CSRC}", f"-I{build_native.INCLUDE}", f"-I{rocm_include}",
           os.path.join(REPO, "tests", "host", "index_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout
    assert "index plan ok" in r.stdout


def test_plan_header_is_host_only_and_hashed():
    """No HIP, no environment and no allocation in the plan; the library's source hash covers it."""
    with open(os.path.join(build_native.CSRC, "pa_index_plan.h")) as f:
        text = f.read()
    for word in ("hip/", "getenv", "malloc", "__device__", "__global__"):
        assert word not in text, word
    assert "pa_index_plan.h" in build_native.HEADERS
