"""The host code's scratch holder (pa::Bufs, csrc/pa_internal.h) on the CPU:
tests/host/bufs_main.cpp exercises get / release / the early free / the
destructor's order against a malloc-backed allocator, built with
AddressSanitizer and UBSan as a program of its own (no GPU, no HIP runtime,
nothing loaded into Python)."""

import os
import shutil
import subprocess

import build_native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bufs_holder_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bufs_main")
    hipcc = shutil.which(build_native._hipcc())
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    cmd = [hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           f"-I{build_native.CSRC}", f"-I{build_native.INCLUDE}", f"-I{rocm_include}",
           os.path.join(REPO, "tests", "host", "bufs_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout
    assert "bufs ok" in r.stdout
