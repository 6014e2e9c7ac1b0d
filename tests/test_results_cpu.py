"""The host's per-slot results without a GPU: libreasr_amd/csrc/lasr_results.hip.h (what both decode protocols and every fetch call go
through) under AddressSanitizer + UndefinedBehaviorSanitizer, against the plain-vector restatement in tests/c/results_check.cpp."""
import os
import shutil
import subprocess


def test_result_store_under_asan_ubsan(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx, "g++ is part of the image"
    exe = str(tmp_path / "results_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(root, "tests", "c", "results_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "results_check: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
