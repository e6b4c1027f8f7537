"""The number-theoretic transform's index arithmetic on a CPU, and its C++ host API.  tests/cpp/ntt_host_check.cpp runs ecsimd_amd/csrc/ntt.cuh's pass body lane
by lane over the portable field -- every schedule the radix cap reaches at 2 .. 2^13 elements, subgroup and cosets, batches that share a tile and leave the
last one ragged, in place and out of place -- against tools/ntt_model.py's transforms; it is a stand-alone program, built here with -fsanitize=address,undefined
so that an index outside a buffer or the LDS image stops it.  tests/cpp/ntt_tests.cpp drives include/ecsimd/ntt.h; its link-only half runs without a GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ntt_model as model   # noqa: E402

CHECK_SRC = os.path.join(ROOT, "tests", "cpp", "ntt_host_check.cpp")
SRC = os.path.join(ROOT, "tests", "cpp", "ntt_tests.cpp")
OUT = os.path.join(ROOT, "build", "tests", "ntt_tests")


def test_the_pass_body_equals_the_model_on_a_cpu_under_the_sanitizers(tmp_path):
    exe, cases = tmp_path / "ntt_host_check", tmp_path / "cases.txt"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", CHECK_SRC, "-o", str(exe)], check=True)
    cases.write_text(model.host_check_cases(log_ns=range(1, 14)))
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    cases_run, transforms, failures = (int(w) for w in r.stdout.split("\n")[-2].replace(",", "").split() if w.isdigit())
    assert failures == 0 and cases_run == 25 and transforms == 25 * 20           # ten schedules in place and the default out of place, forward and inverse


def test_the_check_sees_a_wrong_transform(tmp_path):
    exe, cases = tmp_path / "ntt_host_check", tmp_path / "cases.txt"
    subprocess.run(["g++", "-std=c++17", "-O1", CHECK_SRC, "-o", str(exe)], check=True)
    text = model.host_check_cases(log_ns=(3,)).split("\n")
    text[-2] = "%x" % ((int(text[-2], 16) + 1) % model.FR)                         # the last expected output, off by one
    cases.write_text("\n".join(text))
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "FAIL forward" in r.stdout


def build_binary():
    import ecsimd_amd
    if not os.path.exists(ecsimd_amd.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    libdir = os.path.join(ROOT, "ecsimd_amd")
    newest = max(os.path.getmtime(p) for p in [SRC, os.path.join(ROOT, "tests", "cpp", "mini_test.h"), ecsimd_amd.lib_path()] +
                 [os.path.join(ROOT, "include", "ecsimd", f) for f in os.listdir(os.path.join(ROOT, "include", "ecsimd"))] + [os.path.join(ROOT, "include", "ecsimd_ntt.h")])
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"), SRC, "-o", OUT,
                        "-L", libdir, "-lecsimd_hip", "-Wl,-rpath," + libdir], check=True)
    return OUT


def test_the_scenario_compiles_and_links():
    assert os.path.exists(build_binary())


@pytest.mark.gpu
def test_ntt_through_the_cpp_api():
    r = subprocess.run([build_binary()], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
