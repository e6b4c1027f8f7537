"""BLS12-381 G2 through the C header and the C++ host API: tests/c/bls12_381_g2_caller.c compiles as C99 and links every prototype;
tests/cpp/bls12_381_g2_tests.cpp (the generator in both encodings, 2 G2, the flags, a refused record, both routes of the sum against the lanes) is compiled against
include/ecsimd and run on the GPU, the way tests/test_cpp_bls12_381.py drives its scenario.  The compile-and-link halves run without a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "bls12_381_g2_tests.cpp")
OUT = os.path.join(ROOT, "build", "tests", "bls12_381_g2_tests")
HEADER = os.path.join(ROOT, "include", "ecsimd_bls12_381_g2.h")


def library():
    import ecsimd_amd
    if not os.path.exists(ecsimd_amd.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return ecsimd_amd.lib_path()


def build_binary():
    lib = library()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    libdir = os.path.join(ROOT, "ecsimd_amd")
    newest = max(os.path.getmtime(p) for p in [SRC, os.path.join(ROOT, "tests", "cpp", "mini_test.h"), lib, HEADER] +
                 [os.path.join(ROOT, "include", "ecsimd", f) for f in os.listdir(os.path.join(ROOT, "include", "ecsimd"))])
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"), SRC, "-o", OUT,
                        "-L", libdir, "-lecsimd_hip", "-Wl,-rpath," + libdir], check=True)
    return OUT


def test_the_header_compiles_as_c99_and_every_prototype_links(tmp_path):
    library()
    libdir = os.path.join(ROOT, "ecsimd_amd")
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "bls12_381_g2_caller.c"), "-o", str(exe),
                    "-L", libdir, "-lecsimd_hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True, check=True).stdout
    declared = set(re.findall(r"\b(ecsimd_bls381_g2_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    assert len(declared) == 10
    for s in declared:
        assert re.search(r"\bU %s\b" % s, out), s


def test_the_scenario_compiles_and_links():
    assert os.path.exists(build_binary())


@pytest.mark.gpu
def test_bls12_381_g2_through_the_cpp_api():
    r = subprocess.run([build_binary()], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
