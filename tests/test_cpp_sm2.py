"""The SM2 signature scheme through the C++ host API: tests/cpp/sm2_tests.cpp (the signature example of GB/T 32918.2 -- the record the fixture holds as "example" --
through hip::sm3, sm2_pubkey, sm2_digest, sm2_sign_digest, sm2_verify and sm2_verify_digest on curve_sm2, refused keys through ok) compiled against
include/ecsimd and run on the GPU, the way tests/test_cpp_p384.py drives its scenario.  The link-only half runs without a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sm2_tests.cpp")
OUT = os.path.join(ROOT, "build", "tests", "sm2_tests")


def build_binary():
    import ecsimd_amd
    if not os.path.exists(ecsimd_amd.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    libdir = os.path.join(ROOT, "ecsimd_amd")
    newest = max(os.path.getmtime(p) for p in [SRC, os.path.join(ROOT, "tests", "cpp", "mini_test.h"), ecsimd_amd.lib_path()] +
                 [os.path.join(ROOT, "include", "ecsimd", f) for f in os.listdir(os.path.join(ROOT, "include", "ecsimd"))] + [os.path.join(ROOT, "include", "ecsimd_sm2.h")])
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"), SRC, "-o", OUT,
                        "-L", libdir, "-lecsimd_hip", "-Wl,-rpath," + libdir], check=True)
    return OUT


def test_the_scenario_compiles_and_links():
    assert os.path.exists(build_binary())


@pytest.mark.gpu
def test_sm2_through_the_cpp_api():
    r = subprocess.run([build_binary()], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
