"""CPU suite for Keccak-256 / Ethereum addresses: the host model, the golden file, the C ABI's new symbols, and what the shipped gfx950 listing of
k_keccak.hip must keep (no scratch, no branch beyond the bounds exit and the block loop, the permutation's size).

The model (tools/keccak_model.py) is pinned in two steps, because nothing on a stock Python offers Keccak-256 itself: with pad byte 0x06 it IS SHA3-256, which
hashlib has -- that checks the permutation, the rate and the sponge at every length; the pad byte 0x01 is then pinned by published known answers."""
import hashlib
import json
import os
import random
import re
import subprocess
import sys

import pytest

from helpers import CURVE_PARAMS, SECP256K1, ec_mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import keccak_listing  # noqa: E402
import keccak_model as model  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "keccak256_vectors.json")
PROFILE = os.path.join(ROOT, "profiles", "r08", "keccak_eth.txt")
G = (CURVE_PARAMS[SECP256K1]["gx"], CURVE_PARAMS[SECP256K1]["gy"])


def test_the_model_with_sha3_padding_is_sha3_256_at_every_length():
    rng = random.Random(20261017)
    for length in list(range(0, 301)) + [135, 136, 137, 271, 272, 273, 1000]:
        m = bytes(rng.randrange(256) for _ in range(length))
        assert model.sponge256(m, 0x06) == hashlib.sha3_256(m).digest(), length


def test_known_answers_pin_the_pad_byte():
    assert model.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert model.keccak256(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
    assert model.keccak256(b"") != hashlib.sha3_256(b"").digest()
    for d, address in ((1, "7e5f4552091a69125d5dfcb7b8c2659029395bdf"), (2, "2b5ad5c4795c026514f8317c7a215e218dccd6cf"), (3, "6813eb9362372eef6200f3b1dbc3f819671cba69")):
        assert model.eth_address(*ec_mul(SECP256K1, d, G)).hex() == address


def test_the_round_constants_are_the_published_ones():
    assert model.RC[0] == 1 and model.RC[1] == 0x8082 and model.RC[23] == 0x8000000080008008 and len(set(model.RC)) == 22      # (two values occur twice)


def test_the_golden_file_holds_data_only_and_agrees_with_the_model():
    g = json.load(open(GOLDEN))
    assert set(g) == {"comment", "digests", "addresses"}
    assert len(g["digests"]) >= 30 and len(g["addresses"]) >= 10
    assert g["digests"][0] == {"msg": "", "keccak256": "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"}
    assert g["digests"][1] == {"msg": b"abc".hex(), "keccak256": "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"}
    for row in g["digests"]:
        assert model.keccak256(bytes.fromhex(row["msg"])).hex() == row["keccak256"]
    assert [a["address"] for a in g["addresses"][:3]] == ["7e5f4552091a69125d5dfcb7b8c2659029395bdf", "2b5ad5c4795c026514f8317c7a215e218dccd6cf", "6813eb9362372eef6200f3b1dbc3f819671cba69"]
    for a in g["addresses"]:
        x, y = ec_mul(SECP256K1, int(a["d"], 16), G)
        assert (x, y) == (int(a["x"], 16), int(a["y"], 16))
        assert model.eth_address(x, y).hex() == a["address"]


# ---- the C ABI and the package
NEW_SYMBOLS = ["ecsimd_hip_keccak256", "ecsimd_hip_eth_address", "ecsimd_hip_eth_recover"]


def test_the_three_symbols_are_declared_and_exported():
    import ecsimd_amd
    from ecsimd_amd.engine import declared_symbols
    for s in NEW_SYMBOLS:
        assert s in declared_symbols(), s
    if not os.path.exists(ecsimd_amd.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.run(["nm", "-D", "--defined-only", ecsimd_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (ecsimd_hip_\w+)", out))
    for s in NEW_SYMBOLS:
        assert s in exported, s


def test_the_flag_and_the_methods_are_public():
    import ecsimd_amd
    assert ecsimd_amd.ETH_REQUIRE_LOW_S == 1 and "ETH_REQUIRE_LOW_S" in ecsimd_amd.__all__
    header = open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read()
    assert re.search(r"enum\s*\{\s*ECSIMD_HIP_ETH_REQUIRE_LOW_S\s*=\s*1\s*\}", header)
    for name in ("keccak256", "eth_address", "eth_recover"):
        assert callable(getattr(ecsimd_amd.Engine, name))


# ---- the shipped listing
@pytest.fixture(scope="module")
def kernels():
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", os.path.join(ROOT, "ecsimd_amd", "csrc"), "ARCH=gfx950"], check=True, capture_output=True)
    ks = {keccak_listing.short(k): v for k, v in keccak_listing.kernels().items()}
    hashes = [k for k in ks if k.startswith("k_keccak256")]
    assert len(hashes) == 6 and "k_eth_address<0>" in ks and "k_eth_address<1>" in ks, sorted(ks)      # 8-, 4-, 1-byte loads x {uniform, per-lane lengths}
    return ks


def test_no_keccak_kernel_uses_scratch(kernels):
    for name, k in kernels.items():
        assert k["scratch"] == 0, (name, k)


def test_the_only_branches_are_the_bounds_exit_and_the_block_loop(kernels):
    """The loop `for (b = 0; b < full; ++b)` is two conditional branches in the listing: the compiler rotates it, so a "no whole block" test jumps from in
    front of the loop to right behind it (tools/keccak_listing.py calls it the guard) and the closing branch jumps back.  Nothing else may branch: the
    last block's loads are steered by address arithmetic, not by branches."""
    for name, k in kernels.items():
        if name.startswith("k_keccak256"):
            assert sorted(k["branches"]) == ["exit", "guard", "loop"], (name, k["branches"])
        else:
            assert k["branches"] == ["exit"], (name, k["branches"])


def committed(key):
    m = re.search(r"^%s\s*=\s*(\d+)\s*$" % re.escape(key), open(PROFILE).read(), re.M)
    assert m, f"{key} = <number> is missing from profiles/r08/keccak_eth.txt"
    return int(m.group(1))


def test_the_permutation_is_the_size_the_profile_says(kernels):
    """A guard against a silent regression (a lane array sent to scratch, rotations by a variable count), not a performance claim: the VALU instructions
    between the labels of k_keccak256's block loop -- one block absorbed and one Keccak-f[1600] -- within 5 % of the committed figure, and every rotation
    still a pair of funnel shifts: 24 rounds x (5 + 24) rotations x 2."""
    want = committed("loop_valu")
    for name, k in kernels.items():
        if name.startswith("k_keccak256"):
            print(name, k["loop_valu"], k["loop_alignbit"])
            assert abs(k["loop_valu"] - want) <= 0.05 * want, (name, k["loop_valu"], want)
            assert k["loop_alignbit"] == committed("loop_alignbit") == 24 * 29 * 2, (name, k["loop_alignbit"])


def test_the_new_sources_hold_none_of_the_words_this_pool_refuses():
    words = [a + b for a, b in (("s_st", "ore_"), ("s_buffer_st", "ore_"), ("s_scratch_st", "ore_"), ("s_atom", "ic_"), ("s_buffer_atom", "ic_"), ("s_dcache_", "wb"), ("s_dcache_", "discard"))]
    new = ["ecsimd_amd/csrc/k_keccak.hip", "ecsimd_amd/csrc/keccak.cuh", "include/ecsimd/keccak256.h", "tools/keccak_model.py", "tools/keccak_listing.py", "tools/time_keccak_eth.py",
           "tests/test_keccak_cpu.py", "tests/test_gpu_keccak_eth.py", "tests/test_cpp_keccak.py", "tests/cpp/keccak_tests.cpp"]
    for f in new:
        text = open(os.path.join(ROOT, f)).read().lower()
        assert not [w for w in words if w in text], f
    listing = open(keccak_listing.DEFAULT).read().lower() if os.path.exists(keccak_listing.DEFAULT) else ""
    assert not [w for w in words if w in listing]
