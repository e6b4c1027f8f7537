"""GPU suite: every capturable entry point replayed from a hipGraph, every host-bound one refused under capture (tests/capture_matrix.py is the list).

The shape of each replay test: an eager warm-up call at the capture's batch size (it sizes the context workspace and builds the tables), a capture on ONE
side stream -- the graph is a chain --, then two replays, each after the inputs were overwritten IN PLACE with another input set.  After each replay every
output of every lane equals (a) the eager call on the same inputs and (b) a reference that never ran on the device: hashlib / hmac, the models under tools/
(pinned to published vectors by the CPU suite), the C restatement of the reference (the `oracle` fixture) for the calls that mirror a reference function,
plain Python integers for the rest.  Where (b) is big-integer curve arithmetic it is taken on SAMPLE -- lanes of every wave -- plus the graph's special lanes.
The second replay is what fails when a call baked an input into the graph by value or when a replay leaves state behind that the next one picks up.

CAPTURABLE_CASES / REFUSES_CASES name the graph (or the refused call) that covers each ABI name; tests/test_capture_matrix_cpu.py holds them to the matrix.
Importing this file needs no GPU.
"""
import ctypes as C
import functools
import hashlib
import hmac
import json
import os
import random
import re
import sys

import numpy as np
import pytest

from helpers import CURVE_PARAMS, P256, SECP256K1, SEED, arr_to_ints, ec_add, ec_mul, fill_random_np, ints_to_arr, jacobian_mgry_to_affine_int
from test_gpu_btc_tree import CYCLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bip32_model            # noqa: E402
import bip340_model           # noqa: E402
import btc_model              # noqa: E402
import btc_tree_model         # noqa: E402
import ecdsa_recover_model    # noqa: E402
import keccak_model           # noqa: E402
import rfc6979_model          # noqa: E402

pytestmark = pytest.mark.gpu
SLICE = int(re.search(r"ECSIMD_HIP_PBKDF2_SLICE\s*=\s*(\d+)", open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read()).group(1))
OUT_AFFINE, WINDOWED, CONSTANT_TIME = 2, 4, 128
N = 3 * 64 + 5                 # a full wave, more waves and a ragged one
NP = 65                        # the PBKDF2 graphs: a whole wave and a partial one
SAMPLE = sorted({64 * w + o for w in range(3) for o in (0, 1, 17, 31, 46, 62, 63)} | set(range(192, N)))      # 26 lanes, every wave
assert len(SAMPLE) >= 24
K1 = SECP256K1
NK1, PK1 = bip340_model.N, bip340_model.P
MASK256 = (1 << 256) - 1


# ---- host <-> device
def dev(engine, a):
    """A numpy array as the device tensor the engine takes: u64 limbs as int64 bit patterns, bytes and 32-bit lengths as they are."""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(engine.tdev)


def npy(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def limbs(values, words=4):
    return ints_to_arr([int(v) for v in values], words)


def be32(values):
    """Integers as rows of 32 big-endian bytes."""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in values), dtype=np.uint8).reshape(len(values), 32).copy()


def rows_of(strings, width, i):
    """Byte strings as the rows of one (n, width) uint8 array, random bytes behind each string (other ones in every input set i), and their lengths."""
    rng = random.Random((len(strings) * 1000 + width) * 10 + i)
    host = np.frombuffer(rng.randbytes(len(strings) * width), dtype=np.uint8).reshape(len(strings), width).copy()
    for i, s in enumerate(strings):
        host[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return host, np.array([len(s) for s in strings], dtype=np.int32)


def cycle_strings(rng, n, shift):
    return [rng.randbytes(CYCLE[(i + shift) % len(CYCLE)]) for i in range(n)]


def digests(a):
    """(n, 4) limbs -> the 32 big-endian bytes of each."""
    return [v.to_bytes(32, "big") for v in arr_to_ints(a)]


def byte_rows(a):
    return [bytes(r) for r in a]


def rand_scalars(rng, n, below=1 << 256):
    return [rng.randrange(1, below) for _ in range(n)]


def lift(cv, rng):
    """A random point of the curve (both primes are 3 mod 4)."""
    c = CURVE_PARAMS[cv]; p = c["p"]
    while True:
        x = rng.randrange(p)
        rhs = (x * x * x + c["a"] * x + c["b"]) % p
        y = pow(rhs, (p + 1) // 4, p)
        if y * y % p == rhs and y:
            return x, (y if rng.getrandbits(1) else p - y)


def mul_g(cv, k):
    c = CURVE_PARAMS[cv]
    return bip340_model.mul_g(k) if cv == K1 else ec_mul(cv, k % c["n"], (c["gx"], c["gy"]))


# ---- the graphs.  inputs(i): input set i (0: warm-up and capture, 1 and 2: the replays) as numpy arrays by name; run(engine, b): the calls on the device
# buffers b, returning the outputs by name; check(i, h, o): the outputs o (numpy) of input set h against the reference.
class Bignum:
    names = ["add", "sub", "sub_if_above", "cmp_eq", "cmp_lt", "mask_op", "shift_left_one", "mul", "square", "swap_if", "if_else", "mask_bit", "from_bytes_be",
             "to_bytes_be", "wide4_to_lanes", "lanes_to_wide4", "memcpy_d2d", "fill_random"]

    def __init__(self, oracle):
        pass

    def inputs(self, i):
        rng = random.Random(100 + i)
        a = [rng.getrandbits(256) for _ in range(N)]; b = [rng.getrandbits(256) for _ in range(N)]
        a[3], b[3] = MASK256, MASK256; a[64], b[64] = MASK256, 1; b[65] = a[65]; a[130], b[130] = 0, 1; a[N - 1] = 1 << 255
        return dict(a=limbs(a), b=limbs(b), p=limbs([rng.getrandbits(255) for _ in range(N)]), mask=np.array([rng.getrandbits(1) for _ in range(N)], dtype=np.uint8),
                    m2=np.array([rng.getrandbits(1) for _ in range(N)], dtype=np.uint8), raw=np.frombuffer(rng.randbytes(N * 32), dtype=np.uint8).copy(),
                    wides=np.frombuffer(rng.randbytes(49 * 128), dtype=np.uint8).copy())

    def outputs(self, e):
        return dict(out_rand=e.empty(N))

    def run(self, e, b):
        import torch
        o = {}
        o["add"], o["carry"] = e.add(b["a"], b["b"]); o["sub"], o["borrow"] = e.sub(b["a"], b["b"])
        o["sia"] = e.sub_if_above(b["a"], b["p"]); o["eq"] = e.cmp_eq(b["a"], b["b"]); o["lt"] = e.cmp_lt(b["a"], b["b"])
        o["and"] = e.mask_op(1, b["mask"], b["m2"]); o["not"] = e.mask_op(0, b["mask"])
        o["shl"], o["shc"] = e.shift_left_one(b["a"]); o["mul"] = e.mul(b["a"], b["b"]); o["sqr"] = e.square(b["a"])
        o["swa"], o["swb"] = b["a"].clone(), b["b"].clone(); e.swap_if(b["mask"], o["swa"], o["swb"])
        o["ife"] = e.if_else(b["mask"], b["a"], b["b"]); o["bit"] = e.mask_bit(b["a"], 77)
        o["from_be"] = e.from_bytes_be(b["raw"]); o["to_be"] = e.to_bytes_be(b["a"])
        o["lanes"] = e.wide4_to_lanes(b["wides"])
        o["wide"] = torch.zeros(49 * 128, dtype=torch.uint8, device=e.tdev); e.lanes_to_wide4(b["a"][:196], o["wide"])
        o["copy"] = e.empty(N); e._call("memcpy_d2d", C.c_void_p(o["copy"].data_ptr()), C.c_void_p(b["a"].data_ptr()), C.c_size_t(N * 32))
        o["rand"] = e.fill_random(N, SEED, 7, first_index=3, clear_top_bits=1, out=b["out_rand"])
        return o

    def check(self, i, h, o):
        a, b, p = arr_to_ints(h["a"]), arr_to_ints(h["b"]), arr_to_ints(h["p"]); m = h["mask"]
        eq = lambda name, want: np.array_equal(o[name], want) or pytest.fail(f"bignum {name}, input set {i}")
        u8 = lambda vals: np.array([int(bool(v)) for v in vals], dtype=np.uint8)
        eq("add", limbs([(x + y) & MASK256 for x, y in zip(a, b)])); eq("carry", u8([(x + y) >> 256 for x, y in zip(a, b)]))
        eq("sub", limbs([(x - y) & MASK256 for x, y in zip(a, b)])); eq("borrow", u8([x < y for x, y in zip(a, b)])); eq("lt", u8([x < y for x, y in zip(a, b)]))
        eq("sia", limbs([x - q if x >= q else x for x, q in zip(a, p)])); eq("eq", u8([x == y for x, y in zip(a, b)]))
        eq("and", m & h["m2"]); eq("not", 1 - m)
        eq("shl", limbs([(x << 1) & MASK256 for x in a])); eq("shc", u8([x >> 255 for x in a]))
        eq("mul", limbs([x * y for x, y in zip(a, b)], 8)); eq("sqr", limbs([x * x for x in a], 8))
        eq("swa", limbs([y if f else x for x, y, f in zip(a, b, m)])); eq("swb", limbs([x if f else y for x, y, f in zip(a, b, m)]))
        eq("ife", limbs([x if f else y for x, y, f in zip(a, b, m)])); eq("bit", u8([(x >> 77) & 1 for x in a]))
        eq("from_be", limbs([int.from_bytes(bytes(h["raw"][32 * j:32 * j + 32]), "big") for j in range(N)])); eq("to_be", be32(a))
        eq("lanes", h["wides"].view(np.uint64).reshape(49, 4, 4).transpose(0, 2, 1).reshape(196, 4))
        eq("wide", np.ascontiguousarray(h["a"][:196].reshape(49, 4, 4).transpose(0, 2, 1)).view(np.uint8).reshape(-1))
        eq("copy", h["a"]); eq("rand", fill_random_np(N, SEED, 7, 3, 1))


class Field:
    names = ["mod_add", "mod_sub", "mod_shift_left", "mod_mul", "mgry_reduce", "mgry_mul", "mgry_sqr", "mgry_from_classical", "mgry_to_classical", "mgry_pow",
             "gfp_inverse", "gfp_opposite", "gfp_sqrt"]
    EXP = limbs([0x1234567890abcdef0fedcba987654321f00dfacecafebeef0123456789abcdef])[0]

    def __init__(self, oracle):
        self.oracle = oracle

    def inputs(self, i):
        rng = random.Random(200 + i)
        a = [rng.getrandbits(255) for _ in range(N)]; b = [rng.getrandbits(255) for _ in range(N)]      # below both primes
        a[0] = 0; a[64] = 1; b[N - 1] = 0
        return dict(a=limbs(a), b=limbs(b), a8=limbs([x * y for x, y in zip(a, b)], 8))

    def run(self, e, b):
        o = {}
        for cv in (P256, K1):
            t = lambda name: f"{name}{cv}"
            for name in ("mod_add", "mod_sub", "mod_mul", "mgry_mul"):
                o[t(name)] = getattr(e, name)(cv, b["a"], b["b"])
            for name in ("mgry_sqr", "mgry_from_classical", "mgry_to_classical", "gfp_inverse", "gfp_opposite"):
                o[t(name)] = getattr(e, name)(cv, b["a"])
            o[t("mod_shift_left")] = e.mod_shift_left(cv, b["a"], 5); o[t("mgry_reduce")] = e.mgry_reduce(cv, b["a8"])
            o[t("mgry_pow")] = e.mgry_pow(cv, b["a"], self.EXP); o[t("gfp_sqrt")], o[t("sqrt_ok")] = e.gfp_sqrt(cv, b["a"])
        return o

    def check(self, i, h, o):
        ora = self.oracle
        for cv in (P256, K1):
            p = CURVE_PARAMS[cv]["p"]
            want = {name: getattr(ora, name)(cv, h["a"], h["b"]) for name in ("mod_add", "mod_sub", "mgry_mul")}
            want.update({name: getattr(ora, name)(cv, h["a"]) for name in ("mgry_sqr", "mgry_from_classical", "mgry_to_classical", "gfp_inverse", "gfp_opposite")})
            want["mod_mul"] = limbs([x * y % p for x, y in zip(arr_to_ints(h["a"]), arr_to_ints(h["b"]))])
            want["mod_shift_left"] = ora.mod_shift_left(cv, h["a"], 5); want["mgry_reduce"] = ora.mgry_reduce(cv, h["a8"]); want["mgry_pow"] = ora.mgry_pow(cv, h["a"], self.EXP)
            for name, w in want.items():
                assert np.array_equal(o[f"{name}{cv}"], w), (name, cv, i)
            root, ok = ora.gfp_sqrt(cv, h["a"])
            assert np.array_equal(o[f"sqrt_ok{cv}"], ok) and 0 < ok.sum() < N and np.array_equal(o[f"gfp_sqrt{cv}"][ok == 1], root[ok == 1]), (cv, i)


class Points:
    names = ["from_affine", "to_affine", "compute_y", "on_curve", "dblu", "zaddu", "zdau", "zdau_repeat", "trplu", "add_z2_1", "add_mixed_complete", "affine_add",
             "sec1_encode", "sec1_decode"]

    def __init__(self, oracle):
        self.oracle = oracle

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def points(i):
        out = {}
        for cv in (P256, K1):
            rng = random.Random(300 + 10 * i + cv); p = CURVE_PARAMS[cv]["p"]
            A = [lift(cv, rng) for _ in range(N)]; B = [lift(cv, rng) for _ in range(N)]
            B[1] = A[1]; B[65] = (A[65][0], p - A[65][1]); B[130] = (0, 0); A[131] = (0, 0)           # affine_add: the tangent, the opposite, infinity on either side
            out[cv] = A, B
        return out

    def inputs(self, i):
        h = {}
        for cv, (A, B) in self.points(i).items():
            rng = random.Random(350 + 10 * i + cv); p = CURVE_PARAMS[cv]["p"]
            J = [lift(cv, rng) for _ in range(N)]                                                   # the Jacobian formulas' points: all finite
            h[f"x{cv}"], h[f"y{cv}"] = limbs([q[0] for q in J]), limbs([q[1] for q in J])
            for name, pts in (("a", A), ("b", B)):
                h[f"{name}x{cv}"], h[f"{name}y{cv}"] = limbs([q[0] for q in pts]), limbs([q[1] for q in pts])
            bad = [q[1] for q in J]; bad[2] = (bad[2] + 1) % p; bad[66] = p; bad[N - 1] ^= 2
            h[f"ybad{cv}"] = limbs(bad)
            h[f"xc{cv}"] = limbs([q[0] if j % 3 else rng.randrange(p) for j, q in enumerate(J)])     # compute_y: a third of the lanes may have no root
            rec65 = [b"\x04" + q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big") for q in J]
            rec33 = [bytes([2 | (q[1] & 1)]) + q[0].to_bytes(32, "big") for q in J]
            rec65[4] = b"\x05" + rec65[4][1:]; rec65[67] = rec65[67][:64] + bytes([rec65[67][64] ^ 1]); rec33[5] = b"\x04" + rec33[5][1:]; rec33[68] = b"\x02" + b"\xff" * 32
            h[f"rec65{cv}"] = np.frombuffer(b"".join(rec65), dtype=np.uint8).reshape(N, 65).copy(); h[f"rec33{cv}"] = np.frombuffer(b"".join(rec33), dtype=np.uint8).reshape(N, 33).copy()
        return h

    def run(self, e, b):
        o = {}
        for cv in (P256, K1):
            clone = lambda pt: [t.clone() for t in pt]
            put = lambda name, pt: o.update({f"{name}{c}{cv}": t for c, t in zip("xyz", pt)})
            J = e.from_affine(cv, b[f"x{cv}"], b[f"y{cv}"]); put("j", J)
            P = clone(J); R = e.dblu(cv, P); put("dblu_r", R); put("dblu_p", P)                                # R = 2P, P rewritten: co-Z
            P2 = clone(P); S = e.zaddu(cv, P2, R); put("zaddu_r", S); put("zaddu_p", P2)                          # S = P + 2P, P2 rewritten: co-Z
            Q = clone(S); T = e.zdau(cv, P2, Q); put("zdau_r", T); put("zdau_q", Q)                              # T = 2P + 3P
            P3 = clone(J); U = e.trplu(cv, P3); put("trplu_r", U); put("trplu_p", P3)
            for name, t in zip(("rx", "ry", "sx", "sy", "z"), e.zdau_repeat(cv, U, (P3[0], P3[1]), 3, 0b010, 29)):
                o[f"rep_{name}{cv}"] = t
            Bm = e.from_affine(cv, b[f"bx{cv}"], b[f"by{cv}"])                                                  # B's Montgomery-form affine coordinates
            put("z21_", e.add_z2_1(cv, T, (Bm[0], Bm[1]))); put("amc_", e.add_mixed_complete(cv, T, (Bm[0], Bm[1])))
            o[f"ax{cv}"], o[f"ay{cv}"] = e.to_affine(cv, T)
            o[f"cy{cv}"], o[f"cyok{cv}"] = e.compute_y(cv, b[f"xc{cv}"]); o[f"on{cv}"] = e.on_curve(cv, b[f"x{cv}"], b[f"ybad{cv}"])
            o[f"sumx{cv}"], o[f"sumy{cv}"], o[f"fin{cv}"] = e.affine_add(cv, (b[f"ax{cv}"], b[f"ay{cv}"]), (b[f"bx{cv}"], b[f"by{cv}"]))
            o[f"enc65{cv}"] = e.sec1_encode(cv, b[f"x{cv}"], b[f"y{cv}"]); o[f"enc33{cv}"] = e.sec1_encode(cv, b[f"x{cv}"], b[f"y{cv}"], compressed=True)
            o[f"d65x{cv}"], o[f"d65y{cv}"], o[f"d65ok{cv}"] = e.sec1_decode(cv, b[f"rec65{cv}"]); o[f"d33x{cv}"], o[f"d33y{cv}"], o[f"d33ok{cv}"] = e.sec1_decode(cv, b[f"rec33{cv}"], compressed=True)
        return o

    def check(self, i, h, o):
        ora = self.oracle
        for cv, (A, B) in self.points(i).items():
            c = CURVE_PARAMS[cv]; p = c["p"]
            got = lambda name: tuple(o[f"{name}{k}{cv}"] for k in "xyz")
            same = lambda name, want: all(np.array_equal(g, w) for g, w in zip(got(name), want)) or pytest.fail(f"points {name}, curve {cv}, input set {i}")
            x, y = h[f"x{cv}"], h[f"y{cv}"]; xi, yi = arr_to_ints(x), arr_to_ints(y)
            J = ora.from_affine(cv, x, y); same("j", J)
            R, P = ora.dblu(cv, J); same("dblu_r", R); same("dblu_p", P)
            S, P2 = ora.zaddu(cv, P, R); same("zaddu_r", S); same("zaddu_p", P2)
            T, Q = ora.zdau(cv, P2, S); same("zdau_r", T); same("zdau_q", Q)
            U, P3 = ora.trplu(cv, J); same("trplu_r", U); same("trplu_p", P3)
            Pr, Qr = U, P3
            for t in range(3):                                                                       # tests/test_gpu_parity.py test_reduced_radix_zdau_vs_oracle
                Rn, Qn = ora.zdau(cv, Pr, Qr)
                Pr, Qr = (Qn, Rn) if (0b010 >> t) & 1 else (Rn, Qn)
            for name, want in zip(("rx", "ry", "sx", "sy", "z"), (Pr[0], Pr[1], Qr[0], Qr[1], Pr[2])):
                assert np.array_equal(o[f"rep_{name}{cv}"], want), (name, cv, i)
            Bm = ora.from_affine(cv, h[f"bx{cv}"], h[f"by{cv}"])
            same("z21_", ora.add_z2_1(cv, T, (Bm[0], Bm[1])))
            ax, ay = ora.to_affine(cv, T)
            assert np.array_equal(o[f"ax{cv}"], ax) and np.array_equal(o[f"ay{cv}"], ay), (cv, i)
            amc = [arr_to_ints(t) for t in got("amc_")]
            for j in SAMPLE + [1, 65, 130]:                                                          # the complete addition: T + B on integers (B[130] is infinity)
                five = ec_mul(cv, 5, (xi[j], yi[j])); assert five == (int(arr_to_ints(ax[j:j + 1])[0]), int(arr_to_ints(ay[j:j + 1])[0]))
                assert jacobian_mgry_to_affine_int(cv, amc[0][j], amc[1][j], amc[2][j]) == ec_add(cv, five, None if B[j] == (0, 0) else B[j]), (cv, i, j)
            cy, cyok = ora.compute_y(cv, h[f"xc{cv}"])
            assert np.array_equal(o[f"cyok{cv}"], cyok) and 0 < cyok.sum() < N and np.array_equal(o[f"cy{cv}"][cyok == 1], cy[cyok == 1]), (cv, i)
            on = [int(v < p and (v * v - u * u * u - c["a"] * u - c["b"]) % p == 0) for u, v in zip(xi, arr_to_ints(h[f"ybad{cv}"]))]
            assert o[f"on{cv}"].tolist() == on and sum(on) == N - 3, (cv, i)
            sums = [ec_add(cv, None if a == (0, 0) else a, None if b == (0, 0) else b) for a, b in zip(A, B)]
            assert o[f"fin{cv}"].tolist() == [int(s is not None) for s in sums] and sums[65] is None, (cv, i)
            assert np.array_equal(o[f"sumx{cv}"], limbs([s[0] if s else 0 for s in sums])) and np.array_equal(o[f"sumy{cv}"], limbs([s[1] if s else 0 for s in sums])), (cv, i)
            assert byte_rows(o[f"enc65{cv}"]) == [b"\x04" + u.to_bytes(32, "big") + v.to_bytes(32, "big") for u, v in zip(xi, yi)], (cv, i)
            assert byte_rows(o[f"enc33{cv}"]) == [bytes([2 | (v & 1)]) + u.to_bytes(32, "big") for u, v in zip(xi, yi)], (cv, i)
            for form, refused in (("d65", (4, 67)), ("d33", (5, 68))):
                ok = o[f"{form}ok{cv}"]
                assert ok.tolist() == [int(j not in refused) for j in range(N)], (form, cv, i)
                assert np.array_equal(o[f"{form}x{cv}"][ok == 1], x[ok == 1]) and np.array_equal(o[f"{form}y{cv}"][ok == 1], y[ok == 1]), (form, cv, i)


class ScalarMults:
    names = ["scalar_mult", "scalar_mult_1s", "scalar_mult_base", "scalar_mult_p256", "double_scalar_mult", "ecdsa_verify_rx"]
    ONE = 0x8f3a1c5d7e9b2a4c6e8f0a1b3c5d7e9f1a2b3c4d5e6f708192a3b4c5d6e7f809
    REFUSED = (7, 70, N - 2)       # invalid public keys
    OUT = ("jx", "jy", "jz", "mx", "my", "mz", "bx", "by", "cx", "cy")

    def __init__(self, oracle):
        self.oracle = oracle

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def host(i):
        rng = random.Random(400 + i)
        pts = {cv: [lift(cv, rng) for _ in range(N)] for cv in (P256, K1)}
        k, u1, u2 = ([rng.getrandbits(256) for _ in range(N)] for _ in range(3))
        u1[0] = 0; u2[1] = 0; u1[64] = NK1 - 1
        qy = [q[1] for q in pts[K1]]; qy[7] = (qy[7] + 1) % PK1; qy[70] = PK1; qy[N - 2] ^= 4
        sums = {}
        for j in SAMPLE + list(ScalarMults.REFUSED):                                            # u1 G + u2 Q on integers, for the sampled lanes
            sums[j] = None if j in ScalarMults.REFUSED else bip340_model.add(bip340_model.mul_g(u1[j]), bip340_model.mul(u2[j], pts[K1][j]))
        r = [rng.getrandbits(256) for _ in range(N)]
        for n_, j in enumerate(SAMPLE):
            if sums[j] is not None and n_ % 3:
                r[j] = sums[j][0] % NK1                                                      # two sampled lanes in three verify
        return pts, k, u1, u2, qy, sums, r

    def inputs(self, i):
        pts, k, u1, u2, qy, sums, r = self.host(i)
        return dict(k=limbs(k), u1=limbs(u1), u2=limbs(u2), r=limbs(r), qy=limbs(qy), px=limbs([q[0] for q in pts[P256]]), py=limbs([q[1] for q in pts[P256]]),
                    kx=limbs([q[0] for q in pts[K1]]), ky=limbs([q[1] for q in pts[K1]]))

    def outputs(self, e):
        return {name: e.empty(N) for name in self.OUT}

    def run(self, e, b):
        o = {name: b[name] for name in self.OUT}                                          # written through out=: allocated before the capture
        e.scalar_mult(P256, b["k"], b["px"], b["py"], out=[b["jx"], b["jy"], b["jz"]])                               # the ladder, Jacobian
        M = e.from_affine(P256, b["px"], b["py"]); e.scalar_mult_p256(b["k"], M[0], M[1], out=[b["mx"], b["my"], b["mz"]])
        o["sx"], o["sy"] = e.scalar_mult_1s(K1, limbs([self.ONE])[0], b["kx"], b["ky"], flags=OUT_AFFINE)
        e.scalar_mult_base(P256, b["k"], flags=OUT_AFFINE, out=[b["bx"], b["by"], None])                             # the small-batch comb
        e.scalar_mult_base(K1, b["k"], flags=OUT_AFFINE | WINDOWED | CONSTANT_TIME, out=[b["cx"], b["cy"], None])
        o["dx"], o["dy"], o["fin"] = e.double_scalar_mult(K1, b["u1"], b["u2"], b["kx"], b["qy"])
        o["vok"] = e.ecdsa_verify_rx(K1, b["u1"], b["u2"], b["kx"], b["qy"], b["r"])
        return o

    def check(self, i, h, o):
        pts, k, u1, u2, qy, sums, r = self.host(i)
        J = self.oracle.scalar_mult(P256, h["k"], h["px"], h["py"], threads=8)
        assert all(np.array_equal(o[a], w) for a, w in zip(("jx", "jy", "jz"), J)) and all(np.array_equal(o[a], w) for a, w in zip(("mx", "my", "mz"), J)), i
        at = lambda name, j: int(arr_to_ints(o[name][j:j + 1])[0])
        for j in SAMPLE:
            assert (at("sx", j), at("sy", j)) == bip340_model.mul(self.ONE, pts[K1][j]), (i, j)
            assert (at("cx", j), at("cy", j)) == bip340_model.mul_g(k[j]), (i, j)
        c = CURVE_PARAMS[P256]                                                               # the small-batch comb returns the ladder's affine bits: every lane against the oracle ...
        gx, gy = limbs([c["gx"]] * N), limbs([c["gy"]] * N)
        ox, oy = self.oracle.to_affine(P256, self.oracle.scalar_mult(P256, h["k"], gx, gy, threads=8))
        assert np.array_equal(o["bx"], ox) and np.array_equal(o["by"], oy), i
        for j in SAMPLE:                                                                     # ... and the sample against the affine textbook model
            assert (at("bx", j), at("by", j)) == mul_g(P256, k[j]), (i, j)
        for j, want in sums.items():
            assert (at("dx", j), at("dy", j), int(o["fin"][j])) == ((*want, 1) if want else (0, 0, 0)), (i, j)
            assert int(o["vok"][j]) == int(want is not None and want[0] % NK1 == r[j]), (i, j)
        assert 8 <= sum(int(o["vok"][j]) for j in SAMPLE) < len(SAMPLE) and not any(o["fin"][list(self.REFUSED)])


class EcdsaChain:
    """sha256 -> ecdsa_sign_deterministic -> ecdsa_recover -> ecdsa_verify on one built-in curve."""
    names = []
    REFUSED = {5: 0, 70: "n", N - 1: "n + 1"}

    def __init__(self, oracle, cv):
        self.cv = cv

    def inputs(self, i):
        rng = random.Random(500 + 10 * i + self.cv); n = CURVE_PARAMS[self.cv]["n"]
        d = rand_scalars(rng, N, n); d[5] = 0; d[70] = n; d[N - 1] = n + 1
        return dict(msgs=np.frombuffer(rng.randbytes(N * 77), dtype=np.uint8).reshape(N, 77).copy(), d=limbs(d))

    def run(self, e, b):
        o = {}
        o["e"] = e.sha256(b["msgs"])
        o["r"], o["s"], o["v"], o["ok"] = e.ecdsa_sign_deterministic(self.cv, o["e"], b["d"], low_s=True)
        o["qx"], o["qy"], o["rok"] = e.ecdsa_recover(self.cv, o["e"], o["r"], o["s"], o["v"])
        o["vok"] = e.ecdsa_verify(self.cv, o["e"], o["r"], o["s"], o["qx"], o["qy"])
        return o

    def check(self, i, h, o):
        c = CURVE_PARAMS[self.cv]; d = arr_to_ints(h["d"])
        assert digests(o["e"]) == [hashlib.sha256(bytes(m)).digest() for m in h["msgs"]], i
        want_ok = [int(1 <= x < c["n"]) for x in d]
        assert o["ok"].tolist() == want_ok and o["rok"].tolist() == want_ok and o["vok"].tolist() == want_ok, i
        r, s, qx, qy = (arr_to_ints(o[name]) for name in ("r", "s", "qx", "qy"))
        for j in SAMPLE + list(self.REFUSED):
            sig = rfc6979_model.sign(c, int.from_bytes(hashlib.sha256(bytes(h["msgs"][j])).digest(), "big"), d[j], low_s=True)
            if j in self.REFUSED:
                assert sig is None and (r[j], s[j], int(o["v"][j]), qx[j], qy[j]) == (0, 0, 0, 0, 0), (i, j)
            else:
                assert (r[j], s[j], int(o["v"][j])) == sig[:3] and (qx[j], qy[j]) == mul_g(self.cv, d[j]), (i, j)


class EcdsaChainP256(EcdsaChain):
    names = ["sha256", "ecdsa_sign_deterministic"]

    def __init__(self, oracle):
        super().__init__(oracle, P256)


class EcdsaChainK1(EcdsaChain):
    names = ["ecdsa_recover", "ecdsa_verify"]

    def __init__(self, oracle):
        super().__init__(oracle, K1)


class EcdsaPlain:
    """The caller's nonces: rfc6979_nonce, ecdsa_sign, ecdsa_sign_recoverable, and ecdsa_verify on host-made signatures with refused lanes among them."""
    names = ["rfc6979_nonce", "ecdsa_sign", "ecdsa_sign_recoverable"]
    BAD_D, BAD_K = (6, 129), (66, N - 3)
    TAMPERED = {8: "s = n", 71: "r = 0", 133: "key off the curve", N - 1: "another digest"}

    def __init__(self, oracle):
        pass

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def host(i):
        rng = random.Random(600 + i); c = CURVE_PARAMS[K1]
        e, d, k = ([rng.getrandbits(256) for _ in range(N)], rand_scalars(rng, N, NK1), rand_scalars(rng, N, NK1))
        sigs = [ecdsa_recover_model.sign_recoverable(c, e[j], d[j], k[j], kG=bip340_model.mul_g(k[j])) for j in range(N)]
        keys = [bip340_model.mul_g(x) for x in d]
        return e, d, k, sigs, keys

    def inputs(self, i):
        e, d, k, sigs, keys = self.host(i)
        d, k = list(d), list(k); d[6] = 0; d[129] = NK1; k[66] = 0; k[N - 3] = NK1
        r, s, qy, e2 = [g[0] for g in sigs], [g[1] for g in sigs], [q[1] for q in keys], list(e)
        s[8] = NK1; r[71] = 0; qy[133] = (qy[133] + 1) % PK1; e2[N - 1] ^= 1
        return dict(e=limbs(e), d=limbs(d), k=limbs(k), vr=limbs(r), vs=limbs(s), ve=limbs(e2), qx=limbs([q[0] for q in keys]), qy=limbs(qy))

    def run(self, e, b):
        o = {}
        o["k"], o["kok"] = e.rfc6979_nonce(K1, b["e"], b["d"])
        o["r"], o["s"], o["ok"] = e.ecdsa_sign(K1, b["e"], b["d"], b["k"])
        o["r2"], o["s2"], o["v2"], o["ok2"] = e.ecdsa_sign_recoverable(K1, b["e"], b["d"], b["k"])
        o["vok"] = e.ecdsa_verify(K1, b["ve"], b["vr"], b["vs"], b["qx"], b["qy"])
        return o

    def check(self, i, h, o):
        e, d, k, sigs, keys = self.host(i)
        refused = set(self.BAD_D + self.BAD_K)
        want = [(0, 0, 0, 0) if j in refused else (*sigs[j], 1) for j in range(N)]
        assert list(zip(arr_to_ints(o["r"]), arr_to_ints(o["s"]), o["ok"].tolist())) == [(w[0], w[1], w[3]) for w in want], i
        assert list(zip(arr_to_ints(o["r2"]), arr_to_ints(o["s2"]), o["v2"].tolist(), o["ok2"].tolist())) == want, i
        nonces = [None if j in self.BAD_D else rfc6979_model.nonce(NK1, e[j], d[j]) for j in range(N)]
        assert list(zip(arr_to_ints(o["k"]), o["kok"].tolist())) == [(q[0], 1) if q else (0, 0) for q in nonces], i
        assert o["vok"].tolist() == [int(j not in self.TAMPERED) for j in range(N)], i


class SchnorrChain:
    """taproot_tweak_seckey -> schnorr_sign -> schnorr_verify, and schnorr_verify on host-made signatures with refused lanes among them."""
    names = ["taproot_tweak_seckey", "schnorr_sign", "schnorr_verify"]
    REFUSED = (9, 72)              # d = 0, d = n
    MSG = 45

    def __init__(self, oracle):
        pass

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def host(i):
        rng = random.Random(700 + i)
        d = rand_scalars(rng, N, NK1); d[9] = 0; d[72] = NK1
        root, aux = [rng.getrandbits(256) for _ in range(N)], [rng.getrandbits(256) for _ in range(N)]
        msgs = [rng.randbytes(SchnorrChain.MSG) for _ in range(N)]
        vpx, vr, vs = ([rng.getrandbits(255) for _ in range(N)] for _ in range(3))
        for j in SAMPLE:                                                                        # genuine signatures of the same messages under other keys
            vpx[j], vr[j], vs[j] = bip340_model.sign(rng.randrange(1, NK1), msgs[j], rng.getrandbits(256))
        vr[SAMPLE[1]] = PK1; vs[SAMPLE[8]] = NK1; vs[SAMPLE[15]] ^= 1; vpx[SAMPLE[22]] = PK1 + 1     # r >= p, s = n, a wrong s, px >= p
        return d, root, aux, msgs, vpx, vr, vs

    def inputs(self, i):
        d, root, aux, msgs, vpx, vr, vs = self.host(i)
        return dict(d=limbs(d), root=limbs(root), aux=limbs(aux), msgs=np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(N, self.MSG).copy(), vpx=limbs(vpx), vr=limbs(vr), vs=limbs(vs))

    def run(self, e, b):
        o = {}
        o["dq"], o["px0"], o["tok"] = e.taproot_tweak_seckey(b["d"], b["root"])
        o["px"], o["r"], o["s"], o["sok"] = e.schnorr_sign(o["dq"], b["msgs"], b["aux"])
        o["vok"] = e.schnorr_verify(o["px"], b["msgs"], o["r"], o["s"])
        o["vok2"] = e.schnorr_verify(b["vpx"], b["msgs"], b["vr"], b["vs"])
        return o

    def check(self, i, h, o):
        d, root, aux, msgs, vpx, vr, vs = self.host(i)
        want_ok = [int(j not in self.REFUSED) for j in range(N)]
        assert o["tok"].tolist() == want_ok and o["sok"].tolist() == want_ok and o["vok"].tolist() == want_ok, i
        dq, px0, px, r, s = (arr_to_ints(o[name]) for name in ("dq", "px0", "px", "r", "s"))
        for j in SAMPLE + list(self.REFUSED):
            tw = btc_model.taproot_tweak_seckey(d[j], root[j])
            assert (dq[j], px0[j]) == (tw if tw else (0, 0)), (i, j)
            sig = bip340_model.sign(tw[0], msgs[j], aux[j]) if tw else None
            assert (px[j], r[j], s[j]) == (sig if sig else (0, 0, 0)), (i, j)
            assert int(o["vok2"][j]) == int(bip340_model.verify(vpx[j], msgs[j], vr[j], vs[j])), (i, j)
        assert [int(o["vok2"][j]) for j in (SAMPLE[1], SAMPLE[8], SAMPLE[15], SAMPLE[22])] == [0, 0, 0, 0] and sum(int(o["vok2"][j]) for j in SAMPLE) == len(SAMPLE) - 4, i


class TaprootPath:
    """tapleaf_hash -> taproot_merkle_path -> taproot_tweak_pubkey, with the key-path form and xonly_tweak_add beside them."""
    names = ["tapleaf_hash", "taproot_merkle_path", "taproot_tweak_pubkey", "xonly_tweak_add"]
    NODES = 3

    def __init__(self, oracle):
        pass

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def host(i):
        rng = random.Random(800 + i)
        scripts = cycle_strings(rng, N, i)
        versions = [2 * rng.randrange(128) for _ in range(N)]
        depths = [(j + i) % (TaprootPath.NODES + 1) for j in range(N)]; depths[73] = 129; depths[N - 1] = 255       # beyond BIP-341's bound: refused, no node read
        paths = [[rng.randbytes(32) for _ in range(TaprootPath.NODES)] for _ in range(N)]
        px = [lift(K1, rng)[0] for _ in range(N)]; px[10] = PK1; px[74] = 5                                      # x >= p; x = 5 has no point on secp256k1
        assert bip340_model.lift_x(5) is None
        t = [rng.randrange(NK1) for _ in range(N)]; t[0] = 0; t[75] = NK1
        return scripts, versions, depths, paths, px, t

    def inputs(self, i):
        scripts, versions, depths, paths, px, t = self.host(i)
        rows, lens = rows_of(scripts, 200, i)
        return dict(scripts=rows, lens=lens, versions=np.array(versions, dtype=np.uint8), depths=np.array(depths, dtype=np.uint8),
                    paths=np.frombuffer(b"".join(b"".join(p) for p in paths), dtype=np.uint8).reshape(N, 32 * self.NODES).copy(), px=limbs(px), t=limbs(t))

    def run(self, e, b):
        o = {}
        o["leaf"] = e.tapleaf_hash(b["scripts"], b["lens"], b["versions"])
        o["root"], o["pok"] = e.taproot_merkle_path(o["leaf"], b["paths"], b["depths"])
        o["qx"], o["par"], o["ok"] = e.taproot_tweak_pubkey(b["px"], o["root"])
        o["kx"], o["kpar"], o["kok"] = e.taproot_tweak_pubkey(b["px"])
        o["ax"], o["apar"], o["aok"] = e.xonly_tweak_add(b["px"], b["t"])
        return o

    def check(self, i, h, o):
        scripts, versions, depths, paths, px, t = self.host(i)
        leaves = [btc_tree_model.tapleaf_hash(s, v) for s, v in zip(scripts, versions)]
        roots = [btc_tree_model.merkle_path_root(k, p[:dd]) if dd <= 128 else None for k, p, dd in zip(leaves, paths, depths)]
        assert digests(o["leaf"]) == leaves, i
        assert digests(o["root"]) == [q if q else bytes(32) for q in roots] and o["pok"].tolist() == [int(q is not None) for q in roots], i
        triple = lambda q: (*q, 1) if q else (0, 0, 0)
        lanes = SAMPLE + [10, 73, 74, 75]
        got = lambda x, par, ok: [(int(arr_to_ints(o[x][j:j + 1])[0]), int(o[par][j]), int(o[ok][j])) for j in lanes]
        assert got("qx", "par", "ok") == [triple(btc_model.taproot_tweak_pubkey(px[j], int.from_bytes(roots[j] if roots[j] else bytes(32), "big"))) for j in lanes], i
        assert got("kx", "kpar", "kok") == [triple(btc_model.taproot_tweak_pubkey(px[j])) for j in lanes], i
        assert got("ax", "apar", "aok") == [triple(btc_model.xonly_tweak_add(px[j], t[j])) for j in lanes], i
        assert o["ok"][10] == 0 and o["ok"][74] == 0 and o["aok"][75] == 0 and o["aok"][0] == 1


class Eth:
    """keccak256 -> eth_recover, with and without the recovered key."""
    names = ["keccak256", "eth_recover"]
    REFUSED = {11: "v = 2", 76: "s = n", 140: "v = 29", N - 1: "r = 0"}

    def __init__(self, oracle):
        pass

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def host(i):
        rng = random.Random(900 + i); c = CURVE_PARAMS[K1]
        msgs = cycle_strings(rng, N, 2 * i)
        sigs = [(rng.randrange(1, NK1), rng.randrange(1, NK1), rng.getrandbits(1)) for _ in range(N)]        # most lanes: numbers, recovered to some key or refused
        addr = {}
        for j in SAMPLE + list(Eth.REFUSED):                                                                # these: genuine signatures of the digest
            d, k = rng.randrange(1, NK1), rng.randrange(1, NK1)
            sigs[j] = ecdsa_recover_model.sign_recoverable(c, int.from_bytes(keccak_model.keccak256(msgs[j]), "big"), d, k, kG=bip340_model.mul_g(k))
            addr[j] = keccak_model.eth_address(*bip340_model.mul_g(d))
        return msgs, sigs, addr

    def inputs(self, i):
        msgs, sigs, addr = self.host(i)
        r, s = [g[0] for g in sigs], [g[1] for g in sigs]
        v = [g[2] + (27 if j % 2 else 0) for j, g in enumerate(sigs)]                                         # both forms of the recovery id
        for j, g in enumerate(sigs):
            if g[2] > 1: v[j] = g[2]                                                                         # (x(R) >= n: 2^-128; Ethereum refuses it)
        v[11] = 2; s[76] = NK1; v[140] = 29; r[N - 1] = 0
        rows, lens = rows_of(msgs, 200, i)
        return dict(msgs=rows, lens=lens, r=limbs(r), s=limbs(s), v=np.array(v, dtype=np.uint8))

    def run(self, e, b):
        o = {}
        o["e"] = e.keccak256(b["msgs"], b["lens"])
        o["addr"], o["qx"], o["qy"], o["ok"] = e.eth_recover(o["e"], b["r"], b["s"], b["v"], want_key=True)
        o["addr2"], o["ok2"] = e.eth_recover(o["e"], b["r"], b["s"], b["v"])
        return o

    def check(self, i, h, o):
        msgs, sigs, addr = self.host(i)
        assert digests(o["e"]) == [keccak_model.keccak256(m) for m in msgs], i
        assert np.array_equal(o["ok"], o["ok2"]) and np.array_equal(o["addr"], o["addr2"]), i
        qx, qy = arr_to_ints(o["qx"]), arr_to_ints(o["qy"])
        for j in addr:
            if j in self.REFUSED:
                assert (int(o["ok"][j]), bytes(o["addr"][j]), qx[j], qy[j]) == (0, bytes(20), 0, 0), (i, j)
            else:
                assert (int(o["ok"][j]), bytes(o["addr"][j])) == (1, addr[j]) and keccak_model.eth_address(qx[j], qy[j]) == addr[j], (i, j)


class Bip32Chain:
    """bip32_master -> bip32_ckd_priv (hardened, then not) -> scalar_mult_base (constant-time comb) -> eth_address and btc_pubkey_hash; bip32_ckd_pub beside them."""
    names = ["bip32_master", "bip32_ckd_priv", "bip32_ckd_pub", "eth_address", "btc_pubkey_hash"]
    H = 1 << 31

    def __init__(self, oracle):
        pass

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def host(i):
        rng = random.Random(1000 + i)
        seeds = [rng.randbytes(64) for _ in range(N)]
        hard = [Bip32Chain.H + rng.randrange(Bip32Chain.H) for _ in range(N)]; soft = [rng.randrange(Bip32Chain.H) for _ in range(N)]
        keys = [lift(K1, rng) for _ in range(N)]
        chain = [rng.getrandbits(256) for _ in range(N)]
        index = [rng.randrange(Bip32Chain.H) for _ in range(N)]; index[12] = Bip32Chain.H + 1                 # a hardened index to CKDpub: refused
        keys[77] = (keys[77][0], keys[77][1] ^ 1)                                                            # a key off the curve: refused
        return seeds, hard, soft, keys, chain, index

    def inputs(self, i):
        seeds, hard, soft, keys, chain, index = self.host(i)
        u32 = lambda v: np.array(v, dtype=np.uint32).view(np.int32)
        return dict(seeds=np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(N, 64).copy(), hard=u32(hard), soft=u32(soft), qx=limbs([q[0] for q in keys]), qy=limbs([q[1] for q in keys]),
                    chain=limbs(chain), index=u32(index))

    def run(self, e, b):
        o = {}
        o["k"], o["c"], o["ok"] = e.bip32_master(b["seeds"])
        o["k1"], o["c1"], o["ok1"] = e.bip32_ckd_priv(o["k"], o["c"], b["hard"])
        o["k2"], o["c2"], o["ok2"] = e.bip32_ckd_priv(o["k1"], o["c1"], b["soft"])
        o["x"], o["y"] = e.scalar_mult_base(K1, o["k2"], flags=OUT_AFFINE | WINDOWED | CONSTANT_TIME)
        o["addr"] = e.eth_address(o["x"], o["y"]); o["h160"] = e.btc_pubkey_hash(o["x"], o["y"]); o["h160u"] = e.btc_pubkey_hash(o["x"], o["y"], compressed=False)
        o["cx"], o["cy"], o["cc"], o["pok"] = e.bip32_ckd_pub(b["qx"], b["qy"], b["chain"], b["index"])
        return o

    def check(self, i, h, o):
        seeds, hard, soft, keys, chain, index = self.host(i)
        I = [hmac.new(b"Bitcoin seed", s, hashlib.sha512).digest() for s in seeds]                           # every lane's master node from hashlib
        assert digests(o["k"]) == [x[:32] for x in I] and digests(o["c"]) == [x[32:] for x in I] and o["ok"].all(), i
        assert o["ok1"].all() and o["ok2"].all() and o["pok"].tolist() == [int(j not in (12, 77)) for j in range(N)], i
        ints = {name: arr_to_ints(o[name]) for name in ("k1", "c1", "k2", "c2", "x", "y", "cx", "cy", "cc")}
        for j in SAMPLE + [12, 77]:
            k, c = bip32_model.master(seeds[j])
            n1 = bip32_model.ckd_priv(k, c, hard[j]); n2 = bip32_model.ckd_priv(*n1, soft[j])
            assert (ints["k1"][j], ints["c1"][j]) == n1 and (ints["k2"][j], ints["c2"][j]) == n2, (i, j)
            x, y = bip340_model.mul_g(n2[0])
            assert (ints["x"][j], ints["y"][j]) == (x, y) and bytes(o["addr"][j]) == keccak_model.eth_address(x, y), (i, j)
            assert bytes(o["h160"][j]) == btc_model.btc_pubkey_hash(x, y) and bytes(o["h160u"][j]) == btc_model.btc_pubkey_hash(x, y, compressed=False), (i, j)
            pub = bip32_model.ckd_pub(keys[j], chain[j], index[j])
            assert (ints["cx"][j], ints["cy"][j], ints["cc"][j]) == ((*pub[0], pub[1]) if pub else (0, 0, 0)) and (pub is None) == (j in (12, 77)), (i, j)


class Hashes:
    names = ["sha512", "hmac_sha512", "ripemd160", "hash160", "sha256d", "sha256_lens", "sha256d_lens", "hash160_lens", "ripemd160_lens"]
    FIXED = 119

    def __init__(self, oracle):
        pass

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def host(i):
        rng = random.Random(1100 + i)
        return cycle_strings(rng, N, 3 * i + 1), [rng.randbytes(40) for _ in range(N)]

    def inputs(self, i):
        msgs, keys = self.host(i)
        rows, lens = rows_of(msgs, 200, i)
        return dict(msgs=rows, lens=lens, keys=np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(N, 40).copy())

    def run(self, e, b):
        o = {}
        fixed = b["msgs"][:, :self.FIXED]                                  # rows 200 bytes apart
        o["sha512"] = e.sha512(fixed); o["hmac"] = e.hmac_sha512(b["keys"], fixed)
        for name in ("ripemd160", "hash160", "sha256d"):
            o[name] = getattr(e, name)(fixed); o[name + "_lens"] = getattr(e, name)(b["msgs"], b["lens"])
        o["sha256_lens"] = e.sha256(b["msgs"], b["lens"])
        return o

    def check(self, i, h, o):
        msgs, keys = self.host(i)
        fixed = [bytes(r[:self.FIXED]) for r in h["msgs"]]
        assert byte_rows(o["sha512"]) == [hashlib.sha512(m).digest() for m in fixed] and byte_rows(o["hmac"]) == [hmac.new(k, m, hashlib.sha512).digest() for k, m in zip(keys, fixed)], i
        ref = {"ripemd160": btc_model.ripemd160, "hash160": btc_model.hash160, "sha256d": btc_model.sha256d, "sha256": lambda m: hashlib.sha256(m).digest()}
        out = lambda name: digests(o[name]) if name.startswith("sha256") else byte_rows(o[name])
        for name in ("ripemd160", "hash160", "sha256d"):
            assert out(name) == [ref[name](m) for m in fixed], (name, i)
        for name in ("ripemd160", "hash160", "sha256d", "sha256"):
            assert out(name + "_lens") == [ref[name](m) for m in msgs], (name, i)


class Bip39:
    names = ["bip39_seed"]

    def __init__(self, oracle):
        pass

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def host(i):
        rng = random.Random(1200 + i)
        return cycle_strings(rng, NP, i), [rng.randbytes((5 * j + i) % 21) for j in range(NP)]

    def inputs(self, i):
        sentences, phrases = self.host(i)
        m, ml = rows_of(sentences, 200, i); p, pl = rows_of(phrases, 20, i)
        return dict(m=m, ml=ml, p=p, pl=pl)

    def run(self, e, b):
        return {"seed": e.bip39_seed(b["m"], b["p"], b["ml"], b["pl"])}

    def check(self, i, h, o):
        sentences, phrases = self.host(i)
        assert byte_rows(o["seed"]) == [hashlib.pbkdf2_hmac("sha512", m, b"mnemonic" + p, 2048, 64) for m, p in zip(sentences, phrases)], i


class Pbkdf2Sliced:
    """SLICE + 1 iterations, 65 bytes: two slices, two output blocks, the states parked in the workspace between the launches, the wipe."""
    names = ["pbkdf2_hmac_sha512"]
    DK, WIDTH = 65, 80

    def __init__(self, oracle):
        pass

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def host(i):
        rng = random.Random(1300 + i)
        return cycle_strings(rng, NP, i + 4), [rng.randbytes((7 * j + i) % 25) for j in range(NP)]

    def inputs(self, i):
        pws, salts = self.host(i)
        p, pl = rows_of(pws, 200, i); s, sl = rows_of(salts, 24, i)
        return dict(p=p, pl=pl, s=s, sl=sl, out=np.full((NP, self.WIDTH), 0x5a, dtype=np.uint8))

    def run(self, e, b):
        e.pbkdf2_hmac_sha512(b["p"], b["s"], SLICE + 1, self.DK, pw_lens=b["pl"], salt_lens=b["sl"], out=b["out"])
        return {"out": b["out"]}

    def check(self, i, h, o):
        pws, salts = self.host(i)
        assert byte_rows(o["out"][:, :self.DK]) == [hashlib.pbkdf2_hmac("sha512", p, s, SLICE + 1, self.DK) for p, s in zip(pws, salts)], i
        assert (o["out"][:, self.DK:] == 0x5a).all(), "the bytes between the keys stay as they were"


class Streams:
    """Selecting the context's own stream and coming back inside a capture: under capture both calls only store the handle, and the capture stays valid."""
    names = ["set_stream", "use_own_stream"]

    def __init__(self, oracle):
        pass

    def inputs(self, i):
        rng = random.Random(1400 + i)
        return dict(msgs=np.frombuffer(rng.randbytes(N * 64), dtype=np.uint8).reshape(N, 64).copy())

    def run(self, e, b):
        e._check(e.lib.ecsimd_hip_use_own_stream(e.ctx), "use_own_stream")
        return {"e": e.sha256(b["msgs"])}                                  # (the engine selects torch's current stream again: ecsimd_hip_set_stream)

    def check(self, i, h, o):
        assert digests(o["e"]) == [hashlib.sha256(bytes(m)).digest() for m in h["msgs"]], i


class Fe29Raw:
    """The raw reduced-radix product on the proofs' witnesses (tests/golden/fe29_witnesses.json): the exact model's output limbs are the reference."""
    names = ["fe29_raw"]

    def __init__(self, oracle):
        data = json.load(open(os.path.join(ROOT, "tests", "golden", "fe29_witnesses.json")))
        self.entries = [x for x in data["entries"] if (x["curve"], x["op"], x["swap"]) == ("secp256k1", "mul", 0)]
        assert len(self.entries) >= 27

    def inputs(self, i):
        return dict(limbs=np.array([x["in"] for x in self.entries[9 * i:9 * i + 9]], dtype=np.int64).astype(np.int32))

    def run(self, e, b):
        return {"out": e.fe29_raw(K1, 7, b["limbs"])}

    def check(self, i, h, o):
        assert np.array_equal(o["out"], np.array([x["out"] for x in self.entries[9 * i:9 * i + 9]], dtype=np.int64).astype(np.int32)), i


GRAPHS = {"bignum": Bignum, "field": Field, "points": Points, "scalar_mults": ScalarMults, "ecdsa_chain_p256": EcdsaChainP256, "ecdsa_chain_secp256k1": EcdsaChainK1,
          "ecdsa_plain": EcdsaPlain, "schnorr_chain": SchnorrChain, "taproot_path": TaprootPath, "eth": Eth, "bip32_chain": Bip32Chain, "hashes": Hashes, "bip39": Bip39,
          "pbkdf2_sliced": Pbkdf2Sliced, "streams": Streams, "fe29_raw": Fe29Raw}
CAPTURABLE_CASES = {name: graph for graph, cls in GRAPHS.items() for name in cls.names}


@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_replay_equals_eager_and_the_models(engine, oracle, graph):
    import torch
    G = GRAPHS[graph](oracle)
    sets = [G.inputs(i) for i in range(3)]
    bufs = {k: dev(engine, v) for k, v in sets[0].items()}
    if hasattr(G, "outputs"):
        bufs.update(G.outputs(engine))                                  # out= where the engine's method has it: the caller's arrays, not the graph's pool
    G.run(engine, bufs); torch.cuda.synchronize()                       # warm-up at the capture's batch size: workspace, tables
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = G.run(engine, bufs)                                   # (outputs the engine allocates here live in the graph's pool: read while g is alive)
    torch.cuda.synchronize()
    for i in (1, 2):
        for k, v in sets[i].items():
            bufs[k].copy_(dev(engine, v))                               # new inputs, same buffers
        torch.cuda.synchronize()
        g.replay(); torch.cuda.synchronize()
        got = {k: v.clone() for k, v in out.items()}
        eager = G.run(engine, bufs); torch.cuda.synchronize()
        assert sorted(got) == sorted(eager)
        different = [k for k in got if not torch.equal(got[k], eager[k])]
        assert not different, (graph, i, different)                     # (a) every output of every lane equals the eager call's
        G.check(i, sets[i], {k: npy(v) for k, v in got.items()})        # (b) and the reference's
    del g


# ---- the wipe is a node of the graph
def _wipe_calls():
    rng = random.Random(1500)
    e, d, k = limbs([rng.getrandbits(256) for _ in range(N)]), limbs(rand_scalars(rng, N, NK1)), limbs(rand_scalars(rng, N, NK1))
    msgs = np.frombuffer(rng.randbytes(N * 32), dtype=np.uint8).reshape(N, 32).copy()
    pw = np.frombuffer(rng.randbytes(NP * 24), dtype=np.uint8).reshape(NP, 24).copy(); salt = np.frombuffer(rng.randbytes(NP * 12), dtype=np.uint8).reshape(NP, 12).copy()
    return {
        "ecdsa_sign": (dict(e=e, d=d, k=k), lambda g, b: g.ecdsa_sign(K1, b["e"], b["d"], b["k"])),
        "ecdsa_sign_recoverable": (dict(e=e, d=d, k=k), lambda g, b: g.ecdsa_sign_recoverable(P256, b["e"], b["d"], b["k"])),
        "ecdsa_sign_deterministic": (dict(e=e, d=d), lambda g, b: g.ecdsa_sign_deterministic(K1, b["e"], b["d"])),
        "schnorr_sign": (dict(d=d, msgs=msgs, aux=e), lambda g, b: g.schnorr_sign(b["d"], b["msgs"], b["aux"])),
        "taproot_tweak_seckey": (dict(d=d, root=e), lambda g, b: g.taproot_tweak_seckey(b["d"], b["root"])),
        "bip32_ckd_priv": (dict(k=d, c=e), lambda g, b: g.bip32_ckd_priv(b["k"], b["c"], 5)),
        "pbkdf2_hmac_sha512": (dict(pw=pw, salt=salt), lambda g, b: g.pbkdf2_hmac_sha512(b["pw"], b["salt"], SLICE + 1, 65)),
    }


WIPING_CALLS = sorted(_wipe_calls())


@pytest.mark.parametrize("call", WIPING_CALLS)
def test_the_workspace_is_wiped_by_every_replay(call):
    """A context of its own per call.  The workspace block is filled with 0xA5, the call runs eagerly and the zeroed prefix of the block is recorded; the block
    is filled again, the captured graph replayed and the block read back: the same non-empty prefix is zero and every byte behind it is still 0xA5.  The
    layout is measured, not assumed, and the fill proves that the readback sees what a replay leaves behind -- a wipe that only the capturing call performed
    would leave the replay's secrets (non-zero bytes) inside the prefix."""
    import torch
    from ecsimd_amd import Engine
    host, run = _wipe_calls()[call]
    eng = Engine(0)
    try:
        bufs = {k: dev(eng, v) for k, v in host.items()}
        run(eng, bufs); torch.cuda.synchronize()                        # warm-up: sizes the workspace
        ptr, size = C.c_void_p(), C.c_size_t()
        eng._check(eng.lib.ecsimd_hip_workspace_info(eng.ctx, C.byref(ptr), C.byref(size)), "workspace_info")
        assert ptr.value and size.value
        fill = np.full(size.value, 0xA5, dtype=np.uint8)

        def refill():
            eng._bind_stream()
            eng._check(eng.lib.ecsimd_hip_memcpy_h2d(eng.ctx, ptr, fill.ctypes.data_as(C.c_void_p), C.c_size_t(size.value)), "memcpy_h2d")

        def zeroed_prefix():
            ws = eng.workspace_bytes()
            assert ws.size == size.value, "the workspace did not move"
            nz = np.flatnonzero(ws)
            prefix = int(nz[0]) if nz.size else ws.size
            assert (ws[prefix:] == 0xA5).all(), f"{call}: bytes behind the zeroed prefix of {prefix} were written and not wiped"
            return prefix

        refill(); assert zeroed_prefix() == 0                           # the readback sees the fill
        run(eng, bufs); torch.cuda.synchronize()
        eager = zeroed_prefix()
        assert 0 < eager <= size.value
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                out = run(eng, bufs)
        torch.cuda.synchronize()
        for _ in range(2):
            refill()
            g.replay(); torch.cuda.synchronize()
            assert zeroed_prefix() == eager, call
        del out, g
    finally:
        eng.close()


# ---- the calls that need the host refuse, and leave the capture valid
def _refuse_sync(eng, t): eng.sync()
def _refuse_malloc(eng, t): eng._check(eng.lib.ecsimd_hip_malloc(eng.ctx, C.byref(t["fresh"]), C.c_size_t(64)), "malloc")
def _refuse_free(eng, t): eng._check(eng.lib.ecsimd_hip_free(eng.ctx, t["spare"]), "free")
def _refuse_h2d(eng, t): eng._check(eng.lib.ecsimd_hip_memcpy_h2d(eng.ctx, C.c_void_p(t["dev"].data_ptr()), t["host"].ctypes.data_as(C.c_void_p), C.c_size_t(64)), "memcpy_h2d")
def _refuse_d2h(eng, t): eng._check(eng.lib.ecsimd_hip_memcpy_d2h(eng.ctx, t["host"].ctypes.data_as(C.c_void_p), C.c_void_p(t["dev"].data_ptr()), C.c_size_t(64)), "memcpy_d2h")
def _refuse_mask_count(eng, t): eng.mask_count(t["dev"])
def _refuse_scalar_mult_host(eng, t): eng.scalar_mult_host(P256, t["k"], flags=OUT_AFFINE)
def _refuse_merkle_root(eng, t): eng.btc_merkle_root(t["leaves"], [3, 1])
def _refuse_peak(eng, t): eng.peak_mad32(16)


REFUSES_CASES = {"sync": _refuse_sync, "malloc": _refuse_malloc, "free": _refuse_free, "memcpy_h2d": _refuse_h2d, "memcpy_d2h": _refuse_d2h, "mask_count": _refuse_mask_count,
                 "scalar_mult_host": _refuse_scalar_mult_host, "btc_merkle_root": _refuse_merkle_root, "peak_mad32": _refuse_peak}


def test_host_bound_calls_refuse_under_capture_and_leave_it_valid():
    """Every REFUSES name once inside one capture, then a capturable call: each refusal names capture, the capture ends without error, the replay is right."""
    import torch
    from ecsimd_amd import Engine, EcsimdHipError
    eng = Engine(0)
    try:
        rng = random.Random(1600)
        msgs = torch.from_numpy(np.frombuffer(rng.randbytes(N * 50), dtype=np.uint8).reshape(N, 50).copy()).to(eng.tdev)
        spare = C.c_void_p()
        eng._check(eng.lib.ecsimd_hip_malloc(eng.ctx, C.byref(spare), C.c_size_t(64)), "malloc")
        t = dict(spare=spare, fresh=C.c_void_p(), dev=torch.ones(64, dtype=torch.uint8, device=eng.tdev), host=np.zeros(64, dtype=np.uint8), k=limbs([1, 2, 3, 4]),
                 leaves=dev(eng, limbs([5, 6, 7, 8])))
        for name, call in REFUSES_CASES.items():                        # outside a capture every one of them works
            call(eng, dict(t, spare=t["fresh"]) if name == "free" else t)                       # (free: the block malloc has just handed out)
        assert t["fresh"].value
        t["fresh"] = C.c_void_p()
        eng.sha256(msgs); torch.cuda.synchronize()
        said = {}
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for name, call in REFUSES_CASES.items():
                    eng._bind_stream()
                    try:
                        call(eng, t)
                        said[name] = "it did not refuse"
                    except EcsimdHipError as exc:
                        said[name] = str(exc)
                e = eng.sha256(msgs)
        torch.cuda.synchronize()                                        # the capture ended without error
        assert all("capture" in m and "(-1)" in m for m in said.values()), said
        msgs.copy_(torch.from_numpy(np.frombuffer(rng.randbytes(N * 50), dtype=np.uint8).reshape(N, 50).copy()).to(eng.tdev))
        g.replay(); torch.cuda.synchronize()
        assert digests(npy(e)) == [hashlib.sha256(bytes(m)).digest() for m in msgs.cpu().numpy()]
        eng._bind_stream()
        eng._check(eng.lib.ecsimd_hip_free(eng.ctx, spare), "free")    # and outside the capture the block is freed
        del g
    finally:
        eng.close()


# ---- two torch streams, two calls that share and wipe the workspace
def test_switching_streams_orders_the_newer_calls_too(engine):
    """ecdsa_sign_deterministic on stream A and schnorr_verify on stream B, three times alternating with no synchronisation between them: the second must
    not start on the shared workspace before the first has wiped it.  Results equal the eager ones and the models."""
    import torch
    rng = random.Random(1700); c = CURVE_PARAMS[K1]
    e, d = [rng.getrandbits(256) for _ in range(N)], rand_scalars(rng, N, NK1)
    msgs = [rng.randbytes(32) for _ in range(N)]
    sigs = {j: bip340_model.sign(rng.randrange(1, NK1), msgs[j], rng.getrandbits(256)) for j in SAMPLE}
    px, r, s = ([sigs[j][q] if j in sigs else rng.getrandbits(255) for j in range(N)] for q in range(3))
    s[SAMPLE[3]] ^= 1
    te, td, tpx, tr, ts = (dev(engine, limbs(v)) for v in (e, d, px, r, s))
    tm = dev(engine, np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(N, 32).copy())
    ea = engine.ecdsa_sign_deterministic(K1, te, td); eb = engine.schnorr_verify(tpx, tm, tr, ts)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(sa):
            ga = engine.ecdsa_sign_deterministic(K1, te, td)
        with torch.cuda.stream(sb):
            gb = engine.schnorr_verify(tpx, tm, tr, ts)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(ga, ea)) and torch.equal(gb, eb)
    gr, gs, gv = arr_to_ints(npy(ea[0])), arr_to_ints(npy(ea[1])), npy(ea[2]).tolist()
    assert npy(ea[3]).all()
    for j in SAMPLE:
        assert (gr[j], gs[j], gv[j]) == rfc6979_model.sign(c, e[j], d[j])[:3], j
        assert int(eb[j]) == int(j != SAMPLE[3]) == int(bip340_model.verify(px[j], msgs[j], r[j], s[j])), j
