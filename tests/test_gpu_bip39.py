"""GPU suite: PBKDF2-HMAC-SHA-512 and the BIP-39 seed (k_pbkdf2.hip).

Every expectation comes from hashlib.pbkdf2_hmac, tools/pbkdf2_model.py (pinned to hashlib and to the published vectors by tests/test_bip39_cpu.py) or the
engine's OTHER calls (hmac_sha512, bip32_*, scalar_mult_base, eth_address) -- never from the call under test.  Every lane of every batch is compared unless a
test says otherwise.
"""
import ctypes as C
import hashlib
import json
import os
import random
import re
import sys

import numpy as np
import pytest

from helpers import SECP256K1, arr_to_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bip32_model       # noqa: E402
import keccak_model      # noqa: E402
import pbkdf2_model as model  # noqa: E402

pytestmark = pytest.mark.gpu
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "bip39_vectors.json")))
SLICE = int(re.search(r"ECSIMD_HIP_PBKDF2_SLICE\s*=\s*(\d+)", open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read()).group(1))
LANE_CHUNK = 1 << int(re.search(r"PBKDF2_UNITS = \(size_t\)1 << (\d+);", open(os.path.join(ROOT, "ecsimd_amd", "csrc", "capi.hip")).read()).group(1))
PW_LENGTHS = [0, 1, 111, 112, 127, 128, 129, 215, 256]
SALT_LENGTHS = [0, 1, 8, 107, 108, 123, 124, 125, 240]       # 107 / 108: the counter meets the padding boundary of the first block; 123 .. 125: it straddles the block's end
DK = [1, 63, 64, 65, 128, 200]
OUT_AFFINE, WINDOWED, CONSTANT_TIME = 2, 4, 128
H = 1 << 31


def ref(pw, salt, c, dk):
    return hashlib.pbkdf2_hmac("sha512", pw, salt, c, dk)


def rows(engine, host, stride, offset, n, length):
    """`host` (bytes of n records `stride` apart) on the device `offset` bytes behind a 16-byte aligned base, as the (n, length) strided view the engine takes."""
    import torch
    raw = torch.zeros(offset + n * stride + 16, dtype=torch.uint8, device=engine.tdev)
    assert raw.data_ptr() % 16 == 0
    if host:
        raw[offset:offset + len(host)] = torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).to(engine.tdev)
    return raw.as_strided((n, length), (stride, 1), offset)


def records(rng, n, length, unit, padded=True):
    """(host bytes, stride, the n strings): random bytes everywhere, between the strings as well."""
    stride = (length + (7 if padded else 0) + unit - 1) // unit * unit
    if padded and stride == length:
        stride += unit
    host = rng.randbytes(n * stride)
    return host, stride, [host[i * stride:i * stride + length] for i in range(n)]


def packed(engine, strings, width=None):
    """Strings of any lengths as rows of one (n, width) tensor, zero-padded, and their lengths."""
    import torch
    width = max([len(s) for s in strings] + [1]) if width is None else width
    host = np.zeros((len(strings), width), dtype=np.uint8)
    for i, s in enumerate(strings):
        host[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return torch.from_numpy(host).to(engine.tdev), torch.from_numpy(np.array([len(s) for s in strings], dtype=np.int32)).to(engine.tdev)


def keys(t):
    return [bytes(r) for r in t.cpu().numpy()]


def derive(engine, rng, n, pw_len, salt_len, c, dk, offset=0, unit=4):
    """One call over n lanes of random strings of the given lengths laid out (offset, unit); returns (got, want)."""
    phost, pstride, pws = records(rng, n, pw_len, unit)
    shost, sstride, salts = records(rng, n, salt_len, unit)
    got = engine.pbkdf2_hmac_sha512(rows(engine, phost, pstride, offset, n, pw_len), rows(engine, shost, sstride, offset, n, salt_len), c, dk)
    return keys(got), [ref(p, s, c, dk) for p, s in zip(pws, salts)]


# ---- 1. lengths and alignments, one axis at a time
@pytest.mark.parametrize("c", [1, 2, 3, 7])
def test_every_password_and_salt_length_equals_hashlib(engine, c):
    rng = random.Random(3900 + c)
    for pw_len in PW_LENGTHS:
        got, want = derive(engine, rng, 130, pw_len, 12, c, 64)
        assert got == want, ("password", pw_len, c)
    for salt_len in SALT_LENGTHS:
        got, want = derive(engine, rng, 130, 24, salt_len, c, 64)
        assert got == want, ("salt", salt_len, c)


@pytest.mark.parametrize("c", [1, 2, 3, 7])
def test_every_key_length_leaves_the_bytes_between_the_keys_alone(engine, c):
    import torch
    rng = random.Random(3950 + c)
    n = 130
    phost, pstride, pws = records(rng, n, 24, 4)
    shost, sstride, salts = records(rng, n, 12, 4)
    pv, sv = rows(engine, phost, pstride, 0, n, 24), rows(engine, shost, sstride, 0, n, 12)
    for dk in DK:
        for stride in (dk + 3, (dk + 8) // 4 * 4):                # byte stores and word stores
            out = torch.full((n, stride), 0xA5, dtype=torch.uint8, device=engine.tdev)
            engine.pbkdf2_hmac_sha512(pv, sv, c, dk, out=out)
            host = out.cpu().numpy()
            assert [bytes(r[:dk]) for r in host] == [ref(p, s, c, dk) for p, s in zip(pws, salts)], (dk, stride, c)
            assert (host[:, dk:] == 0xA5).all(), (dk, stride, c)


@pytest.mark.parametrize("offset, unit", [(0, 4), (4, 4), (1, 1), (3, 1)])
def test_every_alignment_equals_hashlib(engine, offset, unit):
    """unit 4 on a base that is a multiple of 4: word loads; an odd base or stride: byte loads.  Random bytes lie between two records."""
    rng = random.Random(3990 + 10 * offset + unit)
    for c in (1, 2, 3, 7):
        for pw_len, salt_len in ((24, 12), (215, 124), (129, 240), (8, 107)):
            got, want = derive(engine, rng, 130, pw_len, salt_len, c, 65, offset, unit)
            assert got == want, (c, pw_len, salt_len, offset, unit)


# ---- 2. per-lane lengths
def test_per_lane_lengths(engine):
    import torch
    rng = random.Random(3902)
    n = 130
    plens = [rng.randrange(257) for _ in range(n)]
    slens = [rng.randrange(241) for _ in range(n)]
    plens[:6] = [128, 129, 0, 256, 128, 129]
    slens[:6] = [107, 108, 124, 0, 240, 123]
    phost, pstride, prec = records(rng, n, 256, 4)
    shost, sstride, srec = records(rng, n, 240, 1)
    pv, sv = rows(engine, phost, pstride, 4, n, 256), rows(engine, shost, sstride, 3, n, 240)
    given_p, given_s = list(plens), list(slens)
    given_p[7], given_s[8] = pstride + 1000, 0x7fffffff            # above the stride: read as the stride
    plens[7], slens[8] = pstride, sstride
    whole = phost + bytes(16), shost + bytes(16)
    want = [ref(whole[0][i * pstride:i * pstride + plens[i]], whole[1][i * sstride:i * sstride + slens[i]], 3, 72) for i in range(n)]
    as_t = lambda v: torch.from_numpy(np.array(v, dtype=np.int32)).to(engine.tdev)
    got = engine.pbkdf2_hmac_sha512(pv, sv, 3, 72, pw_lens=as_t(given_p), salt_lens=as_t(given_s))
    assert keys(got) == want


# ---- 3. one salt for the call
def test_one_salt_for_the_call_equals_that_salt_on_every_lane(engine):
    import torch
    rng = random.Random(3903)
    n = 130
    phost, pstride, pws = records(rng, n, 31, 1)
    pv = rows(engine, phost, pstride, 1, n, 31)
    for salt_len in (0, 5, 124, 130):
        salt = rng.randbytes(salt_len)
        one = torch.from_numpy(np.frombuffer(salt, dtype=np.uint8).copy()).to(engine.tdev)
        each = one.repeat(n, 1) if salt_len else torch.zeros((n, 0), dtype=torch.uint8, device=engine.tdev)
        a, b = keys(engine.pbkdf2_hmac_sha512(pv, one, 2, 100)), keys(engine.pbkdf2_hmac_sha512(pv, each, 2, 100))
        assert a == b == [ref(p, salt, 2, 100) for p in pws], salt_len


# ---- 4. the published seeds among random sentences
def sentence(rng, words):
    return " ".join("".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randrange(3, 9))) for _ in range(words)).encode()


def test_bip39_seed_on_the_published_vectors_among_random_sentences(engine):
    rng = random.Random(3904)
    n = 130
    sentences = [sentence(rng, rng.choice((12, 15, 18, 21, 24))) for _ in range(n)]
    phrases = [rng.randbytes(rng.randrange(0, 40)) for _ in range(n)]
    for lane, name in ((0, "trezor"), (64, "empty_passphrase"), (129, "long_sentence")):
        sentences[lane], phrases[lane] = KAT[name]["mnemonic"].encode(), KAT[name]["passphrase"].encode()
    assert len(sentences[129]) > 128
    mt, ml = packed(engine, sentences)
    pt, pl = packed(engine, phrases)
    got = keys(engine.bip39_seed(mt, pt, ml, pl))
    assert got == [ref(s, b"mnemonic" + p, 2048, 64) for s, p in zip(sentences, phrases)]
    for lane, name in ((0, "trezor"), (64, "empty_passphrase"), (129, "long_sentence")):
        assert got[lane].hex() == KAT[name]["seed"], name
    # no passphrase at all, and one for the call
    same = [KAT["trezor"]["mnemonic"].encode()] * 3
    st, _ = packed(engine, same)
    assert [k.hex() for k in keys(engine.bip39_seed(st))] == [KAT["empty_passphrase"]["seed"]] * 3
    import torch
    trezor = torch.from_numpy(np.frombuffer(b"TREZOR", dtype=np.uint8).copy()).to(engine.tdev)
    assert [k.hex() for k in keys(engine.bip39_seed(st, trezor))] == [KAT["trezor"]["seed"]] * 3


# ---- 5. the slice boundary
@pytest.mark.parametrize("c", [SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 1])
def test_iteration_counts_around_the_slice_and_a_clean_workspace(c):
    """A context of its own: what its workspace holds afterwards is this call's.  65 lanes: a whole wave and a partial one."""
    from ecsimd_amd import Engine
    assert 65 * (2 * SLICE + 1) * 1.2e-6 < 5.0, "the reference's time: keep ECSIMD_HIP_PBKDF2_SLICE at or below 2^14 or shrink this test towards 65 lanes"
    eng = Engine(0)
    rng = random.Random(3905)
    got, want = derive(eng, rng, 65, 24, 12, c, 64)
    assert got == want, c
    ws = eng.workspace_bytes()
    if c > SLICE:
        assert ws.size >= 65 * 256 and not ws.any(), c
    else:
        assert ws.size == 0, "a derivation of at most one slice uses no workspace"
    eng.close()


# ---- 6. the lane-chunk boundary
def test_more_lanes_than_one_chunk(engine):
    import torch
    n = LANE_CHUNK + 5
    pw = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=engine.tdev)
    salt = bytes(range(40, 52))
    one = torch.from_numpy(np.frombuffer(salt, dtype=np.uint8).copy()).to(engine.tdev)
    got = engine.pbkdf2_hmac_sha512(pw, one, 1, 64)
    msg = torch.from_numpy(np.frombuffer(salt + b"\x00\x00\x00\x01", dtype=np.uint8).copy()).to(engine.tdev).repeat(n, 1)
    assert torch.equal(got, engine.hmac_sha512(pw, msg))           # c = 1: T_1 = U_1 = HMAC(P, S || INT(1)), every lane, on the device
    rng = random.Random(3906)
    lanes = [0, LANE_CHUNK - 1, LANE_CHUNK, n - 1] + [rng.randrange(n) for _ in range(60)]
    idx = torch.tensor(lanes, device=engine.tdev)
    for lane, k, p in zip(lanes, keys(got[idx]), keys(pw[idx])):
        assert k == ref(p, salt, 1, 64), lane


# ---- 7. two output blocks with the full loop
def test_two_output_blocks_at_2048_iterations(engine):
    rng = random.Random(3907)
    got, want = derive(engine, rng, 65, 40, 20, 2048, 128)
    assert got == want


# ---- 8. end to end
def test_from_the_sentence_to_the_ethereum_address(engine):
    import torch
    rng = random.Random(3908)
    n = 64
    sentences = [KAT["trezor"]["mnemonic"].encode()] + [sentence(rng, 12) for _ in range(n - 1)]
    phrases = [b"TREZOR"] + [rng.randbytes(rng.randrange(0, 20)) for _ in range(n - 1)]
    mt, ml = packed(engine, sentences)
    pt, pl = packed(engine, phrases)
    k, c, ok = engine.bip39_master(mt, pt, ml, pl)
    assert "%064x" % arr_to_ints(engine.to_numpy(k))[0] == KAT["trezor"]["master_k"]
    path = [H + 44, H + 60, H + 0, 0]
    k, c, ok2 = engine.bip32_derive_priv(k, c, path)
    index = torch.arange(n, dtype=torch.int32, device=engine.tdev)
    k, c, ok3 = engine.bip32_ckd_priv(k, c, index)
    assert bool((ok & ok2 & ok3).all())
    qx, qy = engine.scalar_mult_base(SECP256K1, k, OUT_AFFINE | WINDOWED | CONSTANT_TIME)[:2]
    got = [bytes(r) for r in engine.eth_address(qx, qy).cpu().numpy()]
    for i in range(n):
        hk, hc = bip32_model.master(model.bip39_seed(sentences[i], phrases[i]))
        hk, hc = bip32_model.derive(hk, hc, path + [i])
        x, y = bip32_model.mul_g(hk)
        assert got[i] == keccak_model.keccak256(x.to_bytes(32, "big") + y.to_bytes(32, "big"))[12:], i


# ---- 9. bad arguments
def test_bad_arguments_are_refused(engine):
    import torch
    from ecsimd_amd.engine import EcsimdHipError
    lib, ctx = engine.lib, engine.ctx
    buf = torch.zeros(4096, dtype=torch.uint8, device=engine.tdev)
    p = buf.data_ptr()
    fn = lib.ecsimd_hip_pbkdf2_hmac_sha512

    def call(pw=p, pw_bytes=8, pw_stride=8, pw_lens=0, salt=p + 1024, salt_bytes=8, salt_stride=8, salt_lens=0, c=1, out=p + 2048, dk=64, out_stride=64, n=4):
        return fn(ctx, C.c_void_p(pw), C.c_size_t(pw_bytes), C.c_size_t(pw_stride), C.c_void_p(pw_lens), C.c_void_p(salt), C.c_size_t(salt_bytes), C.c_size_t(salt_stride),
                  C.c_void_p(salt_lens), C.c_uint32(c), C.c_void_p(out), C.c_size_t(dk), C.c_size_t(out_stride), C.c_size_t(n))
    BAD = -1
    assert call() == 0
    assert call(c=0) == BAD and call(dk=0) == BAD and call(out_stride=63) == BAD
    assert call(pw_stride=7) == BAD and call(salt_stride=7) == BAD
    assert call(salt_stride=0, salt_lens=p + 3072) == BAD and call(salt_stride=0) == 0
    assert call(pw_lens=p + 3073) == BAD and call(salt_lens=p + 3074) == BAD and call(pw_lens=p + 3072, salt_lens=p + 3072) == 0
    assert call(out=p) == BAD and call(out=p + 1024) == BAD and call(out=p + 3072, pw_lens=p + 3072) == BAD
    assert call(pw=0) == BAD and call(salt=0) == BAD and call(out=0) == BAD
    assert call(pw_lens=p + 3072, pw_stride=(1 << 30) + 4) == BAD and call(salt_lens=p + 3072, salt_stride=1 << 32) == BAD      # with lens a lane may be as long as the stride
    assert call(pw=0, pw_bytes=0, pw_stride=0) == 0 and call(salt=0, salt_bytes=0, salt_stride=0) == 0
    assert call(n=0) == 0 and call(pw=0, salt=0, out=0, n=0) == 0
    seed = lib.ecsimd_hip_bip39_seed
    z = C.c_void_p(0)
    assert seed(ctx, C.c_void_p(p), C.c_size_t(8), C.c_size_t(8), z, z, C.c_size_t(0), C.c_size_t(0), z, C.c_void_p(p + 2048), C.c_size_t(4)) == 0
    assert seed(ctx, C.c_void_p(p), C.c_size_t(8), C.c_size_t(8), z, z, C.c_size_t(3), C.c_size_t(0), z, C.c_void_p(p + 2048), C.c_size_t(4)) == BAD
    assert seed(ctx, C.c_void_p(p), C.c_size_t(8), C.c_size_t(8), z, z, C.c_size_t(0), C.c_size_t(0), z, C.c_void_p(p), C.c_size_t(4)) == BAD
    engine.sync()
    # the engine: operands of different batch lengths
    pw = torch.zeros((5, 8), dtype=torch.uint8, device=engine.tdev)
    lens4 = torch.zeros((4,), dtype=torch.int32, device=engine.tdev)
    for bad in (lambda: engine.pbkdf2_hmac_sha512(pw, pw[:4], 1, 64), lambda: engine.pbkdf2_hmac_sha512(pw, pw, 1, 64, pw_lens=lens4),
                lambda: engine.pbkdf2_hmac_sha512(pw, pw, 1, 64, salt_lens=lens4), lambda: engine.bip39_seed(pw, pw[:4]), lambda: engine.bip39_seed(pw, mnemonic_lens=lens4),
                lambda: engine.bip39_master(pw, pw, passphrase_lens=lens4)):
        with pytest.raises(EcsimdHipError, match="batch length"):
            bad()
