"""PBKDF2 with HMAC-SHA-512 as RFC 8018 section 5.2 writes it, and the BIP-39 seed: the host model the GPU tests of ecsimd_hip_pbkdf2_hmac_sha512 and
ecsimd_hip_bip39_seed take their expected values from.

    DK = T_1 || T_2 || ... || T_l<0 .. r - 1>          l = ceil(dkLen / hLen), r = dkLen - (l - 1) hLen
    T_i = F(P, S, c, i) = U_1 ^ U_2 ^ ... ^ U_c
    U_1 = PRF(P, S || INT(i)),  U_j = PRF(P, U_{j - 1})

The PRF is hmac.new(P, ., sha512).  hashlib.pbkdf2_hmac is NOT called here: it is the second, independent expectation tests/test_bip39_cpu.py holds this
file to.  BIP-39: seed = PBKDF2(password = the sentence, salt = "mnemonic" || passphrase, c = 2048, dkLen = 64), both taken as bytes (NFKD, the word list and the
checksum are the caller's).
"""
import hashlib
import hmac

H_LEN = 64
BIP39_ITERATIONS = 2048
BIP39_SALT_PREFIX = b"mnemonic"


def prf(password, data):
    return hmac.new(password, data, hashlib.sha512).digest()


def u_chain(password, salt, iterations, index):
    """U_1 .. U_c of block `index` (counted from 1)."""
    u = prf(password, salt + index.to_bytes(4, "big"))
    yield u
    for _ in range(iterations - 1):
        u = prf(password, u)
        yield u


def f(password, salt, iterations, index):
    t = 0
    for u in u_chain(password, salt, iterations, index):
        t ^= int.from_bytes(u, "big")
    return t.to_bytes(H_LEN, "big")


def pbkdf2_hmac_sha512(password, salt, iterations, dk_bytes):
    if iterations < 1 or dk_bytes < 1:
        raise ValueError("iterations and dk_bytes are at least 1")
    blocks = (dk_bytes + H_LEN - 1) // H_LEN
    return b"".join(f(password, salt, iterations, i) for i in range(1, blocks + 1))[:dk_bytes]


def bip39_seed(mnemonic_bytes, passphrase_bytes=b""):
    return pbkdf2_hmac_sha512(mnemonic_bytes, BIP39_SALT_PREFIX + passphrase_bytes, BIP39_ITERATIONS, 64)


if __name__ == "__main__":
    import sys
    print(bip39_seed(sys.argv[1].encode(), (sys.argv[2] if len(sys.argv) > 2 else "").encode()).hex())
