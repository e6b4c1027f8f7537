"""Keccak-f[1600] and the Keccak[512] sponge on Python integers: the model the device's k_keccak.hip is tested against.

The pad byte is a parameter: 0x01 is the original Keccak padding Ethereum uses (keccak256 below), 0x06 is NIST's SHA-3 -- the two share the permutation
and the rate, so hashlib.sha3_256 checks everything here but that one byte (tests/test_keccak_cpu.py).  No dependencies; slow on purpose.
"""
MASK = (1 << 64) - 1
RHO = [0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14]      # lane (x, y) at x + 5 y


def _round_constants():
    out, r = [], 1
    for _ in range(24):
        c = 0
        for j in range(7):                                    # the LFSR x^8 + x^6 + x^5 + x^4 + 1 feeds bit 2^j - 1
            if r & 1:
                c |= 1 << ((1 << j) - 1)
            r = ((r << 1) ^ (0x71 if r & 0x80 else 0)) & 0xFF
        out.append(c)
    return out


RC = _round_constants()


def rotl(v, n):
    return ((v << n) | (v >> (64 - n))) & MASK if n else v


def keccak_f1600(a):
    """a: 25 lanes (x + 5 y); returns the permuted 25 lanes."""
    for rc in RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1) for x in range(5)]
        a = [a[i] ^ d[i % 5] for i in range(25)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl(a[x + 5 * y], RHO[x + 5 * y])
        a = [b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & MASK & b[(x + 2) % 5 + 5 * y]) for y in range(5) for x in range(5)]
        a[0] ^= rc
    return a


def sponge256(data: bytes, pad: int, rate: int = 136) -> bytes:
    """32 bytes out of the sponge with capacity 512: `pad` right behind the message, zeros, bit 7 of the block's last byte."""
    block = bytearray(data) + bytes([pad]) + bytes(-(len(data) + 1) % rate)
    block[-1] ^= 0x80
    a = [0] * 25
    for off in range(0, len(block), rate):
        for j in range(rate // 8):
            a[j] ^= int.from_bytes(block[off + 8 * j:off + 8 * j + 8], "little")
        a = keccak_f1600(a)
    return b"".join(v.to_bytes(8, "little") for v in a[:4])


def keccak256(data: bytes) -> bytes:
    return sponge256(data, 0x01)


def sha3_256(data: bytes) -> bytes:
    return sponge256(data, 0x06)


def eth_address(x: int, y: int) -> bytes:
    """The Ethereum address of the public key (x, y): the last 20 bytes of Keccak-256 over its 64 big-endian bytes."""
    return keccak256(x.to_bytes(32, "big") + y.to_bytes(32, "big"))[12:]
