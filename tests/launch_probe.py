"""The launch-level probe: tests/cpp/launch_probe.hip built into build/tests/ and loaded beside the library, one Python function per wrapper.

The kernels behind BIP-32, BIP-340, the Taproot tweaks and the recoverable signatures take the group order as a kernel ARGUMENT; the C ABI always passes
secp256k1's.  The probe calls the library's exported launchers one level below the C ABI, so a test can pass another order (tests/test_gpu_launch_tails.py
says which and why).  Nothing here is part of the product, and nothing here computes an expected value.

Tensors in and out are torch tensors on engine.tdev: 256-bit values as (n, 4) int64 (the engine's convention), masks and bytes as uint8, indices as int32.
Launches go to the null stream; every function synchronises through torch before it returns.
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "launch_probe.hip")
CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
OUT = os.path.join(ROOT, "build", "tests", "liblaunch_probe.so")
WRAPPERS = ("bip32_master", "bip32_ckd_priv", "bip32_ckd_pub_front", "bip32_ckd_pub_accept", "schnorr_verify_front", "schnorr_nonce", "schnorr_finish", "tweak_front",
            "taproot_seckey", "sign_recovery_id", "ecdsa_sign_scalars", "x_mod_n_equals", "gc_x_mod_n_equals")
GMOD_PRIME, GMOD_3MOD4 = 1, 2
TWEAK_KEY_PATH, TWEAK_MERKLE_ROOT = 1, 2


def build_probe(force=False):
    """The path of the probe, rebuilt when its source, kernels.h, gfield.cuh (with field.cuh behind it) or the library is newer -- or whatever the file
    times say, with force."""
    import ecsimd_amd
    if not os.path.exists(ecsimd_amd.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    libdir = os.path.join(ROOT, "ecsimd_amd")
    newest = max(os.path.getmtime(p) for p in [SRC, ecsimd_amd.lib_path()] + [os.path.join(CSRC, f) for f in ("kernels.h", "gfield.cuh", "field.cuh")])
    if force or not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        # host code only: the probe has no device code of its own, and an undefined launcher fails the link here (-z defs) instead of at the first call.
        # Linked beside the target and renamed over it: a process that has the old file loaded keeps its mapping.
        tmp = f"{OUT}.{os.getpid()}.tmp"
        subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unused-function", "-I", CSRC, SRC,
                        "-o", tmp, "-Wl,-z,defs", "-L", libdir, "-lecsimd_hip", "-Wl,-rpath,$ORIGIN/../../ecsimd_amd"], check=True)
        os.replace(tmp, OUT)
    return OUT


def gmod_constants(p, prime=False):
    """What capi.hip's make_gmod derives of an odd modulus 3 <= p < 2^256, as Python integers: the fields of gfield.cuh's gmod by name."""
    assert p & 1 and 3 <= p < 1 << 256
    R = 1 << 256
    inv32 = pow(p, -1, 1 << 32)
    return dict(p=p, r=R % p, rsq=R * R % p, negr=(p - R % p) % p, r3=pow(R, 3, p), pm2=p - 2, psqrt=(p + 1) // 4,
                p30=[(p >> (30 * i)) & (0x3fffffff if i < 8 else 0xffff) for i in range(9)],
                pinv30=inv32 & 0x3fffffff, mprime=(-inv32) % (1 << 32), flags=(GMOD_PRIME if prime else 0) | (GMOD_3MOD4 if p & 3 == 3 else 0))


def _words(v):
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)]


class Probe:
    def __init__(self, engine):
        """engine: the ecsimd_amd.Engine of the test session -- its constructor has loaded the library this probe links against."""
        self.engine, self.torch = engine, engine.torch
        self.lib = C.CDLL(build_probe())
        for name in WRAPPERS:
            getattr(self.lib, "probe_" + name).restype = C.c_int

    # ---- arguments
    def _order(self, n):
        return (C.c_uint32 * 8)(*_words(n))

    def _gmod(self, n, prime):
        g = gmod_constants(n, prime)
        consts = [w for name in ("p", "r", "rsq", "negr", "r3", "pm2", "psqrt") for w in _words(g[name])]
        return (C.c_uint32 * 56)(*consts), (C.c_int32 * 9)(*g["p30"]), (C.c_uint32 * 3)(g["pinv30"], g["mprime"], g["flags"])

    def _p(self, t, rows, width=4):
        """The device pointer of an operand of `rows` lanes (None: a null pointer), shape and place checked as Engine._ptr does."""
        torch = self.torch
        if t is None:
            return C.c_void_p(0)
        assert t.is_cuda and t.device == self.engine.tdev and t.is_contiguous() and int(t.shape[0]) == rows, (t.device, t.shape, rows)
        if width == 4:
            assert t.dtype in (torch.int64, torch.uint64) and t.dim() == 2 and t.shape[1] == 4, (t.dtype, t.shape)
        elif width == 1:
            assert t.dtype == torch.uint8 and t.dim() == 1, (t.dtype, t.shape)
        else:
            assert t.dtype in (torch.int32, torch.uint32) and t.dim() == 1, (t.dtype, t.shape)
        return C.c_void_p(t.data_ptr())

    def _msgs(self, m, rows):
        """(pointer, bytes, stride) of a 2-D uint8 tensor with one message per row; the rows may be a column slice of a wider array (stride > bytes)."""
        assert m.is_cuda and m.dtype == self.torch.uint8 and m.dim() == 2 and int(m.shape[0]) == rows and m.stride(1) == 1 and m.stride(0) >= m.shape[1], (m.shape, m.stride())
        return C.c_void_p(m.data_ptr()), C.c_size_t(int(m.shape[1])), C.c_size_t(int(m.stride(0)))

    def _e(self, n):
        return self.engine.empty(n)

    def _f(self, n):
        return self.torch.zeros((n,), dtype=self.torch.uint8, device=self.engine.tdev)

    def _run(self, name, *args):
        self.torch.cuda.synchronize(self.engine.tdev)           # the inputs were made on torch's stream, the launch goes to the null stream
        rc = getattr(self.lib, "probe_" + name)(*args)
        self.torch.cuda.synchronize(self.engine.tdev)
        assert rc == 0, f"probe_{name}: hipGetLastError() = {rc}"

    # ---- one function per wrapper
    def bip32_master(self, order, seeds):
        n = int(seeds.shape[0]); k, c, ok = self._e(n), self._e(n), self._f(n)
        self._run("bip32_master", self._order(order), *self._msgs(seeds, n), self._p(k, n), self._p(c, n), self._p(ok, n, 1), C.c_size_t(n))
        return k, c, ok

    def bip32_ckd_priv(self, order, k_par, c_par, index, xP=None, yP=None, prime=False):
        n = int(k_par.shape[0]); k, c, ok = self._e(n), self._e(n), self._f(n)
        self._run("bip32_ckd_priv", *self._gmod(order, prime), self._p(k_par, n), self._p(c_par, n), self._p(index, n, 0), C.c_uint32(0), self._p(xP, n), self._p(yP, n),
                  self._p(k, n), self._p(c, n), self._p(ok, n, 1), C.c_size_t(n))
        return k, c, ok

    def bip32_ckd_pub_front(self, order, qx, qy, c_par, index):
        n = int(qx.shape[0]); x, y, t, c, valid = self._e(n), self._e(n), self._e(n), self._e(n), self._f(n)
        self._run("bip32_ckd_pub_front", self._order(order), self._p(qx, n), self._p(qy, n), self._p(c_par, n), self._p(index, n, 0), C.c_uint32(0), self._p(x, n), self._p(y, n),
                  self._p(t, n), self._p(c, n), self._p(valid, n, 1), C.c_size_t(n))
        return x, y, t, c, valid

    def bip32_ckd_pub_accept(self, ax, ay, jz, valid, c_child):
        """c_child is written in place (the kernel clears it where ok = 0) and returned with the rest."""
        n = int(ax.shape[0]); cx, cy, ok = self._e(n), self._e(n), self._f(n)
        self._run("bip32_ckd_pub_accept", self._p(ax, n), self._p(ay, n), self._p(jz, n), self._p(valid, n, 1), self._p(cx, n), self._p(cy, n), self._p(c_child, n),
                  self._p(ok, n, 1), C.c_size_t(n))
        return cx, cy, c_child, ok

    def schnorr_verify_front(self, order, px, r, s, msgs):
        n = int(px.shape[0]); u1, u2, x, y, valid = self._e(n), self._e(n), self._e(n), self._e(n), self._f(n)
        self._run("schnorr_verify_front", self._order(order), self._p(px, n), self._p(r, n), self._p(s, n), *self._msgs(msgs, n), self._p(u1, n), self._p(u2, n), self._p(x, n),
                  self._p(y, n), self._p(valid, n, 1), C.c_size_t(n))
        return u1, u2, x, y, valid

    def schnorr_nonce(self, order, d, aux, px, py, msgs):
        n = int(d.shape[0]); k0 = self._e(n)
        self._run("schnorr_nonce", self._order(order), self._p(d, n), self._p(aux, n), self._p(px, n), self._p(py, n), *self._msgs(msgs, n), self._p(k0, n), C.c_size_t(n))
        return k0

    def schnorr_finish(self, order, d, k0, xP, yP, xR, yR, msgs, want_px=True, prime=False):
        n = int(d.shape[0]); r, s, ok = self._e(n), self._e(n), self._f(n); px = self._e(n) if want_px else None
        self._run("schnorr_finish", *self._gmod(order, prime), self._p(d, n), self._p(k0, n), self._p(xP, n), self._p(yP, n), self._p(xR, n), self._p(yR, n),
                  *self._msgs(msgs, n), self._p(px, n), self._p(r, n), self._p(s, n), self._p(ok, n, 1), C.c_size_t(n))
        return px, r, s, ok

    def tweak_front(self, order, mode, px, merkle=None):
        n = int(px.shape[0]); x, y, t, valid = self._e(n), self._e(n), self._e(n), self._f(n)
        self._run("tweak_front", self._order(order), C.c_int(mode), self._p(px, n), self._p(merkle, n), self._p(x, n), self._p(y, n), self._p(t, n), self._p(valid, n, 1),
                  C.c_size_t(n))
        return x, y, t, valid

    def taproot_seckey(self, order, d, merkle, xP, yP, want_px=True, prime=False):
        n = int(d.shape[0]); d_out, ok = self._e(n), self._f(n); px = self._e(n) if want_px else None
        self._run("taproot_seckey", *self._gmod(order, prime), self._p(d, n), self._p(merkle, n), self._p(xP, n), self._p(yP, n), self._p(d_out, n), self._p(px, n),
                  self._p(ok, n, 1), C.c_size_t(n))
        return d_out, px, ok

    def sign_recovery_id(self, order, x, y, s, ok, low_s):
        """s is replaced in place where the low-s rule asks for it, and returned with v."""
        n = int(x.shape[0]); v = self._f(n)
        self._run("sign_recovery_id", self._order(order), self._p(x, n), self._p(y, n), self._p(s, n), self._p(ok, n, 1), self._p(v, n, 1), C.c_size_t(n), C.c_int(int(bool(low_s))))
        return s, v

    def ecdsa_sign_scalars(self, order, e, d, k, x, prime=True):
        n = int(e.shape[0]); r, s, ok = self._e(n), self._e(n), self._f(n)
        self._run("ecdsa_sign_scalars", *self._gmod(order, prime), self._p(e, n), self._p(d, n), self._p(k, n), self._p(x, n), self._p(r, n), self._p(s, n), self._p(ok, n, 1),
                  C.c_size_t(n))
        return r, s, ok

    def x_mod_n_equals(self, curve, x, finite, r):
        n = int(x.shape[0]); ok = self._f(n)
        self._run("x_mod_n_equals", C.c_int(curve), self._p(x, n), self._p(finite, n, 1), self._p(r, n), self._p(ok, n, 1), C.c_size_t(n))
        return ok

    def gc_x_mod_n_equals(self, order, x, finite, r, prime=True):
        n = int(x.shape[0]); ok = self._f(n)
        self._run("gc_x_mod_n_equals", *self._gmod(order, prime), self._p(x, n), self._p(finite, n, 1), self._p(r, n), self._p(ok, n, 1), C.c_size_t(n))
        return ok


def ints_to_device(engine, values):
    """A list of integers below 2^256 as an (n, 4) device tensor."""
    a = np.array([[(v >> (64 * j)) & 0xffffffffffffffff for j in range(4)] for v in values], dtype=np.uint64).reshape(len(values), 4)
    return engine.to_device(a)


def device_to_ints(t):
    a = t.detach().cpu().numpy().view(np.uint64)
    return [sum(int(a[i, j]) << (64 * j) for j in range(4)) for i in range(a.shape[0])]
