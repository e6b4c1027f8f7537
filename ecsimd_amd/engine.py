"""ctypes binding of include/ecsimd_hip.h over torch device tensors.

Tensors are ``torch.int64`` (bit pattern of the u64 limbs) or ``torch.uint64`` of shape (n, 4)
[(n, 8) for 512-bit products], contiguous, on the engine's device.  Every method enqueues on
torch's CURRENT stream and returns without synchronising, like any torch op.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .flags import BIP32_ALL_HARDENED, ECDSA_LOW_S, ED25519_REJECT_SMALL_ORDER, ETH_REQUIRE_LOW_S

P256, SECP256K1 = 0, 1
CURVES = {"p256": P256, "secp256k1": SECP256K1}
# field ids of the two group orders (include/ecsimd_hip.h enum ecsimd_hip_field): accepted wherever a method below takes a field's `curve`
P256_ORDER, SECP256K1_ORDER = 2, 3
ORDER_FIELD = {P256: P256_ORDER, SECP256K1: SECP256K1_ORDER}
MODULUS_PRIME = 1

_HERE = os.path.dirname(os.path.abspath(__file__))


class EcsimdHipError(RuntimeError):
    pass


def lib_path() -> str:
    # ECSIMD_HIP_LIBRARY: another build of the SAME library (tools/ compares kernel variants with it); never a fallback
    return os.environ.get("ECSIMD_HIP_LIBRARY") or os.path.join(_HERE, "libecsimd_hip.so")


_SYMBOLS = None


def declared_symbols():
    """Every function name declared in include/ecsimd_hip.h (parsed from the header)."""
    global _SYMBOLS
    if _SYMBOLS is None:
        import re
        hdr = os.path.join(os.path.dirname(_HERE), "include", "ecsimd_hip.h")
        text = open(hdr).read()
        _SYMBOLS = sorted(set(re.findall(r"\b(ecsimd_hip_[a-z0-9_]+)\s*\(", text)))
    return _SYMBOLS


def declared_bls12_381_symbols():
    """Every function name declared in include/ecsimd_bls12_381.h (parsed from the header).  declared_symbols() stays the ecsimd_hip_* set, which the library's
    exports are compared with."""
    import re
    hdr = os.path.join(os.path.dirname(_HERE), "include", "ecsimd_bls12_381.h")
    return sorted(set(re.findall(r"\b(ecsimd_bls12_381_[a-z0-9_]+)\s*\(", open(hdr).read())))


def declared_bls12_381_g2_symbols():
    """Every function name declared in include/ecsimd_bls12_381_g2.h (parsed from the header): the ecsimd_bls381_g2_* set."""
    import re
    hdr = os.path.join(os.path.dirname(_HERE), "include", "ecsimd_bls12_381_g2.h")
    return sorted(set(re.findall(r"\b(ecsimd_bls381_g2_[a-z0-9_]+)\s*\(", open(hdr).read())))


def load_library() -> C.CDLL:
    path = lib_path()
    if not os.path.exists(path):
        raise EcsimdHipError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(there is no CPU fallback for the HIP path)")
    lib = C.CDLL(path)
    lib.ecsimd_hip_last_error.restype = C.c_char_p
    lib.ecsimd_hip_version.restype = C.c_char_p
    return lib


def _u64(v):
    return C.c_uint64(int(v) & 0xFFFFFFFFFFFFFFFF)


class MsmPlan(C.Structure):
    """ecsimd_msm_plan_t (include/ecsimd_msm.h)."""
    _fields_ = [("route", C.c_int), ("c", C.c_int), ("windows", C.c_int), ("buckets", C.c_uint32), ("L", C.c_uint32), ("m", C.c_uint32), ("max_chain", C.c_uint32),
                ("launches", C.c_int), ("workspace_bytes", C.c_size_t)]


class SchnorrBatchPlan(C.Structure):
    """ecsimd_schnorr_batch_plan_t (include/ecsimd_schnorr_batch.h)."""
    _fields_ = [("route", C.c_int), ("launches", C.c_int), ("workspace_bytes", C.c_size_t)]


class Ed25519BatchPlan(C.Structure):
    """ecsimd_ed25519_batch_plan_t (include/ecsimd_ed25519_batch.h)."""
    _fields_ = [("route", C.c_int), ("launches", C.c_int), ("workspace_bytes", C.c_size_t)]


class NttPlan(C.Structure):
    """ecsimd_ntt_plan_t (include/ecsimd_ntt.h)."""
    _fields_ = [("passes", C.c_int), ("log_radix", C.c_int * 24), ("lanes", C.c_int), ("lds_bytes", C.c_int), ("launches", C.c_int), ("workspace_bytes", C.c_size_t)]


# the conventional 2^32-th root of unity of BLS12-381's scalar field, 7^((r - 1) / 2^32): what ecsimd_ntt_bls12_381_fr returns
BLS12_381_FR_ROOT = 0x16a2a19edfe81f20d09b681922c813b4b63683508c2280b93829971f439f0d2b


def _limbs(v):
    return (C.c_uint64 * 4)(*[(int(v) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)])


def _from_limbs(l):
    return sum(int(l[i]) << (64 * i) for i in range(4))


class NttDomain:
    """An ecsimd_ntt_domain: the device tables of one (field, log_n, root, shift).  It belongs to the Engine that made it and is destroyed with close() or when
    it is collected -- before its Engine closes."""

    def __init__(self, engine, handle, field, log_n):
        self.engine, self.handle, self.field, self.log_n, self.n = engine, handle, field, log_n, 1 << log_n

    def close(self):
        if self.handle and self.engine.ctx:
            self.engine.lib.ecsimd_ntt_domain_destroy(self.engine.ctx, self.handle)
        self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One context (HIP stream owner) on one GPU."""

    def __init__(self, device: int = 0):
        import torch
        self.torch = torch
        self.lib = load_library()
        self.device = int(device)
        self.ctx = C.c_void_p()
        rc = self.lib.ecsimd_hip_init(C.c_int(self.device), C.byref(self.ctx))
        if rc != 0:
            raise EcsimdHipError(f"ecsimd_hip_init(device={device}) failed with {rc} "
                                 "(-2 = no gfx950 device visible; the HIP path has no CPU fallback)")
        self.tdev = torch.device("cuda", self.device)
        self._rows = set()      # batch lengths of the tensors handed to the call being assembled (see _ptr / _call)

    def close(self):
        if self.ctx:
            self.lib.ecsimd_hip_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- plumbing
    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.ecsimd_hip_last_error(self.ctx)
            raise EcsimdHipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def _bind_stream(self):
        s = self.torch.cuda.current_stream(self.tdev).cuda_stream
        self._check(self.lib.ecsimd_hip_set_stream(self.ctx, C.c_void_p(s)), "set_stream")

    def _ptr(self, t, words=4, dtype_ok=None):
        torch = self.torch
        if t is None:
            return C.c_void_p(0)
        assert t.is_cuda and t.device.index == self.device, "tensor on the wrong device"
        assert t.is_contiguous(), "tensor must be contiguous"
        if words:
            assert t.dtype in (torch.int64, torch.uint64) and t.dim() == 2 and t.shape[1] == words, (t.dtype, t.shape)
        else:
            assert t.dtype == torch.uint8 and t.dim() == 1
        self._rows.add(int(t.shape[0]))
        return C.c_void_p(t.data_ptr())

    def empty(self, n, words=4):
        return self.torch.empty((n, words), dtype=self.torch.int64, device=self.tdev)

    def flags(self, n):
        return self.torch.zeros((n,), dtype=self.torch.uint8, device=self.tdev)

    def to_device(self, arr):
        """numpy uint64 (n, w) -> device int64 tensor with the same bits."""
        a = np.ascontiguousarray(arr, dtype=np.uint64)
        return self.torch.from_numpy(a.view(np.int64)).to(self.tdev)

    def select_rows(self, t, rows):
        """t[rows] for a numpy index array (contiguous result on the device)."""
        return t[self.torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(t.device)].contiguous()

    @staticmethod
    def to_numpy(t):
        a = t.detach().cpu().numpy()
        return a if a.dtype == np.uint8 else a.view(np.uint64)

    def _call(self, name, *args):
        # The C ABI takes ONE length for all operands (in the reference it is a compile-time property of the type): a
        # shorter tensor would be read or written out of bounds on the device, so it is refused here.
        rows, self._rows = self._rows, set()
        if len(rows) > 1:
            raise EcsimdHipError(f"{name}: operands disagree on the batch length: {sorted(rows)}")
        self._bind_stream()
        self._check(getattr(self.lib, "ecsimd_hip_" + name)(self.ctx, *args), name)

    def set_ref_square_compat(self, on: bool):
        """ecsimd_hip_set_ref_square_compat: square like the reference's square() as written (mul.h:160-212)."""
        self._check(self.lib.ecsimd_hip_set_ref_square_compat(self.ctx, C.c_int(int(bool(on)))), "set_ref_square_compat")

    def sync(self):
        self._bind_stream()
        self._check(self.lib.ecsimd_hip_sync(self.ctx), "sync")

    def constant(self, curve, which):
        out = (C.c_uint64 * 4)()
        rc = self.lib.ecsimd_hip_get_constant(C.c_int(curve), C.c_int(which), out)
        if rc != 0:
            raise EcsimdHipError(f"get_constant({curve},{which}) -> {rc}")
        return np.array(list(out), dtype=np.uint64)

    # ---- L2
    def add(self, a, b):
        n = a.shape[0]; out = self.empty(n); f = self.flags(n)
        self._call("add", self._ptr(a), self._ptr(b), self._ptr(out), self._ptr(f, 0), C.c_size_t(n)); return out, f

    def sub(self, a, b):
        n = a.shape[0]; out = self.empty(n); f = self.flags(n)
        self._call("sub", self._ptr(a), self._ptr(b), self._ptr(out), self._ptr(f, 0), C.c_size_t(n)); return out, f

    def sub_if_above(self, a, p):
        n = a.shape[0]; out = self.empty(n)
        self._call("sub_if_above", self._ptr(a), self._ptr(p), self._ptr(out), C.c_size_t(n)); return out

    def cmp_eq(self, a, b):
        n = a.shape[0]; f = self.flags(n)
        self._call("cmp_eq", self._ptr(a, a.shape[1]), self._ptr(b, b.shape[1]), C.c_int(a.shape[1]), self._ptr(f, 0), C.c_size_t(n)); return f

    def mask_op(self, op, a, b=None):
        n = a.shape[0]; f = self.flags(n)
        self._call("mask_op", C.c_int(op), self._ptr(a, 0), self._ptr(b, 0), self._ptr(f, 0), C.c_size_t(n)); return f

    def mask_count(self, a):
        c = C.c_size_t(0)
        self._call("mask_count", self._ptr(a, 0), C.c_size_t(a.shape[0]), C.byref(c)); return int(c.value)

    def cmp_lt(self, a, b):
        n = a.shape[0]; f = self.flags(n)
        self._call("cmp_lt", self._ptr(a), self._ptr(b), self._ptr(f, 0), C.c_size_t(n)); return f

    def shift_left_one(self, a):
        n = a.shape[0]; out = self.empty(n); f = self.flags(n)
        self._call("shift_left_one", self._ptr(a), self._ptr(out), self._ptr(f, 0), C.c_size_t(n)); return out, f

    def mul(self, a, b):
        n = a.shape[0]; out = self.empty(n, 8)
        self._call("mul", self._ptr(a), self._ptr(b), self._ptr(out, 8), C.c_size_t(n)); return out

    def square(self, a):
        n = a.shape[0]; out = self.empty(n, 8)
        self._call("square", self._ptr(a), self._ptr(out, 8), C.c_size_t(n)); return out

    def if_else(self, mask, a, b):
        n = a.shape[0]; out = self.empty(n)
        self._call("if_else", self._ptr(mask, 0), self._ptr(a), self._ptr(b), self._ptr(out), C.c_size_t(n)); return out

    def swap_if(self, mask, a, b):
        self._call("swap_if", self._ptr(mask, 0), self._ptr(a), self._ptr(b), C.c_size_t(a.shape[0]))

    # ---- wire formats
    def _bytes_ptr(self, t):
        assert t.is_cuda and t.is_contiguous() and t.dtype == self.torch.uint8
        return C.c_void_p(t.data_ptr())

    def from_bytes_be(self, b):
        n = b.numel() // 32; out = self.empty(n)
        self._call("from_bytes_be", self._bytes_ptr(b), self._ptr(out), C.c_size_t(n)); return out

    def to_bytes_be(self, a):
        n = a.shape[0]; out = self.torch.empty((n, 32), dtype=self.torch.uint8, device=self.tdev)
        self._call("to_bytes_be", self._ptr(a), self._bytes_ptr(out), C.c_size_t(n)); return out

    def wide4_to_lanes(self, wides, record_bytes=128, offset_bytes=0, n_wides=None):
        """ecsimd_hip_wide4_to_lanes: a device uint8 tensor holding records with one reference wide (u64[limb * 4 + lane]) each -> (4 * wides, 4) elements."""
        n_wides = wides.numel() // record_bytes if n_wides is None else n_wides
        out = self.empty(4 * n_wides)
        self._call("wide4_to_lanes", self._bytes_ptr(wides), C.c_size_t(record_bytes), C.c_size_t(offset_bytes), self._ptr(out), C.c_size_t(n_wides)); return out

    def lanes_to_wide4(self, a, wides, record_bytes=128, offset_bytes=0):
        """ecsimd_hip_lanes_to_wide4: elements 4w .. 4w + 3 of `a` -> the wide at offset_bytes of record w of the device uint8 tensor `wides` (in place)."""
        self._call("lanes_to_wide4", self._ptr(a), self._bytes_ptr(wides), C.c_size_t(record_bytes), C.c_size_t(offset_bytes), C.c_size_t(a.shape[0] // 4)); return wides

    def mask_bit(self, a, bit):
        n = a.shape[0]; f = self.flags(n)
        self._call("mask_bit", self._ptr(a), C.c_int(bit), self._ptr(f, 0), C.c_size_t(n)); return f

    def sec1_encode(self, curve, x, y, compressed=False):
        n = x.shape[0]; out = self.torch.empty((n, 33 if compressed else 65), dtype=self.torch.uint8, device=self.tdev)
        self._call("sec1_encode", C.c_int(curve), self._ptr(x), self._ptr(y), self._bytes_ptr(out), C.c_size_t(n), C.c_int(int(compressed))); return out

    def sec1_decode(self, curve, rec, compressed=False):
        n = rec.shape[0]; x, y, ok = self.empty(n), self.empty(n), self.flags(n)
        self._call("sec1_decode", C.c_int(curve), self._bytes_ptr(rec), self._ptr(x), self._ptr(y), self._ptr(ok, 0), C.c_size_t(n), C.c_int(int(compressed))); return x, y, ok

    # ---- L3
    def _bin(self, name, curve, a, b):
        n = a.shape[0]; out = self.empty(n)
        self._call(name, C.c_int(curve), self._ptr(a), self._ptr(b), self._ptr(out), C.c_size_t(n)); return out

    def _un(self, name, curve, a, words=4):
        n = a.shape[0]; out = self.empty(n)
        self._call(name, C.c_int(curve), self._ptr(a, words), self._ptr(out), C.c_size_t(n)); return out

    def mod_add(self, curve, a, b): return self._bin("mod_add", curve, a, b)
    def mod_sub(self, curve, a, b): return self._bin("mod_sub", curve, a, b)
    def mod_mul(self, curve, a, b): return self._bin("mod_mul", curve, a, b)
    def mgry_mul(self, curve, a, b): return self._bin("mgry_mul", curve, a, b)
    def mgry_sqr(self, curve, a): return self._un("mgry_sqr", curve, a)
    def mgry_reduce(self, curve, a8): return self._un("mgry_reduce", curve, a8, 8)
    def mgry_from_classical(self, curve, a): return self._un("mgry_from_classical", curve, a)
    def mgry_to_classical(self, curve, a): return self._un("mgry_to_classical", curve, a)
    def gfp_inverse(self, curve, a): return self._un("gfp_inverse", curve, a)
    def gfp_opposite(self, curve, a): return self._un("gfp_opposite", curve, a)

    def mod_shift_left(self, curve, a, count):
        n = a.shape[0]; out = self.empty(n)
        self._call("mod_shift_left", C.c_int(curve), self._ptr(a), C.c_int(count), self._ptr(out), C.c_size_t(n)); return out

    def mgry_pow(self, curve, a, exponent):
        n = a.shape[0]; out = self.empty(n)
        e = (C.c_uint64 * 4)(*[int(v) for v in np.asarray(exponent, dtype=np.uint64).reshape(4)])
        self._call("mgry_pow", C.c_int(curve), self._ptr(a), e, self._ptr(out), C.c_size_t(n)); return out

    def gfp_sqrt(self, curve, a):
        n = a.shape[0]; out = self.empty(n); ok = self.flags(n)
        self._call("gfp_sqrt", C.c_int(curve), self._ptr(a), self._ptr(out), self._ptr(ok, 0), C.c_size_t(n)); return out, ok

    # ---- points (in-out arguments are updated IN PLACE, like the reference's reference parameters)
    def from_affine(self, curve, x, y):
        n = x.shape[0]; j = [self.empty(n) for _ in range(3)]
        self._call("from_affine", C.c_int(curve), self._ptr(x), self._ptr(y), *[self._ptr(t) for t in j], C.c_size_t(n)); return tuple(j)

    def to_affine(self, curve, j, x_only=False):
        n = j[0].shape[0]; x = self.empty(n); y = None if x_only else self.empty(n)
        self._call("to_affine", C.c_int(curve), *[self._ptr(t) for t in j], self._ptr(x), self._ptr(y), C.c_size_t(n)); return x, y

    def on_curve(self, curve, x, y):
        n = x.shape[0]; ok = self.flags(n)
        self._call("on_curve", C.c_int(curve), self._ptr(x), self._ptr(y), self._ptr(ok, 0), C.c_size_t(n)); return ok

    def compute_y(self, curve, x):
        n = x.shape[0]; y = self.empty(n); ok = self.flags(n)
        self._call("compute_y", C.c_int(curve), self._ptr(x), self._ptr(y), self._ptr(ok, 0), C.c_size_t(n)); return y, ok

    def dblu(self, curve, p):
        n = p[0].shape[0]; r = [self.empty(n) for _ in range(3)]
        self._call("dblu", C.c_int(curve), *[self._ptr(t) for t in p], *[self._ptr(t) for t in r], C.c_size_t(n)); return tuple(r)

    def trplu(self, curve, p):
        n = p[0].shape[0]; r = [self.empty(n) for _ in range(3)]
        self._call("trplu", C.c_int(curve), *[self._ptr(t) for t in p], *[self._ptr(t) for t in r], C.c_size_t(n)); return tuple(r)

    def zaddu(self, curve, p, o):
        n = p[0].shape[0]; r = [self.empty(n) for _ in range(3)]
        self._call("zaddu", C.c_int(curve), *[self._ptr(t) for t in p], *[self._ptr(t) for t in o], *[self._ptr(t) for t in r], C.c_size_t(n)); return tuple(r)

    def zdau(self, curve, p, q):
        n = p[0].shape[0]; r = [self.empty(n) for _ in range(3)]
        self._call("zdau", C.c_int(curve), *[self._ptr(t) for t in p], *[self._ptr(t) for t in q], *[self._ptr(t) for t in r], C.c_size_t(n)); return tuple(r)

    def zdau_repeat(self, curve, p, qxy, iters, swap_bits=0, radix=29):
        """ecsimd_hip_zdau_repeat: ZDAU `iters` times in registers; returns (rx, ry, sx, sy, z) = the final P, the final Q, their Z."""
        n = p[0].shape[0]; r = [self.empty(n) for _ in range(5)]
        self._call("zdau_repeat", C.c_int(curve), *[self._ptr(t) for t in p], *[self._ptr(t) for t in qxy], *[self._ptr(t) for t in r], C.c_size_t(n),
                   C.c_int(iters), C.c_uint64(swap_bits), C.c_int(radix)); return tuple(r)

    def add_mixed_complete(self, curve, a, bxy):
        n = a[0].shape[0]; r = [self.empty(n) for _ in range(3)]
        self._call("add_mixed_complete", C.c_int(curve), *[self._ptr(t) for t in a], *[self._ptr(t) for t in bxy], *[self._ptr(t) for t in r], C.c_size_t(n)); return tuple(r)

    def add_z2_1(self, curve, a, bxy):
        n = a[0].shape[0]; r = [self.empty(n) for _ in range(3)]
        self._call("add_z2_1", C.c_int(curve), *[self._ptr(t) for t in a], *[self._ptr(t) for t in bxy], *[self._ptr(t) for t in r], C.c_size_t(n)); return tuple(r)

    def scalar_mult(self, curve, k, x, y, flags=0, out=None, x_only=False):
        """x_only (with OUT_AFFINE): no y output -- returns (x, None); ECDH's shared secret is x of k*Q."""
        n = k.shape[0]
        r = out if out is not None else self._fresh_out(n, flags, x_only)
        self._call("scalar_mult", C.c_int(curve), self._ptr(k), self._ptr(x), self._ptr(y), *[self._ptr(t) for t in r], C.c_size_t(n), C.c_int(flags))
        return tuple(r[:2]) if flags & 2 else tuple(r)

    def _fresh_out(self, n, flags, x_only):
        if x_only:
            if not flags & 2:
                raise ValueError("x_only needs OUT_AFFINE")
            return [self.empty(n), None, None]
        return [self.empty(n) for _ in range(3)]

    def scalar_mult_1s(self, curve, k1, x, y, flags=0, x_only=False):
        n = x.shape[0]; r = self._fresh_out(n, flags, x_only)
        e = (C.c_uint64 * 4)(*[int(v) for v in np.asarray(k1, dtype=np.uint64).reshape(4)])
        self._call("scalar_mult_1s", C.c_int(curve), e, self._ptr(x), self._ptr(y), *[self._ptr(t) for t in r], C.c_size_t(n), C.c_int(flags))
        return tuple(r[:2]) if flags & 2 else tuple(r)

    def scalar_mult_host(self, curve, k, x=None, y=None, flags=0, x_only=False, out=None):
        """ecsimd_hip_scalar_mult_host: numpy uint64 (n, 4) arrays in HOST memory in and out (x = y = None: the generator); chunked, copies overlapped with ladders."""
        k = np.ascontiguousarray(k, dtype=np.uint64); n = k.shape[0]
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else C.c_void_p(0)
        if x is None:
            from .flags import BASE_GENERATOR
            flags |= BASE_GENERATOR
        else:
            x = np.ascontiguousarray(x, dtype=np.uint64); y = np.ascontiguousarray(y, dtype=np.uint64)
            assert x.shape == y.shape == k.shape
        outs = (list(out) if out is not None else [np.empty_like(k) for _ in range(1 if (flags & 2 and x_only) else 2 if flags & 2 else 3)]) + [None, None]     # (out: arrays to reuse -- fresh ones are first touched inside the call)
        self._bind_stream()
        self._check(self.lib.ecsimd_hip_scalar_mult_host(self.ctx, C.c_int(curve), ptr(k), ptr(x), ptr(y), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), C.c_size_t(n), C.c_int(flags)), "scalar_mult_host")
        return tuple(o for o in outs if o is not None)

    def scalar_mult_base(self, curve, k, flags=0, out=None, x_only=False):
        n = k.shape[0]
        r = out if out is not None else self._fresh_out(n, flags, x_only)
        self._call("scalar_mult_base", C.c_int(curve), self._ptr(k), *[self._ptr(t) for t in r], C.c_size_t(n), C.c_int(flags))
        return tuple(r[:2]) if flags & 2 else tuple(r)

    def affine_add(self, curve, a, b):
        n = a[0].shape[0]; rx, ry, fin = self.empty(n), self.empty(n), self.flags(n)
        self._call("affine_add", C.c_int(curve), self._ptr(a[0]), self._ptr(a[1]), self._ptr(b[0]), self._ptr(b[1]), self._ptr(rx), self._ptr(ry), self._ptr(fin, 0), C.c_size_t(n))
        return rx, ry, fin

    def double_scalar_mult(self, curve, u1, u2, qx, qy, x_only=False):
        n = u1.shape[0]; rx, fin = self.empty(n), self.flags(n); ry = None if x_only else self.empty(n)
        self._call("double_scalar_mult", C.c_int(curve), self._ptr(u1), self._ptr(u2), self._ptr(qx), self._ptr(qy), self._ptr(rx), self._ptr(ry), self._ptr(fin, 0), C.c_size_t(n))
        return rx, ry, fin

    def ecdsa_verify_rx(self, curve, u1, u2, qx, qy, r):
        n = u1.shape[0]; ok = self.flags(n)
        self._call("ecdsa_verify_rx", C.c_int(curve), self._ptr(u1), self._ptr(u2), self._ptr(qx), self._ptr(qy), self._ptr(r), self._ptr(ok, 0), C.c_size_t(n))
        return ok

    def ecdsa_verify(self, curve, e, r, s, qx, qy):
        """ecsimd_hip_ecdsa_verify: the whole verification, u1 = e/s and u2 = r/s modulo the group order computed on the device."""
        n = e.shape[0]; ok = self.flags(n)
        self._call("ecdsa_verify", C.c_int(curve), self._ptr(e), self._ptr(r), self._ptr(s), self._ptr(qx), self._ptr(qy), self._ptr(ok, 0), C.c_size_t(n))
        return ok

    def ecdsa_sign(self, curve, e, d, k):
        """ecsimd_hip_ecdsa_sign: (r, s, ok) for digests e, private keys d and caller-supplied nonces k."""
        n = e.shape[0]; r, s, ok = self.empty(n), self.empty(n), self.flags(n)
        self._call("ecdsa_sign", C.c_int(curve), self._ptr(e), self._ptr(d), self._ptr(k), self._ptr(r), self._ptr(s), self._ptr(ok, 0), C.c_size_t(n))
        return r, s, ok

    def ecdsa_recover(self, curve, e, r, s, v, x_only=False):
        """ecsimd_hip_ecdsa_recover: (qx, qy, ok), the public key behind each signature (r, s) of the digest e with recovery id v (uint8 tensor)."""
        n = e.shape[0]; qx, ok = self.empty(n), self.flags(n); qy = None if x_only else self.empty(n)
        self._call("ecdsa_recover", C.c_int(curve), self._ptr(e), self._ptr(r), self._ptr(s), self._ptr(v, 0), self._ptr(qx), self._ptr(qy), self._ptr(ok, 0), C.c_size_t(n))
        return qx, qy, ok

    def ecdsa_sign_recoverable(self, curve, e, d, k, low_s=False):
        """ecsimd_hip_ecdsa_sign_recoverable: (r, s, v, ok); v = parity(y(k G)) | (x(k G) >= n ? 2 : 0); low_s: s > n / 2 is returned as n - s, bit 0 of v flipped."""
        n = e.shape[0]; r, s, v, ok = self.empty(n), self.empty(n), self.flags(n), self.flags(n)
        self._call("ecdsa_sign_recoverable", C.c_int(curve), self._ptr(e), self._ptr(d), self._ptr(k), self._ptr(r), self._ptr(s), self._ptr(v, 0), self._ptr(ok, 0), C.c_size_t(n),
                   C.c_int(ECDSA_LOW_S if low_s else 0))
        return r, s, v, ok

    def sha256(self, msgs, lens=None):
        """ecsimd_hip_sha256: the digests of the rows of `msgs` (2-D uint8 device tensor, one message per row; rows may be strided, e.g. a column slice of a
        wider record array) as (n, 4) integers, ready to be the `e` of the ECDSA calls.  lens (optional, as keccak256's): lane i hashes the first lens[i] bytes
        of its row (ecsimd_hip_sha256_lens)."""
        if lens is not None:
            return self._digest_lens("sha256_lens", msgs, lens, None)
        torch = self.torch
        assert msgs.is_cuda and msgs.device.index == self.device, "tensor on the wrong device"
        assert msgs.dtype == torch.uint8 and msgs.dim() == 2, (msgs.dtype, msgs.shape)
        n, length = int(msgs.shape[0]), int(msgs.shape[1])
        if n > 1 and length > 0 and (msgs.stride(1) != 1 or msgs.stride(0) < length):
            msgs = msgs.contiguous()
        stride = int(msgs.stride(0)) if n > 1 and length > 0 else length
        e = self.empty(n)
        self._bind_stream()
        self._check(self.lib.ecsimd_hip_sha256(self.ctx, C.c_void_p(msgs.data_ptr() if n and length else 0), C.c_size_t(length), C.c_size_t(stride), C.c_void_p(e.data_ptr()), C.c_size_t(n)), "sha256")
        return e

    def rfc6979_nonce(self, curve, e, d):
        """ecsimd_hip_rfc6979_nonce: (k, ok), the RFC 6979 (HMAC-SHA-256) nonce of each digest e and private key d; ok = 0 and k = 0 where d is not in [1, n - 1]."""
        n = e.shape[0]; k, ok = self.empty(n), self.flags(n)
        self._call("rfc6979_nonce", C.c_int(curve), self._ptr(e), self._ptr(d), self._ptr(k), self._ptr(ok, 0), C.c_size_t(n))
        return k, ok

    def ecdsa_sign_deterministic(self, curve, e, d, low_s=False, want_v=True):
        """ecsimd_hip_ecdsa_sign_deterministic: (r, s, v, ok) with the RFC 6979 nonce of (e, d), made and wiped on the device; want_v=False passes v = NULL (v is None)."""
        n = e.shape[0]; r, s, ok = self.empty(n), self.empty(n), self.flags(n); v = self.flags(n) if want_v else None
        self._call("ecdsa_sign_deterministic", C.c_int(curve), self._ptr(e), self._ptr(d), self._ptr(r), self._ptr(s), self._ptr(v, 0), self._ptr(ok, 0), C.c_size_t(n),
                   C.c_int(ECDSA_LOW_S if low_s else 0))
        return r, s, v, ok

    def _messages(self, msgs, n):
        """(pointer, length, stride) of a 2-D uint8 device tensor with one message per row (rows may be strided), as ecsimd_hip_sha256 and the Schnorr calls take it."""
        torch = self.torch
        assert msgs.is_cuda and msgs.device.index == self.device, "tensor on the wrong device"
        assert msgs.dtype == torch.uint8 and msgs.dim() == 2, (msgs.dtype, msgs.shape)
        if int(msgs.shape[0]) != n:
            raise EcsimdHipError(f"operands disagree on the batch length: {sorted((n, int(msgs.shape[0])))}")
        length = int(msgs.shape[1])
        if n > 1 and length > 0 and (msgs.stride(1) != 1 or msgs.stride(0) < length):
            msgs = msgs.contiguous()
        stride = int(msgs.stride(0)) if n > 1 and length > 0 else length
        return msgs, C.c_void_p(msgs.data_ptr() if n and length else 0), C.c_size_t(length), C.c_size_t(stride)

    def schnorr_verify(self, px, msgs, r, s):
        """ecsimd_hip_schnorr_verify: ok, one byte per lane, for BIP-340 signatures (r, s) of the rows of `msgs` (2-D uint8 device tensor, rows may be strided)
        under the x-only public keys px.  secp256k1; public data only."""
        n = px.shape[0]; ok = self.flags(n)
        keep, mp, length, stride = self._messages(msgs, n)
        self._call("schnorr_verify", self._ptr(px), mp, length, stride, self._ptr(r), self._ptr(s), self._ptr(ok, 0), C.c_size_t(n))
        return ok

    def schnorr_sign(self, d, msgs, aux=None, want_px=True):
        """ecsimd_hip_schnorr_sign: (px, r, s, ok), BIP-340 default signing of the rows of `msgs` with the SECRET keys d and the auxiliary randomness aux ((n, 4)
        integers; None = 32 zero bytes); px = the x-only public keys (None with want_px=False).  ok = 0 and zeros where d is not in [1, n - 1]."""
        n = d.shape[0]; r, s, ok = self.empty(n), self.empty(n), self.flags(n); px = self.empty(n) if want_px else None
        keep, mp, length, stride = self._messages(msgs, n)
        self._call("schnorr_sign", self._ptr(d), mp, length, stride, self._ptr(aux), self._ptr(px), self._ptr(r), self._ptr(s), self._ptr(ok, 0), C.c_size_t(n))
        return px, r, s, ok

    def keccak256(self, msgs, lens=None):
        """ecsimd_hip_keccak256: Keccak-256 (Ethereum's: pad byte 0x01, not SHA-3) of the rows of `msgs` (2-D uint8 device tensor, rows may be strided) as (n, 4)
        integers, ready to be the `e` of the ECDSA calls.  lens (optional int32 / uint32 device tensor of n lengths, each <= the row length): lane i hashes the
        first lens[i] bytes of its row."""
        n = int(msgs.shape[0]); e = self.empty(n)
        keep, mp, length, stride = self._messages(msgs, n)
        self._call("keccak256", mp, length, stride, self._lens_ptr("keccak256", lens, n), self._ptr(e), C.c_size_t(n))
        return e

    # ---- Ed25519 (include/ecsimd_ed25519.h): keys and signatures are bytes
    def _rows_u8(self, t, width, what):
        """The pointer and the row count of a contiguous (n, width) uint8 device tensor (a view at any byte offset will do)."""
        assert t.is_cuda and t.device.index == self.device, "tensor on the wrong device"
        assert t.dtype == self.torch.uint8 and t.dim() == 2 and int(t.shape[1]) == width and t.is_contiguous(), (what, t.dtype, tuple(t.shape))
        return C.c_void_p(t.data_ptr() if t.shape[0] else 0), int(t.shape[0])

    def ed25519_pubkey(self, seeds):
        """ecsimd_ed25519_pubkey: (n, 32) uint8 public keys of the (n, 32) uint8 SECRET seeds (RFC 8032 5.1.5)."""
        sp, n = self._rows_u8(seeds, 32, "seeds")
        pk = self.torch.empty((n, 32), dtype=self.torch.uint8, device=self.tdev)
        self._bind_stream()
        self._check(self.lib.ecsimd_ed25519_pubkey(self.ctx, sp, C.c_void_p(pk.data_ptr()), C.c_size_t(n)), "ed25519_pubkey")
        return pk

    def ed25519_sign(self, seeds, msgs, lens=None, want_pk=True):
        """ecsimd_ed25519_sign: (sig, pk), the (n, 64) uint8 signatures R || s of the rows of `msgs` (as keccak256's: 2-D uint8, rows may be strided; lens: lane i
        signs the first lens[i] bytes of its row) under the SECRET seeds, and the public keys derived from them (None with want_pk=False)."""
        sp, n = self._rows_u8(seeds, 32, "seeds")
        keep, mp, length, stride = self._messages(msgs, n)
        sig = self.torch.empty((n, 64), dtype=self.torch.uint8, device=self.tdev)
        pk = self.torch.empty((n, 32), dtype=self.torch.uint8, device=self.tdev) if want_pk else None
        lp = self._lens_ptr("ed25519_sign", lens if length.value else None, n)
        self._bind_stream()
        self._check(self.lib.ecsimd_ed25519_sign(self.ctx, sp, mp, length, stride, lp, C.c_void_p(sig.data_ptr()), C.c_void_p(pk.data_ptr() if want_pk else 0), C.c_size_t(n)), "ed25519_sign")
        return sig, pk

    def ed25519_verify(self, pk, msgs, sig, lens=None, reject_small_order=False):
        """ecsimd_ed25519_verify: ok, one byte per lane: s < L, A decodes strictly, and the canonical encoding of [s]B - [k]A is the signature's R (cofactorless);
        reject_small_order also refuses the eight small-order encodings as A or R.  Public data only."""
        pp, n = self._rows_u8(pk, 32, "pk")
        gp, n2 = self._rows_u8(sig, 64, "sig")
        if n2 != n:
            raise EcsimdHipError(f"ed25519_verify: operands disagree on the batch length: {sorted((n, n2))}")
        keep, mp, length, stride = self._messages(msgs, n)
        ok = self.flags(n)
        lp = self._lens_ptr("ed25519_verify", lens if length.value else None, n)
        self._bind_stream()
        self._check(self.lib.ecsimd_ed25519_verify(self.ctx, pp, mp, length, stride, lp, gp, C.c_void_p(ok.data_ptr()), C.c_size_t(n),
                                                   C.c_int(ED25519_REJECT_SMALL_ORDER if reject_small_order else 0)), "ed25519_verify")
        return ok

    def ed25519_raw(self, op, records):
        """ecsimd_ed25519_raw: one function of the layers below on (n, 32 * inputs) uint8 records; returns (n, 32 * outputs) uint8 (see the header's table)."""
        ni, no = int(self.lib.ecsimd_ed25519_raw_inputs(C.c_int(op))), int(self.lib.ecsimd_ed25519_raw_outputs(C.c_int(op)))
        if ni == 0:
            raise EcsimdHipError(f"ed25519_raw: unknown function {op}")
        ip, n = self._rows_u8(records, 32 * ni, "records")
        out = self.torch.empty((n, 32 * no), dtype=self.torch.uint8, device=self.tdev)
        self._bind_stream()
        self._check(self.lib.ecsimd_ed25519_raw(self.ctx, C.c_int(op), ip, C.c_void_p(out.data_ptr()), C.c_size_t(n)), "ed25519_raw")
        return out

    # ---- X25519 (include/ecsimd_x25519.h): scalars, u-coordinates and shared secrets are 32-byte little-endian records
    def _u8_out(self, n, width=32):
        return self.torch.empty((n, width), dtype=self.torch.uint8, device=self.tdev)

    def x25519(self, scalars, us, want_ok=False):
        """ecsimd_x25519: the (n, 32) uint8 shared secrets X25519(scalar, u) of the SECRET (n, 32) uint8 scalars and the peers' (n, 32) uint8 u (RFC 7748
        section 5: clamped scalar, bit 255 of u ignored, zeros at infinity).  want_ok: (out, ok), ok one byte per lane, 0 where the output is all zero."""
        sp, n = self._rows_u8(scalars, 32, "scalars")
        up, n2 = self._rows_u8(us, 32, "us")
        if n2 != n:
            raise EcsimdHipError(f"x25519: operands disagree on the batch length: {sorted((n, n2))}")
        out = self._u8_out(n)
        ok = self.flags(n) if want_ok else None
        self._bind_stream()
        self._check(self.lib.ecsimd_x25519(self.ctx, sp, up, C.c_void_p(out.data_ptr()), C.c_void_p(ok.data_ptr() if want_ok else 0), C.c_size_t(n)), "x25519")
        return (out, ok) if want_ok else out

    def x25519_base(self, scalars):
        """ecsimd_x25519_base: the (n, 32) uint8 public keys X25519(scalar, 9) of the SECRET (n, 32) uint8 private keys."""
        sp, n = self._rows_u8(scalars, 32, "scalars")
        out = self._u8_out(n)
        self._bind_stream()
        self._check(self.lib.ecsimd_x25519_base(self.ctx, sp, C.c_void_p(out.data_ptr()), C.c_size_t(n)), "x25519_base")
        return out

    def x25519_from_ed25519_pk(self, pk):
        """ecsimd_x25519_from_ed25519_pk: (u, ok), the X25519 public keys of (n, 32) uint8 Ed25519 public keys; ok is 0 (and u zero) where a key does not
        decode strictly or is a small-order encoding.  Public data only; no prime-subgroup check."""
        pp, n = self._rows_u8(pk, 32, "pk")
        u, ok = self._u8_out(n), self.flags(n)
        self._bind_stream()
        self._check(self.lib.ecsimd_x25519_from_ed25519_pk(self.ctx, pp, C.c_void_p(u.data_ptr()), C.c_void_p(ok.data_ptr()), C.c_size_t(n)), "x25519_from_ed25519_pk")
        return u, ok

    def x25519_from_ed25519_seed(self, seeds):
        """ecsimd_x25519_from_ed25519_seed: the (n, 32) uint8 X25519 private keys of the SECRET (n, 32) uint8 Ed25519 seeds (the clamped low half of SHA-512)."""
        sp, n = self._rows_u8(seeds, 32, "seeds")
        out = self._u8_out(n)
        self._bind_stream()
        self._check(self.lib.ecsimd_x25519_from_ed25519_seed(self.ctx, sp, C.c_void_p(out.data_ptr()), C.c_size_t(n)), "x25519_from_ed25519_seed")
        return out

    def x25519_raw(self, op, records):
        """ecsimd_x25519_raw: one function of the layers below on (n, 32 * inputs) uint8 records; returns (n, 32 * outputs) uint8 (see the header's table)."""
        ni, no = int(self.lib.ecsimd_x25519_raw_inputs(C.c_int(op))), int(self.lib.ecsimd_x25519_raw_outputs(C.c_int(op)))
        if ni == 0:
            raise EcsimdHipError(f"x25519_raw: unknown function {op}")
        ip, n = self._rows_u8(records, 32 * ni, "records")
        out = self._u8_out(n, 32 * no)
        self._bind_stream()
        self._check(self.lib.ecsimd_x25519_raw(self.ctx, C.c_int(op), ip, C.c_void_p(out.data_ptr()), C.c_size_t(n)), "x25519_raw")
        return out

    # ---- NIST P-384 (include/ecsimd_p384.h): integers are 48 big-endian bytes, public keys X || Y and signatures r || s 96
    (P384_RAW_FE_MUL, P384_RAW_FE_SQR, P384_RAW_FE_ADD, P384_RAW_FE_SUB, P384_RAW_FE_NEG, P384_RAW_FE_INVERT, P384_RAW_FE_CANON, P384_RAW_SC_MUL, P384_RAW_SC_INVERT,
     P384_RAW_DECODE_ENCODE, P384_RAW_POINT_ADD, P384_RAW_POINT_DBL, P384_RAW_BASE_MULT, P384_RAW_VAR_MULT, P384_RAW_DOUBLE_MULT) = range(15)

    def _p384_rows(self, what, *pairs):
        """The pointers of (tensor, width) pairs and their common row count."""
        ptrs, ns = [], set()
        for t, width in pairs:
            p, n = self._rows_u8(t, width, what)
            ptrs.append(p); ns.add(n)
        if len(ns) != 1:
            raise EcsimdHipError(f"{what}: operands disagree on the batch length: {sorted(ns)}")
        return ptrs, ns.pop()

    def p384_sha384(self, msgs, lens=None):
        """ecsimd_p384_sha384: the (n, 48) uint8 SHA-384 digests of the rows of `msgs` (as keccak256's: 2-D uint8, rows may be strided; lens: lane i hashes the
        first lens[i] bytes of its row)."""
        n = int(msgs.shape[0])
        keep, mp, length, stride = self._messages(msgs, n)
        out = self._u8_out(n, 48)
        lp = self._lens_ptr("p384_sha384", lens if length.value else None, n)
        self._bind_stream()
        self._check(self.lib.ecsimd_p384_sha384(self.ctx, mp, length, stride, lp, C.c_void_p(out.data_ptr() if n else 0), C.c_size_t(n)), "p384_sha384")
        return out

    def p384_pubkey(self, d):
        """ecsimd_p384_pubkey: (pub, ok), the (n, 96) uint8 public keys X || Y of the SECRET (n, 48) uint8 private keys; ok = 0 and zeros where d is not in [1, n - 1]."""
        (dp,), n = self._p384_rows("p384_pubkey", (d, 48))
        pub, ok = self._u8_out(n, 96), self.flags(n)
        self._bind_stream()
        self._check(self.lib.ecsimd_p384_pubkey(self.ctx, dp, C.c_void_p(pub.data_ptr() if n else 0), C.c_void_p(ok.data_ptr() if n else 0), C.c_size_t(n)), "p384_pubkey")
        return pub, ok

    def p384_ecdh(self, d, peer):
        """ecsimd_p384_ecdh: (z, ok), z = x(d peer) as (n, 48) uint8 for the SECRET (n, 48) private keys and the peers' (n, 96) public keys; ok = 0 and zeros
        where d is not in [1, n - 1] or the peer does not decode."""
        (dp, pp), n = self._p384_rows("p384_ecdh", (d, 48), (peer, 96))
        z, ok = self._u8_out(n, 48), self.flags(n)
        self._bind_stream()
        self._check(self.lib.ecsimd_p384_ecdh(self.ctx, dp, pp, C.c_void_p(z.data_ptr() if n else 0), C.c_void_p(ok.data_ptr() if n else 0), C.c_size_t(n)), "p384_ecdh")
        return z, ok

    def p384_ecdsa_verify(self, pub, digest, sig):
        """ecsimd_p384_ecdsa_verify: ok, one byte per lane, for the (n, 96) signatures r || s of the (n, 48) digests under the (n, 96) public keys.  Public data."""
        (pp, gp, sp), n = self._p384_rows("p384_ecdsa_verify", (pub, 96), (digest, 48), (sig, 96))
        ok = self.flags(n)
        self._bind_stream()
        self._check(self.lib.ecsimd_p384_ecdsa_verify(self.ctx, pp, gp, sp, C.c_void_p(ok.data_ptr() if n else 0), C.c_size_t(n)), "p384_ecdsa_verify")
        return ok

    def p384_ecdsa_sign(self, d, digest, flags=0):
        """ecsimd_p384_ecdsa_sign: (sig, ok), the deterministic (RFC 6979, HMAC-SHA-384, one candidate) signatures r || s of the (n, 48) digests under the SECRET
        (n, 48) private keys; ok = 0 and zeros where d is not in [1, n - 1]."""
        (dp, gp), n = self._p384_rows("p384_ecdsa_sign", (d, 48), (digest, 48))
        sig, ok = self._u8_out(n, 96), self.flags(n)
        self._bind_stream()
        self._check(self.lib.ecsimd_p384_ecdsa_sign(self.ctx, dp, gp, C.c_void_p(sig.data_ptr() if n else 0), C.c_void_p(ok.data_ptr() if n else 0), C.c_size_t(n), C.c_int(flags)),
                    "p384_ecdsa_sign")
        return sig, ok

    def p384_raw(self, op, records):
        """ecsimd_p384_raw: one function of the layers below on (n, 48 * inputs) uint8 records; returns (n, 48 * outputs) uint8 (see the header's table)."""
        ni, no = int(self.lib.ecsimd_p384_raw_inputs(C.c_int(op))), int(self.lib.ecsimd_p384_raw_outputs(C.c_int(op)))
        if ni == 0:
            raise EcsimdHipError(f"p384_raw: unknown function {op}")
        ip, n = self._rows_u8(records, 48 * ni, "records")
        out = self._u8_out(n, 48 * no)
        self._bind_stream()
        self._check(self.lib.ecsimd_p384_raw(self.ctx, C.c_int(op), ip, C.c_void_p(out.data_ptr() if n else 0), C.c_size_t(n)), "p384_raw")
        return out

    # ---- BLS12-381 G1 and G2 (include/ecsimd_bls12_381.h, include/ecsimd_bls12_381_g2.h): points are the standard encodings, 96 bytes (48 compressed) in G1,
    # 192 (96 compressed, c1 before c0) in G2.  PUBLIC data only.  The two groups' methods go through ONE set of helpers, which take the C functions' stem
    # ("bls12_381_g1", "bls381_g2": the error texts' too) and the uncompressed width w; the compressed width is w / 2.
    (BLS12_381_RAW_FE_MUL, BLS12_381_RAW_FE_SQR, BLS12_381_RAW_FE_ADD, BLS12_381_RAW_FE_SUB, BLS12_381_RAW_FE_NEG, BLS12_381_RAW_FE_INVERT, BLS12_381_RAW_FE_SQRT,
     BLS12_381_RAW_FE_CANON, BLS12_381_RAW_POINT_ADD, BLS12_381_RAW_POINT_DBL, BLS12_381_RAW_POINT_MADD) = range(11)
    (BLS12_381_G2_RAW_FE2_MUL, BLS12_381_G2_RAW_FE2_SQR, BLS12_381_G2_RAW_FE2_ADD, BLS12_381_G2_RAW_FE2_SUB, BLS12_381_G2_RAW_FE2_NEG, BLS12_381_G2_RAW_FE2_INVERT,
     BLS12_381_G2_RAW_FE2_SQRT, BLS12_381_G2_RAW_FE2_CANON, BLS12_381_G2_RAW_POINT_ADD, BLS12_381_G2_RAW_POINT_DBL, BLS12_381_G2_RAW_POINT_MADD) = range(11)

    def _bls12_381_scalars(self, k, what):
        """The C ABI's scalars -- (n, 4) 64-bit little-endian limbs, 16-byte aligned -- from such a tensor or from (n, 32) uint8 little-endian bytes (copied:
        a byte tensor may lie anywhere)."""
        torch = self.torch
        assert k.is_cuda and k.device.index == self.device, "tensor on the wrong device"
        if k.dtype == torch.uint8:
            assert k.dim() == 2 and int(k.shape[1]) == 32, (what, tuple(k.shape))
            k = k.clone(memory_format=torch.contiguous_format).view(torch.int64)
        assert k.dtype in (torch.int64, torch.uint64) and k.dim() == 2 and int(k.shape[1]) == 4 and k.is_contiguous(), (what, k.dtype, tuple(k.shape))
        return k, C.c_void_p(k.data_ptr() if k.shape[0] else 0), int(k.shape[0])

    def _bls12_381_lanes(self, what, inp, in_width, out_widths):
        ip, n = self._rows_u8(inp, in_width, what)
        outs = [self._u8_out(n, w) if w > 1 else self.flags(n) for w in out_widths]
        self._bind_stream()
        self._check(getattr(self.lib, "ecsimd_" + what)(self.ctx, ip, *[C.c_void_p(o.data_ptr() if n else 0) for o in outs], C.c_size_t(n)), what)
        return tuple(outs)

    def _bls12_381_mul(self, stem, w, k, inp):
        what = stem + "_mul"
        keep, kp, n = self._bls12_381_scalars(k, what)
        ip, n2 = self._rows_u8(inp, w, f"in{w}")
        if n2 != n:
            raise EcsimdHipError(f"{what}: operands disagree on the batch length: {sorted((n, n2))}")
        out, ok = self._u8_out(n, w), self.flags(n)
        self._bind_stream()
        self._check(getattr(self.lib, "ecsimd_" + what)(self.ctx, kp, ip, C.c_void_p(out.data_ptr() if n else 0), C.c_void_p(ok.data_ptr() if n else 0), C.c_size_t(n)), what)
        return out, ok

    @staticmethod
    def _bls12_381_msm_plan(stem, n, bits, alg):
        plan = MsmPlan()
        rc = getattr(load_library(), f"ecsimd_{stem}_msm_plan")(C.c_size_t(n), C.c_int(bits), C.c_int(alg), C.byref(plan))
        if rc != 0:
            raise EcsimdHipError(f"{stem}_msm_plan(n={n}, bits={bits}, alg={alg}) failed ({rc}): bits must be 1 .. 256, n at most 2^24, alg 0, 1 or 2")
        return {name: int(getattr(plan, name)) for name, _ in MsmPlan._fields_}

    def _bls12_381_sum(self, what, w, want_invalid, n, *inputs, tail=()):
        """One of the calls with a single result: (out, finite[, invalid]) with out the (w,) uint8 encoding."""
        torch = self.torch
        out = torch.zeros((w,), dtype=torch.uint8, device=self.tdev)
        finite = torch.zeros((1,), dtype=torch.uint8, device=self.tdev)
        invalid = torch.zeros((1,), dtype=torch.int32, device=self.tdev) if want_invalid else None
        self._bind_stream()
        self._check(getattr(self.lib, "ecsimd_" + what)(self.ctx, *inputs, C.c_void_p(out.data_ptr()), C.c_void_p(finite.data_ptr()), C.c_void_p(invalid.data_ptr() if want_invalid else 0),
                                                        C.c_size_t(n), *tail), what)
        return (out, finite, invalid) if want_invalid else (out, finite)

    def _bls12_381_msm(self, stem, w, k, pts, bits, alg, want_invalid):
        what = stem + "_msm"
        keep, kp, n = self._bls12_381_scalars(k, what)
        pp, n2 = self._rows_u8(pts, w, f"pts{w}")
        if n2 != n:
            raise EcsimdHipError(f"{what}: operands disagree on the batch length: {sorted((n, n2))}")
        return self._bls12_381_sum(what, w, want_invalid, n, kp, pp, tail=(C.c_int(bits), C.c_int(alg)))

    def _bls12_381_point_sum(self, stem, w, pts, want_invalid):
        assert pts.dim() == 2 and int(pts.shape[1]) in (w // 2, w), tuple(pts.shape)
        width = int(pts.shape[1])
        pp, n = self._rows_u8(pts, width, "pts")
        return self._bls12_381_sum(stem + "_point_sum", w, want_invalid, n, pp, tail=(C.c_int(1 if width == w // 2 else 0),))

    def _bls12_381_raw(self, what, op, records):
        ni, no = int(getattr(self.lib, f"ecsimd_{what}_inputs")(C.c_int(op))), int(getattr(self.lib, f"ecsimd_{what}_outputs")(C.c_int(op)))
        if ni == 0:
            raise EcsimdHipError(f"{what}: unknown function {op}")
        ip, n = self._rows_u8(records, 48 * ni, "records")
        out = self._u8_out(n, 48 * no)
        self._bind_stream()
        self._check(getattr(self.lib, "ecsimd_" + what)(self.ctx, C.c_int(op), ip, C.c_void_p(out.data_ptr() if n else 0), C.c_size_t(n)), what)
        return out

    def bls12_381_g1_decompress(self, in48):
        """ecsimd_bls12_381_g1_decompress: (out96, ok) for (n, 48) uint8 compressed points; a malformed lane gets zeros and ok = 0.  On-curve only."""
        return self._bls12_381_lanes("bls12_381_g1_decompress", in48, 48, (96, 1))

    def bls12_381_g1_compress(self, in96):
        """ecsimd_bls12_381_g1_compress: (out48, ok) for (n, 96) uint8 uncompressed points, validated the same way."""
        return self._bls12_381_lanes("bls12_381_g1_compress", in96, 96, (48, 1))

    def bls12_381_g1_check(self, in96):
        """ecsimd_bls12_381_g1_check: (on_curve, in_subgroup), one byte per lane each; in_subgroup is [r] P = infinity."""
        return self._bls12_381_lanes("bls12_381_g1_check", in96, 96, (1, 1))

    def bls12_381_g1_mul(self, k, in96):
        """ecsimd_bls12_381_g1_mul: (out96, ok), k[i] P[i] for the 256-bit INTEGERS k ((n, 4) limbs or (n, 32) uint8 little-endian) and the validated points."""
        return self._bls12_381_mul("bls12_381_g1", 96, k, in96)

    @staticmethod
    def bls12_381_g1_msm_plan(n, bits=255, alg=0):
        """ecsimd_bls12_381_g1_msm_plan: msm_plan's dict for bls12_381_g1_msm (the same bucket schedule, this group's workspace_bytes and LANES route).  Host only."""
        return Engine._bls12_381_msm_plan("bls12_381_g1", n, bits, alg)

    def bls12_381_g1_msm(self, k, pts96, bits=255, alg=0, want_invalid=False):
        """ecsimd_bls12_381_g1_msm: (out96, finite) = the (96,) uint8 encoding of the sum of (k[i] mod 2^bits) P[i] and a (1,) uint8 flag (0 and the infinity
        encoding for the identity).  k as bls12_381_g1_mul's; pts96: (n, 96) uint8.  A malformed point contributes nothing; want_invalid: a third tensor, the
        (1,) int32 number of them.  Points are NOT tested for subgroup membership.  Capturable after one warm-up call at the same (n, bits, alg)."""
        return self._bls12_381_msm("bls12_381_g1", 96, k, pts96, bits, alg, want_invalid)

    def bls12_381_g1_point_sum(self, pts, want_invalid=False):
        """ecsimd_bls12_381_g1_point_sum: (out96, finite) = the sum of the points; pts is (n, 96) uint8 uncompressed or (n, 48) uint8 compressed (the width
        decides).  Malformed points are skipped and counted (want_invalid)."""
        return self._bls12_381_point_sum("bls12_381_g1", 96, pts, want_invalid)

    def bls12_381_raw(self, op, records):
        """ecsimd_bls12_381_raw: one function of the layers below on (n, 48 * inputs) uint8 records; returns (n, 48 * outputs) uint8 (see the header's table)."""
        return self._bls12_381_raw("bls12_381_raw", op, records)

    def bls12_381_g2_decompress(self, in96):
        """ecsimd_bls381_g2_decompress: (out192, ok) for (n, 96) uint8 compressed points; a malformed lane gets zeros and ok = 0.  On-curve only."""
        return self._bls12_381_lanes("bls381_g2_decompress", in96, 96, (192, 1))

    def bls12_381_g2_compress(self, in192):
        """ecsimd_bls381_g2_compress: (out96, ok) for (n, 192) uint8 uncompressed points, validated the same way."""
        return self._bls12_381_lanes("bls381_g2_compress", in192, 192, (96, 1))

    def bls12_381_g2_check(self, in192):
        """ecsimd_bls381_g2_check: (on_curve, in_subgroup), one byte per lane each; in_subgroup is [r] Q = infinity."""
        return self._bls12_381_lanes("bls381_g2_check", in192, 192, (1, 1))

    def bls12_381_g2_mul(self, k, in192):
        """ecsimd_bls381_g2_mul: (out192, ok), k[i] Q[i] for the 256-bit INTEGERS k ((n, 4) limbs or (n, 32) uint8 little-endian) and the validated points."""
        return self._bls12_381_mul("bls381_g2", 192, k, in192)

    @staticmethod
    def bls12_381_g2_msm_plan(n, bits=255, alg=0):
        """ecsimd_bls381_g2_msm_plan: msm_plan's dict for bls12_381_g2_msm (the same bucket schedule, this group's workspace_bytes and LANES route).  Host only."""
        return Engine._bls12_381_msm_plan("bls381_g2", n, bits, alg)

    def bls12_381_g2_msm(self, k, pts192, bits=255, alg=0, want_invalid=False):
        """ecsimd_bls381_g2_msm: (out192, finite) = the (192,) uint8 encoding of the sum of (k[i] mod 2^bits) Q[i] and a (1,) uint8 flag (0 and the infinity
        encoding for the identity).  k as bls12_381_g2_mul's; pts192: (n, 192) uint8.  A malformed point contributes nothing; want_invalid: a third tensor, the
        (1,) int32 number of them.  Points are NOT tested for subgroup membership.  Capturable after one warm-up call at the same (n, bits, alg)."""
        return self._bls12_381_msm("bls381_g2", 192, k, pts192, bits, alg, want_invalid)

    def bls12_381_g2_point_sum(self, pts, want_invalid=False):
        """ecsimd_bls381_g2_point_sum: (out192, finite) = the sum of the points; pts is (n, 192) uint8 uncompressed or (n, 96) uint8 compressed (the width
        decides).  Malformed points are skipped and counted (want_invalid)."""
        return self._bls12_381_point_sum("bls381_g2", 192, pts, want_invalid)

    def bls12_381_g2_raw(self, op, records):
        """ecsimd_bls381_g2_raw: one function of the layers below on (n, 48 * inputs) uint8 records (an Fp2 operand is two records, c0 then c1); returns
        (n, 48 * outputs) uint8 (see the header's table)."""
        return self._bls12_381_raw("bls381_g2_raw", op, records)

    # ---- the SM2 signature scheme (include/ecsimd_sm2.h): integers are (n, 4) limb tensors as the ECDSA methods take them, digests likewise
    SM2_DEFAULT_ID = b"1234567812345678"

    @staticmethod
    def sm2_curve():
        """ecsimd_sm2_curve: the id of sm2p256v1 (registered on the first call; what curves.curve_id("sm2") returns).  Host only: no GPU and no Engine."""
        cid = C.c_int(-1)
        rc = load_library().ecsimd_sm2_curve(C.byref(cid))
        if rc != 0:
            raise EcsimdHipError(f"sm2_curve failed ({rc})")
        return cid.value

    def _sm2_call(self, name, *args):
        rows, self._rows = self._rows, set()
        if len(rows) > 1:
            raise EcsimdHipError(f"{name}: operands disagree on the batch length: {sorted(rows)}")
        self._bind_stream()
        self._check(getattr(self.lib, "ecsimd_" + name)(self.ctx, *args), name)

    def _sm2_ids(self, ids, n):
        """(keep-alive, pointer, id_bytes, id_stride) of `ids`: bytes (one identity for the whole batch, copied to the device) or a 2-D uint8 device tensor with
        one identity per row."""
        torch = self.torch
        if isinstance(ids, (bytes, bytearray)):
            t = torch.tensor(list(ids), dtype=torch.uint8, device=self.tdev) if len(ids) else None
            return t, C.c_void_p(t.data_ptr() if t is not None else 0), C.c_size_t(len(ids)), C.c_size_t(0)
        keep, ip, length, stride = self._messages(ids, n)
        if n == 1 or length.value == 0:
            stride = C.c_size_t(0)
        return keep, ip, length, stride

    def sm3(self, msgs, lens=None):
        """ecsimd_sm2_sm3: the SM3 digests of the rows of `msgs` (as sha256's: 2-D uint8, rows may be strided; lens: lane i hashes the first lens[i] bytes of its
        row) as (n, 4) integers."""
        n = int(msgs.shape[0]); e = self.empty(n)
        keep, mp, length, stride = self._messages(msgs, n)
        lp = self._lens_ptr("sm2_sm3", lens if length.value else None, n)
        self._sm2_call("sm2_sm3", mp, length, stride, lp, self._ptr(e), C.c_size_t(n))
        return e

    def sm2_za(self, curve, qx, qy, ids=SM2_DEFAULT_ID):
        """ecsimd_sm2_za: Z_A of each public key and identity (bytes: one for the whole batch; a 2-D uint8 tensor: one per row) as (n, 4) integers."""
        n = int(qx.shape[0]); za = self.empty(n)
        keep, ip, ilen, istride = self._sm2_ids(ids, n)
        self._sm2_call("sm2_za", C.c_int(curve), self._ptr(qx), self._ptr(qy), ip, ilen, istride, self._ptr(za), C.c_size_t(n))
        return za

    def sm2_digest(self, curve, qx, qy, msgs, ids=SM2_DEFAULT_ID, lens=None):
        """ecsimd_sm2_digest: e = SM3(Z_A || M) of each lane as (n, 4) integers, ready to be the `e` of sm2_verify_digest and sm2_sign_digest."""
        n = int(qx.shape[0]); e = self.empty(n)
        keep, ip, ilen, istride = self._sm2_ids(ids, n)
        keep2, mp, length, stride = self._messages(msgs, n)
        lp = self._lens_ptr("sm2_digest", lens if length.value else None, n)
        self._sm2_call("sm2_digest", C.c_int(curve), self._ptr(qx), self._ptr(qy), ip, ilen, istride, mp, length, stride, lp, self._ptr(e), C.c_size_t(n))
        return e

    def sm2_pubkey(self, curve, d):
        """ecsimd_sm2_pubkey: (qx, qy, ok) for the SECRET private keys d; ok = 0 and (0, 0) where d is not in [1, n - 2]."""
        n = int(d.shape[0]); qx, qy, ok = self.empty(n), self.empty(n), self.flags(n)
        self._sm2_call("sm2_pubkey", C.c_int(curve), self._ptr(d), self._ptr(qx), self._ptr(qy), self._ptr(ok, 0), C.c_size_t(n))
        return qx, qy, ok

    def sm2_verify_digest(self, curve, e, r, s, qx, qy):
        """ecsimd_sm2_verify_digest: ok, one byte per lane, for the signatures (r, s) of the digests e under the public keys (qx, qy).  Public data."""
        n = int(e.shape[0]); ok = self.flags(n)
        self._sm2_call("sm2_verify_digest", C.c_int(curve), self._ptr(e), self._ptr(r), self._ptr(s), self._ptr(qx), self._ptr(qy), self._ptr(ok, 0), C.c_size_t(n))
        return ok

    def sm2_verify(self, curve, qx, qy, msgs, r, s, ids=SM2_DEFAULT_ID, lens=None):
        """ecsimd_sm2_verify: ok, one byte per lane, for the signatures (r, s) of the rows of `msgs` under the public keys and identities.  Public data."""
        n = int(qx.shape[0]); ok = self.flags(n)
        keep, ip, ilen, istride = self._sm2_ids(ids, n)
        keep2, mp, length, stride = self._messages(msgs, n)
        lp = self._lens_ptr("sm2_verify", lens if length.value else None, n)
        self._sm2_call("sm2_verify", C.c_int(curve), self._ptr(qx), self._ptr(qy), ip, ilen, istride, mp, length, stride, lp, self._ptr(r), self._ptr(s), self._ptr(ok, 0),
                       C.c_size_t(n))
        return ok

    def sm2_sign_digest(self, curve, e, d, k=None, flags=0):
        """ecsimd_sm2_sign_digest: (r, s, ok) for the digests e under the SECRET keys d and nonces k; k=None: the deterministic nonce (RFC 6979's construction
        with HMAC-SHA-256 -- SM2 has no standard one; any verifier accepts the signature), made and wiped on the device."""
        n = int(e.shape[0]); r, s, ok = self.empty(n), self.empty(n), self.flags(n)
        self._sm2_call("sm2_sign_digest", C.c_int(curve), self._ptr(e), self._ptr(d), self._ptr(k), self._ptr(r), self._ptr(s), self._ptr(ok, 0), C.c_size_t(n), C.c_int(flags))
        return r, s, ok

    def sm2_sign(self, curve, d, msgs, ids=SM2_DEFAULT_ID, k=None, lens=None):
        """(r, s, ok, qx, qy): sm2_pubkey, sm2_digest and sm2_sign_digest in a row -- the message-level signature; a lane whose key is refused has ok = 0."""
        qx, qy, key_ok = self.sm2_pubkey(curve, d)
        e = self.sm2_digest(curve, qx, qy, msgs, ids=ids, lens=lens)
        r, s, ok = self.sm2_sign_digest(curve, e, d, k)
        return r, s, ok, qx, qy

    # ---- multi-scalar multiplication (include/ecsimd_msm.h): ONE point out of a batch.  PUBLIC data only.
    MSM_ALG_AUTO, MSM_ALG_BUCKETS, MSM_ALG_LANES = 0, 1, 2

    @staticmethod
    def msm_plan(n, bits=256, alg=0):
        """ecsimd_msm_plan: what msm(n terms, bits, alg) will do, as a dict (route, c, windows, buckets, L, m, max_chain, launches, workspace_bytes).
        Host only: needs the library, no GPU and no Engine."""
        plan = MsmPlan()
        lib = load_library()
        rc = lib.ecsimd_msm_plan(C.c_size_t(n), C.c_int(bits), C.c_int(alg), C.byref(plan))
        if rc != 0:
            raise EcsimdHipError(f"msm_plan(n={n}, bits={bits}, alg={alg}) failed ({rc}): bits must be 1 .. 256, n at most 2^24, alg 0, 1 or 2")
        return {name: int(getattr(plan, name)) for name, _ in MsmPlan._fields_}

    def _msm_out(self, want_invalid):
        torch = self.torch
        rx, ry = self.empty(1), self.empty(1)
        finite = torch.zeros((1,), dtype=torch.uint8, device=self.tdev)
        invalid = torch.zeros((1,), dtype=torch.int32, device=self.tdev) if want_invalid else None
        return rx, ry, finite, invalid

    def msm(self, curve, k, x, y, bits=256, alg=0, want_invalid=False):
        """ecsimd_msm: (rx, ry, finite) = the sum of (k[i] mod 2^bits) * (x[i], y[i]) as ONE affine point ((1, 4) tensors, (0, 0) and finite = 0 at infinity).
        Points are validated; an invalid one counts as infinity.  want_invalid: a fourth tensor, the (1,) int32 number of invalid points.  PUBLIC data only.
        Capturable after one warm-up call at the same (n, bits, alg): see CAPTURE in the header."""
        n = int(k.shape[0])
        if int(x.shape[0]) != n or int(y.shape[0]) != n:
            raise EcsimdHipError(f"msm: operands disagree on the batch length: {sorted({n, int(x.shape[0]), int(y.shape[0])})}")
        rx, ry, finite, invalid = self._msm_out(want_invalid)
        kp, xp, yp = self._ptr(k), self._ptr(x), self._ptr(y)
        self._rows.clear()
        self._bind_stream()
        self._check(self.lib.ecsimd_msm(self.ctx, C.c_int(curve), kp, xp, yp, C.c_void_p(rx.data_ptr()), C.c_void_p(ry.data_ptr()), C.c_void_p(finite.data_ptr()),
                                        C.c_void_p(invalid.data_ptr() if want_invalid else 0), C.c_size_t(n), C.c_int(bits), C.c_int(alg)), "msm")
        return (rx, ry, finite, invalid) if want_invalid else (rx, ry, finite)

    def point_sum(self, curve, x, y, want_invalid=False):
        """ecsimd_msm_point_sum: (rx, ry, finite) = the sum of the points (x[i], y[i]) as ONE affine point; validation and want_invalid as for msm."""
        n = int(x.shape[0])
        if int(y.shape[0]) != n:
            raise EcsimdHipError(f"point_sum: operands disagree on the batch length: {sorted({n, int(y.shape[0])})}")
        rx, ry, finite, invalid = self._msm_out(want_invalid)
        xp, yp = self._ptr(x), self._ptr(y)
        self._rows.clear()
        self._bind_stream()
        self._check(self.lib.ecsimd_msm_point_sum(self.ctx, C.c_int(curve), xp, yp, C.c_void_p(rx.data_ptr()), C.c_void_p(ry.data_ptr()), C.c_void_p(finite.data_ptr()),
                                                  C.c_void_p(invalid.data_ptr() if want_invalid else 0), C.c_size_t(n)), "point_sum")
        return (rx, ry, finite, invalid) if want_invalid else (rx, ry, finite)

    # ---- number-theoretic transform (include/ecsimd_ntt.h) over a registered prime field: PUBLIC OR SECRET-INDEPENDENT (a data-independent schedule)
    @staticmethod
    def ntt_max_radix_log(r):
        """ECSIMD_NTT_MAX_RADIX_LOG(r): the `flags` that cap every pass at r butterfly stages (a test hook: same values, more passes)."""
        return r & 15

    @staticmethod
    def ntt_field_info(field):
        """ecsimd_ntt_field_info: (two_adicity, default root as an int) of a prime field id.  Host only."""
        s, root = C.c_int(0), (C.c_uint64 * 4)()
        rc = load_library().ecsimd_ntt_field_info(C.c_int(field), C.byref(s), root)
        if rc != 0:
            raise EcsimdHipError(f"ntt_field_info(field={field}) failed ({rc}): the field must be a modulus registered as prime")
        return s.value, _from_limbs(root)

    @staticmethod
    def ntt_bls12_381_fr():
        """ecsimd_ntt_bls12_381_fr: (field id of Fr, the conventional root 7^((r - 1) / 2^32) as an int).  Host only."""
        fid, root = C.c_int(-1), (C.c_uint64 * 4)()
        rc = load_library().ecsimd_ntt_bls12_381_fr(C.byref(fid), root)
        if rc != 0:
            raise EcsimdHipError(f"ntt_bls12_381_fr failed ({rc})")
        return fid.value, _from_limbs(root)

    @staticmethod
    def ntt_plan(log_n, batch=1, flags=0):
        """ecsimd_ntt_plan as a dict (passes, log_radix: 24 entries, lanes, lds_bytes, launches, workspace_bytes).  Host only."""
        plan = NttPlan()
        rc = load_library().ecsimd_ntt_plan(C.c_int(log_n), C.c_size_t(batch), C.c_int(flags), C.byref(plan))
        if rc != 0:
            raise EcsimdHipError(f"ntt_plan(log_n={log_n}, batch={batch}, flags={flags}) failed ({rc}): log_n must be 1 .. 24, batch at least 1, flags 0 or a radix cap 1 .. 9")
        return {name: (list(plan.log_radix) if name == "log_radix" else int(getattr(plan, name))) for name, _ in NttPlan._fields_}

    def ntt_domain(self, field, log_n, root=None, shift=None):
        """ecsimd_ntt_domain_create: the domain {shift * w^k} of size 2^log_n, w = root^(2^(s - log_n)); root None = the field's default root, shift None = 1."""
        handle = C.c_void_p()
        self._bind_stream()
        self._check(self.lib.ecsimd_ntt_domain_create(self.ctx, C.c_int(field), C.c_int(log_n), _limbs(root) if root is not None else None,
                                                      _limbs(shift) if shift is not None else None, C.byref(handle)), "ntt_domain_create")
        return NttDomain(self, handle, field, log_n)

    def _ntt(self, name, dom, x, out, flags):
        rows = int(x.shape[0])
        if rows % dom.n:
            raise EcsimdHipError(f"{name}: {rows} rows are no whole number of arrays of {dom.n}")
        out = self.empty(rows) if out is None else out
        if int(out.shape[0]) != rows:
            raise EcsimdHipError(f"{name}: operands disagree on the batch length: {sorted({rows, int(out.shape[0])})}")
        xp, op = self._ptr(x), self._ptr(out)
        self._rows.clear()
        self._bind_stream()
        self._check(getattr(self.lib, "ecsimd_" + name)(self.ctx, dom.handle, xp, op, C.c_size_t(rows // dom.n), C.c_int(flags)), name)
        return out

    def ntt_forward(self, dom, x, out=None, flags=0):
        """ecsimd_ntt_forward: x is (batch * n, 4), batch arrays one after the other; out[k] = sum_i x[i] (g w^k)^i.  out may be x (in place)."""
        return self._ntt("ntt_forward", dom, x, out, flags)

    def ntt_inverse(self, dom, x, out=None, flags=0):
        """ecsimd_ntt_inverse: the exact inverse of ntt_forward on the same domain."""
        return self._ntt("ntt_inverse", dom, x, out, flags)

    def ntt_bitrev(self, log_n, x, out=None):
        """ecsimd_ntt_bitrev: out[rev(i)] = x[i] in each array of 2^log_n rows; out may be x."""
        rows = int(x.shape[0])
        if rows % (1 << log_n):
            raise EcsimdHipError(f"ntt_bitrev: {rows} rows are no whole number of arrays of {1 << log_n}")
        out = self.empty(rows) if out is None else out
        if int(out.shape[0]) != rows:
            raise EcsimdHipError(f"ntt_bitrev: operands disagree on the batch length: {sorted({rows, int(out.shape[0])})}")
        xp, op = self._ptr(x), self._ptr(out)
        self._rows.clear()
        self._bind_stream()
        self._check(self.lib.ecsimd_ntt_bitrev(self.ctx, C.c_int(log_n), xp, op, C.c_size_t(rows >> log_n)), "ntt_bitrev")
        return out

    def ntt_poly_mul(self, dom, a, b):
        """The product of two polynomials given as dom.n coefficients each (classical): forward both, mod_mul, inverse.  The product's degree must be below dom.n
        -- the caller pads with zeros --, else it comes out reduced modulo x^n - g^n."""
        return self.ntt_inverse(dom, self.mod_mul(dom.field, self.ntt_forward(dom, a), self.ntt_forward(dom, b)))

    # ---- BIP-340 batch verification (include/ecsimd_schnorr_batch.h): ONE verdict out of a batch.  PUBLIC data only.
    @staticmethod
    def schnorr_batch_plan(n, msg_bytes, route=0):
        """ecsimd_schnorr_batch_plan: what schnorr_verify_batch(n signatures, messages of msg_bytes bytes, route) will do, as a dict (route, launches,
        workspace_bytes).  Host only: needs the library, no GPU and no Engine."""
        plan = SchnorrBatchPlan()
        rc = load_library().ecsimd_schnorr_batch_plan(C.c_size_t(n), C.c_size_t(msg_bytes), C.c_int(route), C.byref(plan))
        if rc != 0:
            raise EcsimdHipError(f"schnorr_batch_plan(n={n}, msg_bytes={msg_bytes}, route={route}) failed ({rc}): n at most 2^24 - 1, msg_bytes at most 2^40, route 0, 1 or 2")
        return {name: int(getattr(plan, name)) for name, _ in SchnorrBatchPlan._fields_}

    def _schnorr_batch_args(self, what, px, msgs, r, s):
        n = int(px.shape[0])
        if int(r.shape[0]) != n or int(s.shape[0]) != n:
            raise EcsimdHipError(f"{what}: operands disagree on the batch length: {sorted({n, int(r.shape[0]), int(s.shape[0])})}")
        keep, mp, length, stride = self._messages(msgs, n)
        args = (self._ptr(px), mp, length, stride, self._ptr(r), self._ptr(s))
        self._rows.clear()
        self._bind_stream()
        return n, keep, args

    def schnorr_verify_batch(self, px, msgs, r, s, route=0, out=None):
        """ecsimd_schnorr_verify_batch: a (1,) uint8 tensor, 1 iff EVERY BIP-340 signature (r, s) of the rows of `msgs` under the x-only keys px is valid (a batch
        with an invalid one passes with probability at most 2^-127 on the MSM route); an empty batch gives 1.  route: flags.SCHNORR_BATCH_*.  Which lane is at fault
        is schnorr_verify's to say.  out: a (1,) uint8 device tensor to write instead of a new one.  Capturable after one warm-up call at the same (n, message
        length, route)."""
        n, keep, args = self._schnorr_batch_args("schnorr_verify_batch", px, msgs, r, s)
        ok = self.torch.zeros((1,), dtype=self.torch.uint8, device=self.tdev) if out is None else out
        assert ok.is_cuda and ok.device.index == self.device and ok.dtype == self.torch.uint8 and ok.numel() == 1, "out: one uint8 on the engine's device"
        self._check(self.lib.ecsimd_schnorr_verify_batch(self.ctx, *args, C.c_void_p(ok.data_ptr()), C.c_size_t(n), C.c_int(route)), "schnorr_verify_batch")
        return ok

    def schnorr_batch_randomizers(self, px, msgs, r, s):
        """ecsimd_schnorr_batch_randomizers: the (n, 4) randomizers a_i the MSM route of schnorr_verify_batch weighs the lanes with (odd, below 2^128)."""
        n, keep, args = self._schnorr_batch_args("schnorr_batch_randomizers", px, msgs, r, s)
        a = self.empty(n)
        self._check(self.lib.ecsimd_schnorr_batch_randomizers(self.ctx, *args, C.c_void_p(a.data_ptr() if n else 0), C.c_size_t(n)), "schnorr_batch_randomizers")
        return a

    # ---- Ed25519 batch verification and the Edwards bucket sum (include/ecsimd_ed25519_batch.h).  PUBLIC data only.
    @staticmethod
    def ed25519_msm_plan(n, bits=256, alg=0):
        """ecsimd_ed25519_msm_plan: msm_plan's dict for the bucket sum on the Edwards curve (the same schedule, its own workspace_bytes).  Host only."""
        plan = MsmPlan()
        rc = load_library().ecsimd_ed25519_msm_plan(C.c_size_t(n), C.c_int(bits), C.c_int(alg), C.byref(plan))
        if rc != 0:
            raise EcsimdHipError(f"ed25519_msm_plan(n={n}, bits={bits}, alg={alg}) failed ({rc}): bits must be 1 .. 256, n at most 2^24, alg 0 or 1 (the bucket route only)")
        return {name: int(getattr(plan, name)) for name, _ in MsmPlan._fields_}

    def ed25519_msm(self, k, pts, bits=256, alg=0, want_invalid=False):
        """ecsimd_ed25519_msm: (out, finite) = the (32,) uint8 encoding of the sum of (k[i] mod 2^bits) * P[i] and a (1,) uint8 flag (0 and the identity's
        encoding for the neutral result); k: (n, 32) uint8 little-endian INTEGERS (not residues modulo L), pts: (n, 32) uint8 encodings.  An encoding that does
        not decode strictly contributes nothing; want_invalid: a third tensor, the (1,) int32 number of them.  Capturable after one warm-up call."""
        torch = self.torch
        kp, n = self._rows_u8(k, 32, "k")
        pp, n2 = self._rows_u8(pts, 32, "pts")
        if n2 != n:
            raise EcsimdHipError(f"ed25519_msm: operands disagree on the batch length: {sorted((n, n2))}")
        out = torch.zeros((32,), dtype=torch.uint8, device=self.tdev)
        finite = torch.zeros((1,), dtype=torch.uint8, device=self.tdev)
        invalid = torch.zeros((1,), dtype=torch.int32, device=self.tdev) if want_invalid else None
        self._bind_stream()
        self._check(self.lib.ecsimd_ed25519_msm(self.ctx, kp, pp, C.c_void_p(out.data_ptr()), C.c_void_p(finite.data_ptr()), C.c_void_p(invalid.data_ptr() if want_invalid else 0),
                                                C.c_size_t(n), C.c_int(bits), C.c_int(alg)), "ed25519_msm")
        return (out, finite, invalid) if want_invalid else (out, finite)

    def _ed25519_batch_args(self, what, pk, msgs, sig, lens):
        pp, n = self._rows_u8(pk, 32, "pk")
        gp, n2 = self._rows_u8(sig, 64, "sig")
        if n2 != n:
            raise EcsimdHipError(f"{what}: operands disagree on the batch length: {sorted((n, n2))}")
        keep, mp, length, stride = self._messages(msgs, n)
        lp = self._lens_ptr(what, lens if length.value else None, n)
        self._bind_stream()
        return n, keep, (pp, mp, length, stride, lp, gp)

    def ed25519_verify_cofactored(self, pk, msgs, sig, lens=None, reject_small_order=False):
        """ecsimd_ed25519_verify_cofactored: ok, one byte per lane: s < L, A AND R decode strictly, and [8]([s]B - [h]A - R) is the identity (strict encodings
        with the cofactored equation; not ZIP-215).  The per-lane rule of ed25519_verify_batch: it names the culprits of a refused batch."""
        n, keep, args = self._ed25519_batch_args("ed25519_verify_cofactored", pk, msgs, sig, lens)
        ok = self.flags(n)
        self._check(self.lib.ecsimd_ed25519_verify_cofactored(self.ctx, *args, C.c_void_p(ok.data_ptr()), C.c_size_t(n),
                                                              C.c_int(ED25519_REJECT_SMALL_ORDER if reject_small_order else 0)), "ed25519_verify_cofactored")
        return ok

    @staticmethod
    def ed25519_batch_plan(n, msg_bytes, flags=0):
        """ecsimd_ed25519_batch_plan: what ed25519_verify_batch(n signatures, messages of at most msg_bytes bytes, flags) will do, as a dict (route, launches,
        workspace_bytes).  Host only: needs the library, no GPU and no Engine."""
        plan = Ed25519BatchPlan()
        rc = load_library().ecsimd_ed25519_batch_plan(C.c_size_t(n), C.c_size_t(msg_bytes), C.c_int(flags), C.byref(plan))
        if rc != 0:
            raise EcsimdHipError(f"ed25519_batch_plan(n={n}, msg_bytes={msg_bytes}, flags={flags}) failed ({rc}): n at most 2^24 - 1, msg_bytes at most 2^40, "
                                 "flags one of flags.ED25519_BATCH_* or-able with ED25519_REJECT_SMALL_ORDER")
        return {name: int(getattr(plan, name)) for name, _ in Ed25519BatchPlan._fields_}

    def ed25519_verify_batch(self, pk, msgs, sig, lens=None, flags=0, out=None):
        """ecsimd_ed25519_verify_batch: a (1,) uint8 tensor, 1 iff EVERY lane passes ed25519_verify_cofactored's rule (a batch with a failing lane passes with
        probability at most 2^-127 on the MSM route); an empty batch gives 1.  flags: flags.ED25519_BATCH_AUTO / _MSM / _LANES, or-able with
        flags.ED25519_REJECT_SMALL_ORDER.  out: a (1,) uint8 device tensor to write instead of a new one.  Capturable after one warm-up at the same arguments."""
        n, keep, args = self._ed25519_batch_args("ed25519_verify_batch", pk, msgs, sig, lens)
        ok = self.torch.zeros((1,), dtype=self.torch.uint8, device=self.tdev) if out is None else out
        assert ok.is_cuda and ok.device.index == self.device and ok.dtype == self.torch.uint8 and ok.numel() == 1, "out: one uint8 on the engine's device"
        self._check(self.lib.ecsimd_ed25519_verify_batch(self.ctx, *args, C.c_void_p(ok.data_ptr()), C.c_size_t(n), C.c_int(flags)), "ed25519_verify_batch")
        return ok

    def ed25519_batch_randomizers(self, pk, msgs, sig, lens=None):
        """ecsimd_ed25519_batch_randomizers: the (n, 32) uint8 little-endian randomizers z_i the MSM route of ed25519_verify_batch weighs the lanes with (odd,
        below 2^128)."""
        n, keep, args = self._ed25519_batch_args("ed25519_batch_randomizers", pk, msgs, sig, lens)
        z = self.torch.zeros((n, 32), dtype=self.torch.uint8, device=self.tdev)
        self._check(self.lib.ecsimd_ed25519_batch_randomizers(self.ctx, *args, C.c_void_p(z.data_ptr() if n else 0), C.c_size_t(n)), "ed25519_batch_randomizers")
        return z

    def _lens_ptr(self, what, lens, n):
        """The pointer of an optional int32 / uint32 device tensor of n lengths (None: NULL), as ecsimd_hip_keccak256 and the *_lens calls take it."""
        if lens is None:
            return C.c_void_p(0)
        torch = self.torch
        assert lens.is_cuda and lens.device.index == self.device and lens.is_contiguous() and lens.dim() == 1, "lens: a contiguous 1-D tensor on the engine's device"
        assert lens.dtype in (torch.int32, torch.uint32), lens.dtype
        if int(lens.shape[0]) != n:
            raise EcsimdHipError(f"{what}: operands disagree on the batch length: {sorted((n, int(lens.shape[0])))}")
        return C.c_void_p(lens.data_ptr())

    def eth_address(self, qx, qy):
        """ecsimd_hip_eth_address: (n, 20) uint8, the Ethereum address of each public key (qx, qy) -- the last 20 bytes of Keccak-256 over its 64 big-endian bytes."""
        n = qx.shape[0]; addr = self.torch.empty((n, 20), dtype=self.torch.uint8, device=self.tdev)
        self._call("eth_address", self._ptr(qx), self._ptr(qy), self._bytes_ptr(addr), C.c_size_t(n))
        return addr

    def eth_recover(self, e, r, s, v, require_low_s=False, want_key=False):
        """ecsimd_hip_eth_recover: (addr, ok), or (addr, qx, qy, ok) with want_key: the sender address behind each secp256k1 signature (r, s, v) of the digest e.
        v (uint8 tensor) is 0, 1, 27 or 28; anything else, a signature ecdsa_recover refuses and, with require_low_s, s > n / 2 give ok = 0, a zero address and a
        zero key.  Without want_key the recovered key never leaves the context workspace."""
        n = e.shape[0]; addr = self.torch.empty((n, 20), dtype=self.torch.uint8, device=self.tdev); ok = self.flags(n)
        qx, qy = (self.empty(n), self.empty(n)) if want_key else (None, None)
        self._call("eth_recover", self._ptr(e), self._ptr(r), self._ptr(s), self._ptr(v, 0), self._bytes_ptr(addr), self._ptr(qx), self._ptr(qy), self._ptr(ok, 0), C.c_size_t(n),
                   C.c_int(ETH_REQUIRE_LOW_S if require_low_s else 0))
        return (addr, qx, qy, ok) if want_key else (addr, ok)

    def _digest_lens(self, name, msgs, lens, out20):
        """One of the four *_lens calls: lane i hashes the first lens[i] bytes of its row; the result is (n, 4) integers, or the (n, 20) uint8 tensor out20."""
        n = int(msgs.shape[0]); out = self.empty(n) if out20 is None else out20
        keep, mp, length, stride = self._messages(msgs, n)
        lp = self._lens_ptr(name, lens if length.value else None, n)          # rows of no bytes: every message is empty
        self._call(name, mp, length, stride, lp, self._ptr(out) if out20 is None else self._bytes_ptr(out), C.c_size_t(n))
        return out

    def _digest20(self, name, msgs, lens=None):
        n = int(msgs.shape[0]); out = self.torch.empty((n, 20), dtype=self.torch.uint8, device=self.tdev)
        if lens is not None:
            return self._digest_lens(name + "_lens", msgs, lens, out)
        keep, mp, length, stride = self._messages(msgs, n)
        self._call(name, mp, length, stride, self._bytes_ptr(out), C.c_size_t(n))
        return out

    def ripemd160(self, msgs, lens=None):
        """ecsimd_hip_ripemd160: (n, 20) uint8, RIPEMD-160 of the rows of `msgs` (2-D uint8 device tensor, rows may be strided).  Public data.  lens (optional, as
        keccak256's): the first lens[i] bytes of row i (ecsimd_hip_ripemd160_lens)."""
        return self._digest20("ripemd160", msgs, lens)

    def hash160(self, msgs, lens=None):
        """ecsimd_hip_hash160: (n, 20) uint8, RIPEMD-160(SHA-256(row)) of the rows of `msgs`.  Public data.  lens as ripemd160's (ecsimd_hip_hash160_lens)."""
        return self._digest20("hash160", msgs, lens)

    def sha256d(self, msgs, lens=None):
        """ecsimd_hip_sha256d: SHA-256(SHA-256(row)) of the rows of `msgs` as (n, 4) integers, as sha256 returns its digests.  Public data.  lens as ripemd160's
        (ecsimd_hip_sha256d_lens): a batch of transactions to their txids."""
        if lens is not None:
            return self._digest_lens("sha256d_lens", msgs, lens, None)
        n = int(msgs.shape[0]); e = self.empty(n)
        keep, mp, length, stride = self._messages(msgs, n)
        self._call("sha256d", mp, length, stride, self._ptr(e), C.c_size_t(n))
        return e

    def btc_pubkey_hash(self, qx, qy, compressed=True):
        """ecsimd_hip_btc_pubkey_hash: (n, 20) uint8, HASH160 of the SEC1 encoding (33 bytes, or 65 with compressed=False) of each secp256k1 public key (qx, qy)."""
        n = qx.shape[0]; out = self.torch.empty((n, 20), dtype=self.torch.uint8, device=self.tdev)
        self._call("btc_pubkey_hash", self._ptr(qx), self._ptr(qy), self._bytes_ptr(out), C.c_size_t(n), C.c_int(1 if compressed else 0))
        return out

    def xonly_tweak_add(self, px, t):
        """ecsimd_hip_xonly_tweak_add: (qx, parity, ok) of Q = lift_x(px) + t G on secp256k1; ok = 0 and zeros where px does not lift, t >= n or Q is infinite."""
        n = px.shape[0]; qx, parity, ok = self.empty(n), self.flags(n), self.flags(n)
        self._call("xonly_tweak_add", self._ptr(px), self._ptr(t), self._ptr(qx), self._ptr(parity, 0), self._ptr(ok, 0), C.c_size_t(n))
        return qx, parity, ok

    def taproot_tweak_pubkey(self, px, merkle_root=None):
        """ecsimd_hip_taproot_tweak_pubkey: (qx, parity, ok), the BIP-341 output key of each internal key px; merkle_root None = key-path-only spending."""
        n = px.shape[0]; qx, parity, ok = self.empty(n), self.flags(n), self.flags(n)
        self._call("taproot_tweak_pubkey", self._ptr(px), self._ptr(merkle_root), self._ptr(qx), self._ptr(parity, 0), self._ptr(ok, 0), C.c_size_t(n))
        return qx, parity, ok

    def taproot_tweak_seckey(self, d, merkle_root=None, want_px=True):
        """ecsimd_hip_taproot_tweak_seckey: (d_out, px, ok), the SECRET key of the BIP-341 output key of each secret key d and px = x(d G) (None with want_px=False)."""
        n = d.shape[0]; d_out, ok = self.empty(n), self.flags(n); px = self.empty(n) if want_px else None
        self._call("taproot_tweak_seckey", self._ptr(d), self._ptr(merkle_root), self._ptr(d_out), self._ptr(px), self._ptr(ok, 0), C.c_size_t(n))
        return d_out, px, ok

    def btc_merkle_root(self, leaves, counts, want_mutated=False):
        """ecsimd_hip_btc_merkle_root: the Merkle roots of len(counts) trees of txids, Bitcoin's rule (the last node paired with itself where a level is odd).
        leaves: (sum(counts), 4) integers as sha256d returns them, tree after tree; counts: any host sequence of the trees' sizes, each at least 1.  Returns the
        (m, 4) roots, or (roots, mutated) with want_mutated: one byte per tree, 1 where some level holds a real pair of equal nodes (CVE-2012-2459)."""
        counts = [int(c) for c in counts]
        m = len(counts)
        offsets = (C.c_uint64 * (m + 1))()
        for t, c in enumerate(counts):
            if c < 0:
                raise EcsimdHipError("btc_merkle_root: a negative count")
            offsets[t + 1] = offsets[t] + c
        if int(leaves.shape[0]) != int(offsets[m]):
            raise EcsimdHipError(f"btc_merkle_root: {int(leaves.shape[0])} leaves for counts that add up to {int(offsets[m])}")
        roots = self.empty(m); mutated = self.flags(m) if want_mutated else None
        lp = self._ptr(leaves); self._rows.clear()              # leaves and roots have their own lengths
        self._call("btc_merkle_root", lp, offsets, C.c_size_t(m), C.c_void_p(roots.data_ptr()), C.c_void_p(mutated.data_ptr() if want_mutated else 0))
        return (roots, mutated) if want_mutated else roots

    def tapleaf_hash(self, scripts, lens=None, leaf_version=0xc0):
        """ecsimd_hip_tapleaf_hash: (n, 4) integers, the BIP-341 leaf hash H_TapLeaf(version || compact_size(len) || script) of the rows of `scripts` (2-D uint8
        device tensor, rows may be strided; lens as keccak256's).  leaf_version: one int for every lane, or a uint8 device tensor of n versions."""
        n = int(scripts.shape[0]); e = self.empty(n)
        keep, mp, length, stride = self._messages(scripts, n)
        per_lane = not isinstance(leaf_version, int)
        vp = self._ptr(leaf_version, 0) if per_lane else C.c_void_p(0)
        self._call("tapleaf_hash", mp, length, stride, self._lens_ptr("tapleaf_hash", lens if length.value else None, n), vp, C.c_uint32(0 if per_lane else leaf_version), self._ptr(e), C.c_size_t(n))
        return e

    def taproot_merkle_path(self, leaf, path, depth):
        """ecsimd_hip_taproot_merkle_path: (root, ok), the TapBranch walk from each leaf hash over its control block's path.  path: 2-D uint8 device tensor, row i
        holding lane i's nodes of 32 bytes, the leaf's sibling first (rows may be strided: the tail of a control block); depth: one int for every lane, or a uint8
        device tensor of n depths.  ok = 0 and root = 0 where a depth is above 128.  A row must hold 32 x depth bytes (checked for an int depth only); rows of no bytes mean depth 0."""
        n = int(leaf.shape[0]); root, ok = self.empty(n), self.flags(n)
        keep, pp, width, stride = self._messages(path, n)
        per_lane = not isinstance(depth, int)
        if per_lane and width.value == 0:
            per_lane, depth = False, 0                          # rows of no bytes hold no node
        if not per_lane and depth <= 128 and 32 * depth > width.value:
            raise EcsimdHipError(f"taproot_merkle_path: rows of {width.value} bytes for a depth of {depth}")
        dp = self._ptr(depth, 0) if per_lane else C.c_void_p(0)
        self._call("taproot_merkle_path", self._ptr(leaf), pp, stride, dp, C.c_uint32(0 if per_lane else depth), self._ptr(root), self._ptr(ok, 0), C.c_size_t(n))
        return root, ok

    def taproot_script_path_ok(self, qx, control_blocks, depths, scripts, lens=None):
        """BIP-341's script-path check on the device, from existing calls: a uint8 verdict per lane, 1 where the control block and the script commit to the
        output key qx.  control_blocks: (n, 33 + 32 d) uint8 device tensor -- the control byte (leaf version | the output key's parity), the internal key, the
        path; depths: uint8 device tensor, the number of path nodes of each lane (the rest of its row is not read); scripts / lens as tapleaf_hash's.
        tapleaf_hash -> taproot_merkle_path -> taproot_tweak_pubkey -> the comparison of qx and the parity."""
        control = control_blocks[:, 0]
        keys = self.torch.empty((int(control_blocks.shape[0]), 32), dtype=self.torch.uint8, device=self.tdev)      # a copy of its own: from_bytes_be wants 16-byte alignment
        keys.copy_(control_blocks[:, 1:33])
        px = self.from_bytes_be(keys)
        leaf = self.tapleaf_hash(scripts, lens, (control & 0xfe).contiguous())
        root, in_bound = self.taproot_merkle_path(leaf, control_blocks[:, 33:], depths)
        q, parity, ok = self.taproot_tweak_pubkey(px, root)
        return ok & in_bound & self.cmp_eq(q, qx) & (parity == (control & 1)).to(self.torch.uint8)

    def sha512(self, msgs):
        """ecsimd_hip_sha512: (n, 64) uint8, SHA-512 of the rows of `msgs` (2-D uint8 device tensor, rows may be strided).  Public data."""
        n = int(msgs.shape[0]); out = self.torch.empty((n, 64), dtype=self.torch.uint8, device=self.tdev)
        keep, mp, length, stride = self._messages(msgs, n)
        self._call("sha512", mp, length, stride, self._bytes_ptr(out), C.c_size_t(n))
        return out

    def hmac_sha512(self, keys, msgs):
        """ecsimd_hip_hmac_sha512: (n, 64) uint8, HMAC-SHA-512 of the rows of `msgs` under `keys`: a 1-D uint8 device tensor is ONE key for the whole call, a 2-D
        one holds a key per row (rows may be strided).  Public data."""
        torch = self.torch
        n = int(msgs.shape[0]); out = torch.empty((n, 64), dtype=torch.uint8, device=self.tdev)
        keep, mp, length, stride = self._messages(msgs, n)
        assert keys.is_cuda and keys.device.index == self.device and keys.dtype == torch.uint8 and keys.dim() in (1, 2), (keys.dtype, keys.shape)
        if keys.dim() == 1:
            keys = keys.contiguous()
            kp, klen, kstride = C.c_void_p(keys.data_ptr() if keys.shape[0] else 0), C.c_size_t(int(keys.shape[0])), C.c_size_t(0)
        else:
            keys, kp, klen, kstride = self._messages(keys, n)
        self._call("hmac_sha512", kp, klen, kstride, mp, length, stride, self._bytes_ptr(out), C.c_size_t(n))
        return out

    def _index(self, index, n, what):
        """(pointer, index_all) of a BIP-32 index argument: an int for every lane, or an int32 / uint32 device tensor of n indices."""
        if isinstance(index, (int, np.integer)):
            index = int(index)
            if not 0 <= index < 1 << 32:
                raise EcsimdHipError(f"{what}: the index {index} is not a 32-bit value")
            return C.c_void_p(0), C.c_uint32(index)
        torch = self.torch
        assert index.is_cuda and index.device.index == self.device and index.is_contiguous() and index.dim() == 1, "index: a contiguous 1-D tensor on the engine's device"
        assert index.dtype in (torch.int32, torch.uint32), index.dtype
        if int(index.shape[0]) != n:
            raise EcsimdHipError(f"{what}: operands disagree on the batch length: {sorted((n, int(index.shape[0])))}")
        return C.c_void_p(index.data_ptr() if n else 0), C.c_uint32(0)

    def bip32_master(self, seeds):
        """ecsimd_hip_bip32_master: (k, c, ok), the BIP-32 master key and chain code of each SECRET seed, a row of `seeds` (2-D uint8 device tensor of 16 .. 64
        columns, rows may be strided).  ok = 0 and zeros where the left half of the hash is 0 or >= n."""
        n = int(seeds.shape[0]); k, c, ok = self.empty(n), self.empty(n), self.flags(n)
        keep, sp, length, stride = self._messages(seeds, n)
        self._call("bip32_master", sp, length, stride, self._ptr(k), self._ptr(c), self._ptr(ok, 0), C.c_size_t(n))
        return k, c, ok

    def bip32_ckd_priv(self, k, c, index, all_hardened=False):
        """ecsimd_hip_bip32_ckd_priv: (k_child, c_child, ok), BIP-32's CKDpriv of the SECRET keys k and chain codes c at `index` (an int, or an int32 / uint32
        device tensor with one index per lane).  all_hardened: the caller's promise that every index is >= 2^31 -- no point multiplication then; a lane that breaks
        it is refused.  ok = 0 and zeros where k is not in [1, n - 1]."""
        n = k.shape[0]; kc, cc, ok = self.empty(n), self.empty(n), self.flags(n)
        ip, iall = self._index(index, n, "bip32_ckd_priv")
        self._call("bip32_ckd_priv", self._ptr(k), self._ptr(c), ip, iall, self._ptr(kc), self._ptr(cc), self._ptr(ok, 0), C.c_size_t(n),
                   C.c_int(BIP32_ALL_HARDENED if all_hardened else 0))
        return kc, cc, ok

    def bip32_ckd_pub(self, qx, qy, c, index):
        """ecsimd_hip_bip32_ckd_pub: (cx, cy, c_child, ok), BIP-32's CKDpub of the public keys (qx, qy) and chain codes c at `index` (as for bip32_ckd_priv).
        ok = 0 and zeros for a hardened index and for a key that is not on the curve.  Public data."""
        n = qx.shape[0]; cx, cy, cc, ok = self.empty(n), self.empty(n), self.empty(n), self.flags(n)
        ip, iall = self._index(index, n, "bip32_ckd_pub")
        self._call("bip32_ckd_pub", self._ptr(qx), self._ptr(qy), self._ptr(c), ip, iall, self._ptr(cx), self._ptr(cy), self._ptr(cc), self._ptr(ok, 0), C.c_size_t(n))
        return cx, cy, cc, ok

    def bip32_derive_priv(self, k, c, path):
        """(k, c, ok) at the end of `path` (a list of ints, one index per level, the same for every lane) below the SECRET nodes (k, c): a host loop of
        bip32_ckd_priv, on the hardened-only route at hardened levels.  ok is the AND of the levels' masks (a refused lane's zero key is refused again below)."""
        ok = self.torch.ones((k.shape[0],), dtype=self.torch.uint8, device=self.tdev)
        for index in path:
            k, c, level_ok = self.bip32_ckd_priv(k, c, int(index), all_hardened=int(index) >= 1 << 31)
            ok = ok & level_ok
        return k, c, ok

    def _lens(self, lens, n, what):
        """The pointer of a per-lane length argument: None, or an int32 / uint32 device tensor of n lengths."""
        if lens is None:
            return C.c_void_p(0)
        torch = self.torch
        assert lens.is_cuda and lens.device.index == self.device and lens.is_contiguous() and lens.dim() == 1, "lens: a contiguous 1-D tensor on the engine's device"
        assert lens.dtype in (torch.int32, torch.uint32), lens.dtype
        if int(lens.shape[0]) != n:
            raise EcsimdHipError(f"{what}: operands disagree on the batch length: {sorted((n, int(lens.shape[0])))}")
        return C.c_void_p(lens.data_ptr() if n else 0)

    def _rows_or_one(self, t, n, what):
        """(keep-alive, pointer, length, stride) of a 2-D uint8 device tensor with a row per lane, or of a 1-D one that serves the whole call (stride 0)."""
        torch = self.torch
        assert t.is_cuda and t.device.index == self.device and t.dtype == torch.uint8 and t.dim() in (1, 2), (t.dtype, t.shape)
        if t.dim() == 1:
            t = t.contiguous()
            return t, C.c_void_p(t.data_ptr() if t.shape[0] else 0), C.c_size_t(int(t.shape[0])), C.c_size_t(0)
        try:
            return self._messages(t, n)
        except EcsimdHipError as exc:
            raise EcsimdHipError(f"{what}: {exc}") from None

    def pbkdf2_hmac_sha512(self, passwords, salts, iterations, dk_bytes, pw_lens=None, salt_lens=None, out=None):
        """ecsimd_hip_pbkdf2_hmac_sha512: (n, dk_bytes) uint8, PBKDF2-HMAC-SHA-512 of the rows of `passwords` (2-D uint8 device tensor, rows may be strided) under
        `salts`: a 2-D tensor holds a salt per row, a 1-D one is ONE salt for the whole call.  pw_lens / salt_lens (optional int32 / uint32 device tensors of n
        lengths, each at most the row length): lane i uses the first lens[i] bytes of its row.  out (optional): a 2-D uint8 device tensor of n rows of at least
        dk_bytes columns whose rows are written in place (a column slice of a wider array keeps the bytes between the keys).  SECRET contents, public lengths."""
        torch = self.torch
        assert passwords.dim() == 2, passwords.shape
        n = int(passwords.shape[0])
        if out is None:
            out = torch.empty((n, int(dk_bytes)), dtype=torch.uint8, device=self.tdev)
        assert out.is_cuda and out.device.index == self.device and out.dtype == torch.uint8 and out.dim() == 2 and out.shape[1] >= dk_bytes and (out.stride(1) == 1 or out.shape[1] <= 1), (out.dtype, out.shape)
        if int(out.shape[0]) != n:
            raise EcsimdHipError(f"pbkdf2_hmac_sha512: operands disagree on the batch length: {sorted((n, int(out.shape[0])))}")
        keep_p, pp, plen, pstride = self._rows_or_one(passwords, n, "pbkdf2_hmac_sha512")
        keep_s, sp, slen, sstride = self._rows_or_one(salts, n, "pbkdf2_hmac_sha512")
        if salts.dim() == 1 and salt_lens is not None:
            raise EcsimdHipError("pbkdf2_hmac_sha512: one salt for the call takes no salt_lens")
        stride = int(out.stride(0)) if n > 1 else max(int(out.shape[1]), int(dk_bytes))
        self._call("pbkdf2_hmac_sha512", pp, plen, pstride, self._lens(pw_lens, n, "pbkdf2_hmac_sha512"), sp, slen, sstride, self._lens(salt_lens, n, "pbkdf2_hmac_sha512"),
                   C.c_uint32(int(iterations)), C.c_void_p(out.data_ptr() if n else 0), C.c_size_t(int(dk_bytes)), C.c_size_t(stride), C.c_size_t(n))
        return out[:, :dk_bytes] if out.shape[1] != dk_bytes else out

    def bip39_seed(self, mnemonics, passphrases=None, mnemonic_lens=None, passphrase_lens=None):
        """ecsimd_hip_bip39_seed: (n, 64) uint8, the BIP-39 seed of each SECRET sentence, a row of `mnemonics` (2-D uint8 device tensor; mnemonic_lens: the
        sentences' own lengths where they differ).  passphrases: None = the empty passphrase, a 1-D tensor = one for the call, a 2-D one = a row per lane (with
        passphrase_lens).  Bytes as given: NFKD, the word list and the checksum are the caller's."""
        torch = self.torch
        assert mnemonics.dim() == 2, mnemonics.shape
        n = int(mnemonics.shape[0]); seed = torch.empty((n, 64), dtype=torch.uint8, device=self.tdev)
        if passphrases is None:
            passphrases = torch.empty((0,), dtype=torch.uint8, device=self.tdev)
        keep_m, mp, mlen, mstride = self._rows_or_one(mnemonics, n, "bip39_seed")
        keep_p, pp, plen, pstride = self._rows_or_one(passphrases, n, "bip39_seed")
        if passphrases.dim() == 1 and passphrase_lens is not None:
            raise EcsimdHipError("bip39_seed: one passphrase for the call takes no passphrase_lens")
        self._call("bip39_seed", mp, mlen, mstride, self._lens(mnemonic_lens, n, "bip39_seed"), pp, plen, pstride, self._lens(passphrase_lens, n, "bip39_seed"),
                   C.c_void_p(seed.data_ptr() if n else 0), C.c_size_t(n))
        return seed

    def bip39_master(self, mnemonics, passphrases=None, mnemonic_lens=None, passphrase_lens=None):
        """(k, c, ok): the BIP-32 master key and chain code of each SECRET sentence -- bip39_seed, then bip32_master on the 64-byte seeds."""
        return self.bip32_master(self.bip39_seed(mnemonics, passphrases, mnemonic_lens, passphrase_lens))

    def fe29_raw(self, curve, op, inputs, swap=0):
        """ecsimd_hip_fe29_raw: one function of the reduced-radix layer on raw int32 limbs; `inputs` is an int32 tensor (n, NIN, 9); returns (n, NOUT, 9)."""
        torch = self.torch
        nout = 6 if op in (0, 10) else 1 if op in (7, 8) else 4 if op == 9 else 3
        assert inputs.dtype == torch.int32 and inputs.dim() == 3 and inputs.shape[2] == 9 and inputs.is_contiguous() and inputs.device.index == self.device
        n = inputs.shape[0]
        out = torch.empty((n, nout, 9), dtype=torch.int32, device=self.tdev)
        self._bind_stream()
        self._check(self.lib.ecsimd_hip_fe29_raw(self.ctx, C.c_int(curve), C.c_int(op), C.c_void_p(inputs.data_ptr()), C.c_void_p(out.data_ptr()), C.c_size_t(n), C.c_int(swap)), "fe29_raw")
        return out

    def workspace_bytes(self):
        """ecsimd_hip_workspace_info as a uint8 numpy copy of the context's scratch block (diagnostic: what the last call left behind)."""
        ptr, size = C.c_void_p(), C.c_size_t()
        self._check(self.lib.ecsimd_hip_workspace_info(self.ctx, C.byref(ptr), C.byref(size)), "workspace_info")
        self.torch.cuda.synchronize(self.tdev)
        host = np.empty(size.value, dtype=np.uint8)
        if size.value:
            self._check(self.lib.ecsimd_hip_memcpy_d2h(self.ctx, host.ctypes.data_as(C.c_void_p), ptr, C.c_size_t(size.value)), "memcpy_d2h")
        return host

    def scalar_mult_p256(self, k, xm, ym, out=None):
        n = k.shape[0]
        r = out if out is not None else [self.empty(n) for _ in range(3)]
        self._call("scalar_mult_p256", self._ptr(k), self._ptr(xm), self._ptr(ym), *[self._ptr(t) for t in r], C.c_size_t(n))
        return tuple(r)

    # ---- synthetic inputs / measurement
    def fill_random(self, n, seed, stream, first_index=0, clear_top_bits=0, out=None):
        t = out if out is not None else self.empty(n)
        self._call("fill_random", self._ptr(t), C.c_size_t(n), _u64(seed), _u64(stream), _u64(first_index), C.c_int(clear_top_bits)); return t

    def peak_mad32(self, iters=2048, reps=1):
        """(mad32 executed, milliseconds) of the fastest of `reps` runs of the dependency-free
        v_mad_u64_u32 stream (several runs let the clock settle: the probe is only a few ms long)."""
        best = None
        for _ in range(max(1, reps)):
            mads, ms = C.c_double(0), C.c_double(0)
            self._call("peak_mad32", C.c_int(iters), C.byref(mads), C.byref(ms))
            if best is None or mads.value / ms.value > best[0] / best[1]:
                best = (mads.value, ms.value)
        return best


def register_modulus(p: int, prime: bool = False) -> int:
    """ecsimd_hip_register_modulus: the field id of the odd modulus p (process-wide; no GPU needed)."""
    lib = load_library()
    limbs = (C.c_uint64 * 4)(*[(p >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)])
    fid = C.c_int(-1)
    rc = lib.ecsimd_hip_register_modulus(limbs, C.c_int(MODULUS_PRIME if prime else 0), C.byref(fid))
    if rc != 0:
        raise EcsimdHipError(f"ecsimd_hip_register_modulus({p:#x}) failed with {rc} (the modulus must be odd and >= 3)")
    return fid.value


CURVE_GENERIC_KERNELS = 1
FIRST_REGISTERED_CURVE = 0x10000


def register_curve(p: int, a: int, b: int, gx: int, gy: int, n: int | None = None, generic_kernels: bool = False) -> int:
    """ecsimd_hip_register_curve: the curve id of y^2 = x^3 + a x + b over GF(p) with generator (gx, gy) -- the reference's curve_group<Curve> for any
    Curve, as a run-time registration (process-wide; no GPU needed).  generic_kernels: register P-256 / secp256k1 parameters like any other curve."""
    lib = load_library()
    lim = lambda v: (C.c_uint64 * 4)(*[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)])
    cid = C.c_int(-1)
    rc = lib.ecsimd_hip_register_curve(lim(p), lim(a % p), lim(b % p), lim(gx), lim(gy), lim(n) if n is not None else None,
                                       C.c_int(CURVE_GENERIC_KERNELS if generic_kernels else 0), C.byref(cid))
    if rc != 0:
        raise EcsimdHipError(f"ecsimd_hip_register_curve(p = {p:#x}) failed with {rc}: p must be a prime = 3 mod 4, the generator on the curve, the curve non-singular")
    return cid.value


CURVE_HAS_ORDER, CURVE_COMB, CURVE_ECDSA, CURVE_WINDOW_VARIABLE_BASE = 1, 2, 4, 8


def curve_capabilities(curve: int) -> int:
    """ecsimd_hip_curve_capabilities: what an id can do beyond the reference's layers (a mask of CURVE_*; host only)."""
    lib = load_library()
    caps = C.c_int(0)
    rc = lib.ecsimd_hip_curve_capabilities(C.c_int(curve), C.byref(caps))
    if rc != 0:
        raise EcsimdHipError(f"ecsimd_hip_curve_capabilities({curve}) -> {rc}: unknown curve id")
    return caps.value


def shard_range_c(n_total: int, member: int, members: int):
    """ecsimd_hip_shard_range: the C ABI's partition of a batch over a device group (pure host arithmetic)."""
    lib = load_library()
    first, count = C.c_size_t(0), C.c_size_t(0)
    rc = lib.ecsimd_hip_shard_range(C.c_size_t(n_total), C.c_int(member), C.c_int(members), C.byref(first), C.byref(count))
    if rc != 0:
        raise EcsimdHipError(f"ecsimd_hip_shard_range({n_total}, {member}, {members}) -> {rc}")
    return int(first.value), int(count.value)


class DeviceGroup:
    """ecsimd_hip_group_*: one batch over several GPUs behind the C ABI (one context per device, contiguous shards,
    one RCCL gather to member 0).  `devices` may list a device twice (members then exchange by device copies)."""

    def __init__(self, devices):
        import torch
        self.torch = torch
        self.lib = load_library()
        self.lib.ecsimd_hip_group_last_error.restype = C.c_char_p
        self.devices = [int(d) for d in devices]
        self.g = C.c_void_p()
        arr = (C.c_int * len(self.devices))(*self.devices)
        rc = self.lib.ecsimd_hip_group_init(arr, C.c_int(len(self.devices)), C.byref(self.g))
        if rc != 0:
            raise EcsimdHipError(f"ecsimd_hip_group_init({self.devices}) failed with {rc}")

    def close(self):
        if self.g:
            self.lib.ecsimd_hip_group_destroy(self.g)
            self.g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.ecsimd_hip_group_last_error(self.g)
            raise EcsimdHipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    @property
    def size(self):
        return int(self.lib.ecsimd_hip_group_size(self.g))

    @property
    def uses_rccl(self):
        return bool(self.lib.ecsimd_hip_group_uses_rccl(self.g))

    @property
    def rccl_version(self):
        """ncclGetVersion of the RCCL the gather goes through (22606 = 2.26.6); 0 when the group needs none."""
        return int(self.lib.ecsimd_hip_group_rccl_version(self.g))

    def alloc_outputs(self, n, flags=0, x_only=False):
        torch = self.torch
        dev0 = torch.device("cuda", self.devices[0])
        return [torch.empty((n, 4), dtype=torch.int64, device=dev0) for _ in range((1 if x_only else 2) if flags & 2 else 3)]

    def enqueue(self, curve, k_shards, x_shards, y_shards, outs, n, flags=0):
        """ecsimd_hip_group_scalar_mult without the wait: *_shards[m] = member m's slice (a tensor on that member's device),
        outs = 1 (x only), 2 (affine) or 3 (Jacobian) tensors of n rows on member 0's device.  The inputs must be complete
        (they were produced on torch's streams, the group runs on its own)."""
        G = self.size
        ptrs = lambda ts: (C.c_void_p * G)(*[C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0) for t in ts])
        o = [C.c_void_p(t.data_ptr()) for t in outs] + [C.c_void_p(0)] * (3 - len(outs))
        self._check(self.lib.ecsimd_hip_group_scalar_mult(self.g, C.c_int(curve), ptrs(k_shards), ptrs(x_shards), ptrs(y_shards),
                                                          o[0], o[1], o[2], C.c_size_t(n), C.c_int(flags)), "group_scalar_mult")

    def sync(self):
        """ecsimd_hip_group_sync: waits for every member and the gather; returns the last gather's duration in ms (-1: none)."""
        ms = C.c_double(0)
        self._check(self.lib.ecsimd_hip_group_sync(self.g, C.byref(ms)), "group_sync")
        return float(ms.value)

    def member_ms(self, member):
        ms = C.c_double(0)
        self._check(self.lib.ecsimd_hip_group_member_ms(self.g, C.c_int(member), C.byref(ms)), "group_member_ms")
        return float(ms.value)

    def scalar_mult(self, curve, k_shards, x_shards, y_shards, n, flags=0, x_only=False):
        """Device-resident form, synchronous: returns (ox[, oy[, oz]]) on member 0's device and the gather time in ms."""
        outs = self.alloc_outputs(n, flags, x_only)
        for m in range(self.size):
            self.torch.cuda.synchronize(self.devices[m])         # the inputs were produced on torch's streams
        self.enqueue(curve, k_shards, x_shards, y_shards, outs, n, flags)
        return tuple(outs), self.sync()

    def rccl_selftest(self, elements=1 << 16):
        self._check(self.lib.ecsimd_hip_group_rccl_selftest(self.g, C.c_size_t(elements)), "group_rccl_selftest")

    def scalar_mult_host(self, curve, k, x, y, flags=0, x_only=False):
        """Host-array form: numpy uint64 (n, 4) arrays in, numpy arrays out."""
        k, x, y = (np.ascontiguousarray(a, dtype=np.uint64) for a in (k, x, y))
        n = len(k)
        outs = [np.empty((n, 4), dtype=np.uint64) for _ in range((1 if x_only else 2) if flags & 2 else 3)]
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        o = [p(a) for a in outs] + [C.c_void_p(0)] * (3 - len(outs))
        self._check(self.lib.ecsimd_hip_group_scalar_mult_host(self.g, C.c_int(curve), p(k), p(x), p(y), o[0], o[1], o[2], C.c_size_t(n), C.c_int(flags)),
                    "group_scalar_mult_host")
        return tuple(outs)
