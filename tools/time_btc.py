"""Times the Bitcoin calls on one MI355X next to their yardsticks, in one process and run:

    python tools/time_btc.py [--lanes 4194304] [--reps 9]

HIP events on the engine's stream (torch's current stream), two warm-up calls, then `reps` repetitions: the median, with the fastest and the slowest in
brackets.  Yardsticks: eth_address for btc_pubkey_hash, sha256 at the same length (33 and 128 bytes) for hash160 / sha256d / ripemd160, schnorr_verify and the
chain of existing public calls (sha256 over tag block || data, sec1_decode, scalar_mult_base, affine_add) for taproot_tweak_pubkey, schnorr_sign for
taproot_tweak_seckey.  Prints one line per call and the ratios; profiles/r09/btc.txt keeps the output.
"""
import argparse
import hashlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    import torch
    from ecsimd_amd import Engine, SECP256K1
    eng = Engine(0)
    n = a.lanes
    OUT_AFFINE, WINDOWED_SIGNED = 2, 8
    msgs = {b: torch.randint(0, 256, (n, b), dtype=torch.uint8, device=eng.tdev) for b in (32, 33, 128)}
    d = eng.fill_random(n, 7, 1, clear_top_bits=1)
    roots = eng.fill_random(n, 8, 1)
    sign = 1 << 20                                             # the signing calls keep up to 256 B per lane of secrets in the workspace: in slices
    parts = [eng.schnorr_sign(d[i:i + sign], msgs[32][i:i + sign]) for i in range(0, n, sign)]
    px, r, s, ok = (torch.cat([p[j] for p in parts]) for j in range(4))
    assert bool(ok.all())
    qx, qy = eng.scalar_mult_base(SECP256K1, d, OUT_AFFINE | WINDOWED_SIGNED)[:2]
    t = hashlib.sha256(b"TapTweak").digest()
    tag = torch.from_numpy(__import__("numpy").frombuffer(t + t, dtype="uint8").copy()).to(eng.tdev)
    two = torch.full((n, 1), 2, dtype=torch.uint8, device=eng.tdev)

    def chain():
        """taproot_tweak_pubkey's result from the engine's other public calls (t >= n is not refused here: the yardstick does a little less)"""
        pb, hb = eng.to_bytes_be(px).reshape(n, 32), eng.to_bytes_be(roots).reshape(n, 32)
        tw = eng.sha256(torch.cat([tag.expand(n, 64), pb, hb], dim=1).contiguous())
        x, y, lifted = eng.sec1_decode(SECP256K1, torch.cat([two, pb], dim=1).contiguous(), compressed=True)
        tg = eng.scalar_mult_base(SECP256K1, tw, OUT_AFFINE | WINDOWED_SIGNED)
        return eng.affine_add(SECP256K1, (x, y), tg[:2])

    def seckey_sliced():
        for i in range(0, n, sign):
            eng.taproot_tweak_seckey(d[i:i + sign], roots[i:i + sign])

    def sign_sliced():
        for i in range(0, n, sign):
            eng.schnorr_sign(d[i:i + sign], msgs[32][i:i + sign])

    def timed(fn):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record(); t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return statistics.median(ms), min(ms), max(ms)

    calls = [("eth_address", lambda: eng.eth_address(qx, qy)), ("btc_pubkey_hash", lambda: eng.btc_pubkey_hash(qx, qy)),
             ("btc_pubkey_hash_uncompressed", lambda: eng.btc_pubkey_hash(qx, qy, compressed=False))]
    for b in (33, 128):
        calls += [(f"sha256_{b}", lambda b=b: eng.sha256(msgs[b])), (f"sha256d_{b}", lambda b=b: eng.sha256d(msgs[b])),
                  (f"hash160_{b}", lambda b=b: eng.hash160(msgs[b])), (f"ripemd160_{b}", lambda b=b: eng.ripemd160(msgs[b]))]
    calls += [("schnorr_verify", lambda: eng.schnorr_verify(px, msgs[32], r, s)), ("taproot_tweak_pubkey", lambda: eng.taproot_tweak_pubkey(px, roots)),
              ("taproot_tweak_pubkey_key_path", lambda: eng.taproot_tweak_pubkey(px)), ("xonly_tweak_add", lambda: eng.xonly_tweak_add(px, roots)),
              ("chain_of_existing_calls", chain), ("schnorr_sign", sign_sliced), ("taproot_tweak_seckey", seckey_sliced)]
    rate = {}
    for name, fn in calls:
        ms, lo, hi = timed(fn)
        rate[name] = n / ms / 1e3
        print(f"{name:30s} {ms:9.3f} ms [{lo:.3f} .. {hi:.3f}]  {rate[name]:9.1f} M/s  ({n} lanes, median of {a.reps})", flush=True)
    ratio = lambda x, y: print(f"{x} / {y} = {rate[x] / rate[y]:.3f}")
    ratio("btc_pubkey_hash", "eth_address")
    for b in (33, 128):
        ratio(f"hash160_{b}", f"sha256_{b}"); ratio(f"sha256d_{b}", f"sha256_{b}")
    ratio("taproot_tweak_pubkey", "schnorr_verify"); ratio("taproot_tweak_pubkey", "chain_of_existing_calls"); ratio("taproot_tweak_seckey", "schnorr_sign")


if __name__ == "__main__":
    main()
