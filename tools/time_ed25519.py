"""Times the three Ed25519 calls on one MI355X next to their yardsticks, in one process and run:

    python tools/time_ed25519.py [--lanes 1048576] [--big 4194304] [--reps 5]

HIP events on the engine's stream (torch's current stream), two warm-up calls, then `reps` repetitions: the median, with the fastest and the slowest in
brackets.  ed25519_verify at `lanes` and `big` lanes with 64- and 200-byte messages, ed25519_sign and ed25519_pubkey at `lanes`; beside them schnorr_verify and
schnorr_sign on 32-byte messages at `lanes`, timed in the same run -- the in-run ratio is what the README quotes.  Also timed: ONE launch sequence of
ed25519_verify at its lane chunk (ED25519_VERIFY_CHUNK in capi.hip), the longest single launch of the feature, to hold against what DESIGN.md section 4d
allows a launch on a shared device.  The a-priori figure beside the measured rate: the field multiplications per verification that
profiles/r13/ed25519_listing.json derives from the shipped listing (tools/ed25519_listing.py).
Prints one line per call and the ratios.
"""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1 << 20)
    ap.add_argument("--big", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from ecsimd_amd import Engine
    eng = Engine(0)
    n = a.lanes
    capi = open(os.path.join(ROOT, "ecsimd_amd", "csrc", "capi.hip")).read()
    chunk = 1 << int(re.search(r"ED25519_VERIFY_CHUNK = \(size_t\)1 << (\d+);", capi).group(1))

    def timed(fn):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record(); t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return statistics.median(ms), min(ms), max(ms)

    # 64 distinct signers tiled over the batch: signed on the device, so every timed verification accepts and runs the whole loop
    def batch(lanes, length):
        tile = 1 << 12
        seeds = torch.randint(0, 256, (tile, 32), dtype=torch.uint8, device=eng.tdev)
        msgs = torch.randint(0, 256, (tile, length), dtype=torch.uint8, device=eng.tdev)
        sig, pk = eng.ed25519_sign(seeds, msgs)
        reps = (lanes + tile - 1) // tile
        return (seeds.repeat(reps, 1)[:lanes].contiguous(), msgs.repeat(reps, 1)[:lanes].contiguous(), sig.repeat(reps, 1)[:lanes].contiguous(),
                pk.repeat(reps, 1)[:lanes].contiguous())

    rate = {}

    def report(name, fn, lanes):
        ms, lo, hi = timed(fn)
        rate[name] = lanes / ms / 1e3
        print(f"{name:34s} {ms:10.3f} ms [{lo:.3f} .. {hi:.3f}]  {rate[name]:10.3f} M/s  ({lanes} lanes, median of {a.reps})", flush=True)
        return ms

    for lanes in (n, a.big):
        for length in (64, 200):
            seeds, msgs, sig, pk = batch(lanes, length)
            ok = eng.ed25519_verify(pk, msgs, sig)
            assert int(ok.sum()) == lanes, "the timed batch does not verify"
            report(f"ed25519_verify_{length}B_2^{lanes.bit_length() - 1}", lambda: eng.ed25519_verify(pk, msgs, sig), lanes)
            if lanes == n and length == 64:
                report("ed25519_sign_64B", lambda: eng.ed25519_sign(seeds, msgs), lanes)
                report("ed25519_pubkey", lambda: eng.ed25519_pubkey(seeds), lanes)
                one = min(lanes, chunk)
                ms = report("ed25519_verify_one_chunk", lambda: eng.ed25519_verify(pk[:one], msgs[:one], sig[:one]), one)
                print(f"  the longest single launch is below that call's {ms:.3f} ms (front end + loop, {one} lanes)")
            del seeds, msgs, sig, pk, ok
    # the yardsticks: BIP-340 on secp256k1, 32-byte messages
    d = torch.randint(1, 2**62, (n, 4), dtype=torch.int64, device=eng.tdev)
    m32 = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=eng.tdev)
    px, r, s, ok = eng.schnorr_sign(d, m32)
    assert int(ok.sum()) == n
    report("schnorr_sign_32B", lambda: eng.schnorr_sign(d, m32), n)
    report("schnorr_verify_32B", lambda: eng.schnorr_verify(px, m32, r, s), n)
    lanes_name = f"2^{n.bit_length() - 1}"
    print(f"ed25519_verify (64 B) / schnorr_verify (32 B), rate: {rate['ed25519_verify_64B_' + lanes_name] / rate['schnorr_verify_32B']:.3f}")
    print(f"ed25519_sign (64 B) / schnorr_sign (32 B), rate: {rate['ed25519_sign_64B'] / rate['schnorr_sign_32B']:.3f}")
    listing = os.path.join(ROOT, "profiles", "r13", "ed25519_listing.json")
    if os.path.exists(listing):
        J = json.load(open(listing))
        valu = J["verify_valu_per_lane"]
        print(f"VALU instructions issued per second by ed25519_verify (64 B): {valu * rate['ed25519_verify_64B_' + lanes_name] * 1e-6:.1f} T "
              f"({valu} per verification from the listing, {J['verify_field_multiplications']} field multiplications)")


if __name__ == "__main__":
    main()
