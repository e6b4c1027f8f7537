"""Times the five P-384 calls on one MI355X next to their yardsticks, in one process and run:

    python tools/time_p384.py [--lanes 1048576] [--reps 5] [--out FILE]

HIP events on the engine's stream (torch's current stream), two warm-up calls, then `reps` repetitions: the median, with the fastest and the slowest in
brackets.  p384_sha384 (64-byte messages), p384_pubkey, p384_ecdh, p384_ecdsa_sign and p384_ecdsa_verify at `lanes`, alternating with ecdsa_verify on P-256 and
ed25519_verify (64-byte messages) at the same batch, each yardstick timed twice -- before and after the P-384 calls -- so that a drift of the device's clock
shows.  The in-run ratios are what the README quotes.  The a-priori figure beside the measured rate: the VALU instructions per verification that
profiles/r18/p384_listing.json derives from the shipped listing (tools/p384_listing.py).  Prints one line per call and the ratios; --out appends them to a file.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ecsimd_amd import Engine, P256
    eng = Engine(0)
    n = a.lanes
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record(); t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return statistics.median(ms), min(ms), max(ms)

    rate = {}

    def report(name, fn, lanes):
        ms, lo, hi = timed(fn)
        rate[name] = lanes / ms / 1e3
        say(f"{name:28s} {ms:10.3f} ms [{lo:.3f} .. {hi:.3f}, spread {100 * (hi - lo) / ms:.1f} %]  {rate[name]:10.3f} M/s  ({lanes} lanes, median of {a.reps})")

    def tile(t, lanes):
        return t.repeat((lanes + t.shape[0] - 1) // t.shape[0], 1)[:lanes].contiguous()

    # 4096 distinct signers tiled over the batch, signed on the device: every timed verification accepts and runs the whole loop
    small = 1 << 12
    d = torch.randint(0, 256, (small, 48), dtype=torch.uint8, device=eng.tdev); d[:, 0] = 0
    msgs = torch.randint(0, 256, (small, 64), dtype=torch.uint8, device=eng.tdev)
    digest = eng.p384_sha384(msgs)
    pub, ok = eng.p384_pubkey(d); assert int(ok.sum()) == small
    sig, ok = eng.p384_ecdsa_sign(d, digest); assert int(ok.sum()) == small
    peer = torch.roll(pub, 1, 0)
    D, M, H, Q, S, PEER = (tile(t, n) for t in (d, msgs, digest, pub, sig, peer))
    assert int(eng.p384_ecdsa_verify(Q, H, S).sum()) == n, "the timed batch does not verify"
    # the yardsticks' batches
    d256 = torch.randint(1, 2**62, (n, 4), dtype=torch.int64, device=eng.tdev)
    e256 = torch.randint(1, 2**62, (n, 4), dtype=torch.int64, device=eng.tdev)
    qx, qy = eng.scalar_mult_base(P256, d256, flags=2)
    r256, s256, _, ok = eng.ecdsa_sign_deterministic(P256, e256, d256); assert int(ok.sum()) == n
    assert int(eng.ecdsa_verify(P256, e256, r256, s256, qx, qy).sum()) == n
    seeds = torch.randint(0, 256, (small, 32), dtype=torch.uint8, device=eng.tdev)
    esig, epk = eng.ed25519_sign(seeds, msgs)
    ES, EPK = tile(esig, n), tile(epk, n)

    def yardsticks(tag):
        report("p256_ecdsa_verify" + tag, lambda: eng.ecdsa_verify(P256, e256, r256, s256, qx, qy), n)
        report("ed25519_verify_64B" + tag, lambda: eng.ed25519_verify(EPK, M, ES), n)

    yardsticks("")
    report("p384_ecdsa_verify", lambda: eng.p384_ecdsa_verify(Q, H, S), n)
    report("p384_ecdh", lambda: eng.p384_ecdh(D, PEER), n)
    report("p384_ecdsa_sign", lambda: eng.p384_ecdsa_sign(D, H), n)
    report("p384_pubkey", lambda: eng.p384_pubkey(D), n)
    report("p384_sha384_64B", lambda: eng.p384_sha384(M), n)
    yardsticks(" (again)")
    for y in ("p256_ecdsa_verify", "ed25519_verify_64B"):
        say(f"p384_ecdsa_verify / {y}, rate: {rate['p384_ecdsa_verify'] / rate[y]:.4f}  (against the second pass: {rate['p384_ecdsa_verify'] / rate[y + ' (again)']:.4f})")
    listing = os.path.join(ROOT, "profiles", "r18", "p384_listing.json")
    if os.path.exists(listing):
        J = json.load(open(listing))
        valu = J["verify_valu_per_lane"]
        say(f"VALU instructions issued per second by p384_ecdsa_verify: {valu * rate['p384_ecdsa_verify'] * 1e-6:.2f} T ({valu} per verification and "
            f"{J['verify_mads_per_lane']} v_mad_u64_u32 from the listing)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
