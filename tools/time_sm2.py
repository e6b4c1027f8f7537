"""Times the SM2 calls on one MI355X next to their yardsticks, in one process and run:

    python tools/time_sm2.py [--lanes 1048576] [--reps 9] [--out FILE]

HIP events on the engine's stream (torch's current stream).  Every call is warmed up twice (the first builds the curve's window tables), then `reps` rounds go
through ALL the calls in turn -- the calls alternate, so a drift of the device's clock lands on every one of them alike -- and each call's median is reported,
with its fastest and slowest round in brackets.  Timed at `lanes`: sm2_verify (32-byte messages, the default ID), sm2_verify_digest, sm2_sign_digest with the
caller's nonce and with the deterministic one, sm2_pubkey and sm3 at 128 bytes; and, as yardsticks, the parent's code on the SAME registered curve and batch:
ecdsa_verify, ecdsa_sign, and sha256 at 128 bytes.  The in-run ratios are what the README quotes.  --out appends the lines to a file.
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ecsimd_amd import Engine
    eng = Engine(0)
    cv = Engine.sm2_curve()
    n = a.lanes
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    rnd = lambda: torch.randint(1, 2**62, (n, 4), dtype=torch.int64, device=eng.tdev)
    d, k, e0 = rnd(), rnd(), rnd()
    msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=eng.tdev)
    long_msgs = torch.randint(0, 256, (n, 128), dtype=torch.uint8, device=eng.tdev)
    qx, qy, ok = eng.sm2_pubkey(cv, d); assert int(ok.sum()) == n
    e = eng.sm2_digest(cv, qx, qy, msgs)
    r, s, ok = eng.sm2_sign_digest(cv, e, d, k); assert int(ok.sum()) == n
    assert int(eng.sm2_verify(cv, qx, qy, msgs, r, s).sum()) == n and int(eng.sm2_verify_digest(cv, e, r, s, qx, qy).sum()) == n, "the timed batch does not verify"
    er, es, ok = eng.ecdsa_sign(cv, e0, d, k); assert int(ok.sum()) == n
    assert int(eng.ecdsa_verify(cv, e0, er, es, qx, qy).sum()) == n, "the yardstick's batch does not verify"

    calls = [
        ("ecdsa_verify (yardstick)", lambda: eng.ecdsa_verify(cv, e0, er, es, qx, qy)),
        ("sm2_verify_32B", lambda: eng.sm2_verify(cv, qx, qy, msgs, r, s)),
        ("sm2_verify_digest", lambda: eng.sm2_verify_digest(cv, e, r, s, qx, qy)),
        ("ecdsa_sign (yardstick)", lambda: eng.ecdsa_sign(cv, e0, d, k)),
        ("sm2_sign_digest", lambda: eng.sm2_sign_digest(cv, e, d, k)),
        ("sm2_sign_digest_deterministic", lambda: eng.sm2_sign_digest(cv, e, d)),
        ("sm2_pubkey", lambda: eng.sm2_pubkey(cv, d)),
        ("sha256_128B (yardstick)", lambda: eng.sha256(long_msgs)),
        ("sm3_128B", lambda: eng.sm3(long_msgs)),
    ]
    for _, fn in calls:
        fn(); fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in calls}
    for _ in range(a.reps):
        for name, fn in calls:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record(); t1.synchronize()
            ms[name].append(t0.elapsed_time(t1))
    rate = {}
    for name, _ in calls:
        med, lo, hi = statistics.median(ms[name]), min(ms[name]), max(ms[name])
        rate[name] = n / med / 1e3
        say(f"{name:32s} {med:10.3f} ms [{lo:.3f} .. {hi:.3f}, spread {100 * (hi - lo) / med:.1f} %]  {rate[name]:10.3f} M/s  ({n} lanes, median of {a.reps}, calls alternating)")
    for num, den in (("sm2_verify_32B", "ecdsa_verify (yardstick)"), ("sm2_verify_digest", "ecdsa_verify (yardstick)"), ("sm2_sign_digest", "ecdsa_sign (yardstick)"),
                     ("sm2_sign_digest_deterministic", "ecdsa_sign (yardstick)"), ("sm2_pubkey", "ecdsa_sign (yardstick)"), ("sm3_128B", "sha256_128B (yardstick)")):
        say(f"{num} / {den}, rate: {rate[num] / rate[den]:.4f}")
    listing = os.path.join(ROOT, "profiles", "r20", "sm2_listing.json")
    if os.path.exists(listing):
        valu = json.load(open(listing))["valu_per_compression"]
        say(f"VALU instructions issued per second by sm3_128B: {3 * valu * rate['sm3_128B'] * 1e-6:.2f} T (3 compressions of {valu} from the listing)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
