"""Times the X25519 calls on one MI355X next to their yardsticks, in one process and run:

    python tools/time_x25519.py [--lanes 1048576] [--big 4194304] [--reps 5] [--out profiles/r14/x25519.txt]

HIP events on the engine's stream (torch's current stream), two warm-up calls, then `reps` repetitions: the median, with the fastest and the slowest in
brackets.  x25519 at `lanes` and `big` lanes; x25519 on u = 9, x25519_base and both conversions at `lanes`; ONE chunk's launch of x25519 alone (X25519_CHUNK in
capi.hip), the longest single launch of the feature, to hold against the 109.7 ms DESIGN.md section 4d accepted for a launch on a shared device.  Beside them,
in the same run: ed25519_verify (64-byte messages), ed25519_pubkey (the comb x25519_base uses) and the P-256 x-only ladder.  The in-run ratios are what the
README quotes.  The a-priori figure beside the measured rate: the VALU instructions per call that profiles/r14/x25519_listing.json derives from the shipped
listing (tools/x25519_listing.py).  Prints one line per call and the ratios, and writes the same text to --out.
"""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P256_G = (0x6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296, 0x4fe342e2fe1a7f9b8ee7eb4a7c0f9e162bce33576b315ececbb6406837bf51f5)
LAUNCH_LIMIT_MS = 109.7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1 << 20)
    ap.add_argument("--big", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "x25519.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from ecsimd_amd import Engine, P256
    eng = Engine(0)
    n = a.lanes
    capi = open(os.path.join(ROOT, "ecsimd_amd", "csrc", "capi.hip")).read()
    chunk = 1 << int(re.search(r"X25519_CHUNK = \(size_t\)1 << (\d+);", capi).group(1))
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

    rate, took = {}, {}

    def report(name, fn, lanes):
        ms, lo, hi = timed(fn)
        rate[name], took[name] = lanes / ms / 1e3, ms
        say(f"{name:34s} {ms:10.3f} ms [{lo:.3f} .. {hi:.3f}]  {rate[name]:10.3f} M/s  ({lanes} lanes, median of {a.reps})")
        return ms

    say(f"device: {torch.cuda.get_device_name(0)}; X25519_CHUNK = 2^{chunk.bit_length() - 1} lanes per launch")
    rnd = lambda lanes, width=32: torch.randint(0, 256, (lanes, width), dtype=torch.uint8, device=eng.tdev)
    k, u = rnd(a.big), rnd(a.big)
    nine = torch.zeros((n, 32), dtype=torch.uint8, device=eng.tdev); nine[:, 0] = 9
    report(f"x25519_2^{n.bit_length() - 1}", lambda: eng.x25519(k[:n], u[:n]), n)
    report(f"x25519_2^{a.big.bit_length() - 1}", lambda: eng.x25519(k, u), a.big)
    report("x25519_with_ok", lambda: eng.x25519(k[:n], u[:n], want_ok=True), n)
    report("x25519_on_u_9", lambda: eng.x25519(k[:n], nine), n)
    report("x25519_base", lambda: eng.x25519_base(k[:n]), n)
    assert torch.equal(eng.x25519_base(k[:n]), eng.x25519(k[:n], nine)), "the two routes to a public key disagree"
    one = min(n, chunk)
    ms_chunk = report("x25519_one_chunk", lambda: eng.x25519(k[:one], u[:one]), one)
    say(f"  one launch of the ladder over a whole chunk: {ms_chunk:.3f} ms against the {LAUNCH_LIMIT_MS} ms limit of DESIGN.md section 4d: "
        + ("within it" if ms_chunk <= LAUNCH_LIMIT_MS else "ABOVE it -- halve X25519_CHUNK"))
    report("x25519_from_ed25519_seed", lambda: eng.x25519_from_ed25519_seed(k[:n]), n)
    pk = eng.ed25519_pubkey(k[:n])
    report("x25519_from_ed25519_pk", lambda: eng.x25519_from_ed25519_pk(pk), n)
    # the yardsticks
    report("ed25519_pubkey", lambda: eng.ed25519_pubkey(k[:n]), n)
    tile = 1 << 12
    msgs = rnd(tile, 64)
    sig, tpk = eng.ed25519_sign(k[:tile].contiguous(), msgs)
    reps = (n + tile - 1) // tile
    vm, vs, vp = (t.repeat(reps, 1)[:n].contiguous() for t in (msgs, sig, tpk))
    assert int(eng.ed25519_verify(vp, vm, vs).sum()) == n, "the timed batch does not verify"
    report("ed25519_verify_64B", lambda: eng.ed25519_verify(vp, vm, vs), n)
    del vm, vs, vp
    limbs = lambda v: [(v >> (64 * j)) & (2**64 - 1) for j in range(4)]
    gx, gy = (eng.to_device(np.tile(np.array(limbs(c), dtype=np.uint64), (n, 1))) for c in P256_G)
    s = torch.randint(1, 2**62, (n, 4), dtype=torch.int64, device=eng.tdev)
    bx, by = eng.scalar_mult(P256, s, gx, gy, flags=2)                       # lane-distinct affine base points
    kk = torch.randint(1, 2**62, (n, 4), dtype=torch.int64, device=eng.tdev)
    report("p256_ladder_x_only", lambda: eng.scalar_mult(P256, kk, bx, by, flags=2, x_only=True), n)
    name = f"x25519_2^{n.bit_length() - 1}"
    say(f"x25519 / p256 x-only ladder, rate: {rate[name] / rate['p256_ladder_x_only']:.3f}")
    say(f"x25519 / ed25519_verify (64 B), rate: {rate[name] / rate['ed25519_verify_64B']:.3f}")
    say(f"x25519_base / x25519 on u = 9, rate: {rate['x25519_base'] / rate['x25519_on_u_9']:.3f}  "
        + ("(the comb route is faster: it stays)" if rate["x25519_base"] > rate["x25519_on_u_9"] else "(the comb route is NOT faster: delete it)"))
    say(f"x25519_base / ed25519_pubkey, rate: {rate['x25519_base'] / rate['ed25519_pubkey']:.3f}")
    listing = os.path.join(ROOT, "profiles", "r14", "x25519_listing.json")
    if os.path.exists(listing):
        J = json.load(open(listing))
        valu = J["x25519_valu_per_lane"]
        say(f"VALU lane-instructions issued per second by x25519: {valu * rate[name] * 1e-6:.1f} T ({valu} per call from the listing, "
            f"{J['ladder_step']['valu']} per ladder step)")
        say(f"  a-priori from the listing: x25519_base / x25519 = {valu / J['x25519_base_valu_per_lane']:.2f} in rate; measured {rate['x25519_base'] / rate['x25519_on_u_9']:.2f}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
