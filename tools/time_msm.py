"""Times ecsimd_msm's two routes against each other on one MI355X, in one process and run:

    python tools/time_msm.py [--sizes 12,14,16,18,20,22] [--reps 5] [--out profiles/r15/msm.txt]

HIP events on the engine's stream (torch's current stream).  Per (curve, bits, n): two warm-up calls of each route, then `reps` rounds that ALTERNATE the
routes -- BUCKETS, LANES, BUCKETS, LANES, ... -- so that clock and temperature drift falls on both alike; the median per route, with the fastest and the
slowest in brackets: that bracket is the repeat spread the comparison is held to.  LANES is what a caller could do before this entry point existed (per-lane
ecsimd_hip_scalar_mult with ALG_WINDOWED) plus a reduction.  n = 2^12 .. 2^22, bits 256 and 128, both curves; point_sum at 2^20.  The two routes' results are
compared at every size (the same affine bytes, or the run stops).  Random 256-bit scalars and lane-distinct points P_i = s_i G.  At the end: the measured
crossover per (curve, bits), beside the ECSIMD_MSM_AUTO_THRESHOLD the library ships, and the ratio at n = 2^20, bits = 256 that the README quotes.
Prints one line per measurement and writes the same text to --out.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BUCKETS, LANES = 1, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="12,14,16,18,20,22")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "msm.txt"))
    a = ap.parse_args()
    import torch
    from ecsimd_amd import Engine, P256, SECP256K1
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import msm_model
    eng = Engine(0)
    sizes = [1 << int(s) for s in a.sizes.split(",")]
    top = max(sizes + [1 << 20])
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def once(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(); out = fn(); t1.record(); t1.synchronize()
        return t0.elapsed_time(t1), out

    def stats(ms):
        return statistics.median(ms), min(ms), max(ms)

    say(f"device: {torch.cuda.get_device_name(0)}; ECSIMD_MSM_AUTO_THRESHOLD as shipped = {msm_model.AUTO_THRESHOLD}; {a.reps} alternating repeats after 2 warm-up calls per route")
    faster_from = {}
    for cv, name in ((P256, "p256"), (SECP256K1, "secp256k1")):
        s = torch.randint(-2**63, 2**63 - 1, (top, 4), dtype=torch.int64, device=eng.tdev)
        x, y = eng.scalar_mult_base(cv, s, flags=2 | 8)                      # lane-distinct affine points s_i G
        k = torch.randint(-2**63, 2**63 - 1, (top, 4), dtype=torch.int64, device=eng.tdev)
        torch.cuda.synchronize()
        for bits in (256, 128):
            for n in sizes:
                kn, xn, yn = k[:n], x[:n], y[:n]
                run = {alg: (lambda alg=alg: eng.msm(cv, kn, xn, yn, bits=bits, alg=alg)) for alg in (BUCKETS, LANES)}
                for alg in run:
                    for _ in range(2):
                        run[alg]()
                ms, out = {BUCKETS: [], LANES: []}, {}
                for _ in range(a.reps):
                    for alg in (BUCKETS, LANES):
                        t, out[alg] = once(run[alg])
                        ms[alg].append(t)
                assert all(torch.equal(p, q) for p, q in zip(out[BUCKETS], out[LANES])), f"the routes disagree at {name}, bits = {bits}, n = {n}"
                assert int(out[BUCKETS][2][0]) == 1
                b, l = stats(ms[BUCKETS]), stats(ms[LANES])
                plan = eng.msm_plan(n, bits, BUCKETS)
                clear = b[2] < l[1] or l[2] < b[1]                              # the slowest of one is below the fastest of the other
                say(f"{name:10s} bits {bits:3d} n 2^{n.bit_length() - 1:<2d} BUCKETS {b[0]:9.3f} ms [{b[1]:.3f} .. {b[2]:.3f}] {n / b[0] / 1e3:8.3f} M terms/s   "
                    f"LANES {l[0]:9.3f} ms [{l[1]:.3f} .. {l[2]:.3f}] {n / l[0] / 1e3:8.3f} M terms/s   LANES / BUCKETS {l[0] / b[0]:6.2f}"
                    f"{'' if clear else '  (inside the repeat spread)'}   c {plan['c']} windows {plan['windows']} L {plan['L']} m {plan['m']} launches {plan['launches']}")
                if b[2] < l[1]:
                    faster_from.setdefault((name, bits), n)
                else:
                    faster_from.pop((name, bits), None)
                if bits == 256 and n == 1 << 20:
                    say(f"  the bar at n = 2^20, bits = 256 on {name}: BUCKETS' slowest repeat {b[2]:.3f} ms against LANES' fastest {l[1]:.3f} ms: "
                        + ("BUCKETS is faster by more than the spread" if b[2] < l[1] else "BUCKETS is NOT faster by more than the spread: AUTO must not choose it"))
        n = 1 << 20
        for _ in range(2):
            eng.point_sum(cv, x[:n], y[:n])
        t = stats([once(lambda: eng.point_sum(cv, x[:n], y[:n]))[0] for _ in range(a.reps)])
        say(f"{name:10s} point_sum n 2^20 {t[0]:9.3f} ms [{t[1]:.3f} .. {t[2]:.3f}] {n / t[0] / 1e3:8.3f} M points/s")
        del s, x, y, k
    for (name, bits), n in sorted(faster_from.items()):
        say(f"crossover {name} bits {bits}: BUCKETS is faster than LANES by more than the spread from n = 2^{n.bit_length() - 1} on (of the sizes timed)")
    for key in sorted({(nm, b) for nm in ("p256", "secp256k1") for b in (256, 128)} - set(faster_from)):
        say(f"crossover {key[0]} bits {key[1]}: BUCKETS was not faster at the largest size timed")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
