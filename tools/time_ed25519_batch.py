"""Times ecsimd_ed25519_verify_batch's two routes against each other, and against plain ecsimd_ed25519_verify, on one MI355X, in one process and run:

    python tools/time_ed25519_batch.py [--sizes 65536,262144,...] [--reps 5] [--out profiles/r17/ed25519_batch.txt]

tools/time_schnorr_batch.py's protocol.  HIP events on the engine's stream (torch's current stream).  Per size n: two warm-up calls of each of the three -- the
MSM route, the LANES route, ed25519_verify --, then `reps` rounds that ALTERNATE them -- MSM, LANES, verify, MSM, LANES, verify, ... -- so that clock and
temperature drift falls on all alike; the median of each, with the fastest and the slowest repeat in brackets: that bracket is the spread the comparison is held
to.  Sizes 2^16, 2^18, 2^20, 2^21, 2^22, 2^23 and 2^24 - 1 (the largest batch of one call).  Valid signatures over 32-byte messages, made on the device by
ed25519_sign; all three must accept every one of them (or the run stops).  At the end: the threshold the header's rule gives -- the smallest timed n from which,
there and at every larger timed size, the MSM route's slowest repeat is below the LANES route's fastest; none: above ECSIMD_MSM_MAX_N -- beside the
ECSIMD_ED25519_BATCH_AUTO_THRESHOLD the library ships.  Prints one line per measurement and writes the same text to --out.
"""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MSM, LANES, VERIFY = 2, 4, "ed25519_verify"
DEFAULT_SIZES = [1 << 16, 1 << 18, 1 << 20, 1 << 21, 1 << 22, 1 << 23, (1 << 24) - 1]


def shipped_threshold():
    text = open(os.path.join(ROOT, "include", "ecsimd_ed25519_batch.h")).read()
    return re.search(r"#define ECSIMD_ED25519_BATCH_AUTO_THRESHOLD\s+(.*)", text).group(1).strip()


def size_name(u):
    return f"2^{u.bit_length() - 1}" if u & (u - 1) == 0 else f"2^{u.bit_length()} - {(1 << u.bit_length()) - u}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(str(u) for u in DEFAULT_SIZES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "ed25519_batch.txt"))
    a = ap.parse_args()
    import torch
    from ecsimd_amd import Engine
    eng = Engine(0)
    sizes = sorted(int(s) for s in a.sizes.split(","))
    top = max(sizes)
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

    say(f"device: {torch.cuda.get_device_name(0)}; ECSIMD_ED25519_BATCH_AUTO_THRESHOLD as shipped = {shipped_threshold()}; "
        f"{a.reps} alternating repeats after 2 warm-up calls per route; 32-byte messages")
    seeds = torch.randint(0, 256, (top, 32), dtype=torch.uint8, device=eng.tdev)
    msgs = torch.randint(0, 256, (top, 32), dtype=torch.uint8, device=eng.tdev)
    sig, pk = eng.ed25519_sign(seeds, msgs)
    del seeds
    torch.cuda.synchronize()
    faster_from = None
    for u in sizes:
        pu, mu, su = pk[:u], msgs[:u], sig[:u]
        run = {MSM: lambda: eng.ed25519_verify_batch(pu, mu, su, flags=MSM), LANES: lambda: eng.ed25519_verify_batch(pu, mu, su, flags=LANES),
               VERIFY: lambda: eng.ed25519_verify(pu, mu, su)}
        for fn in run.values():
            for _ in range(2):
                fn()
        ms, out = {k: [] for k in run}, {}
        for _ in range(a.reps):
            for k in run:
                t, out[k] = once(run[k])
                ms[k].append(t)
        assert int(out[MSM][0]) == 1 and int(out[LANES][0]) == 1 and bool(out[VERIFY].all()), f"a route refused a valid batch at n = {u}"
        m, l, v = stats(ms[MSM]), stats(ms[LANES]), stats(ms[VERIFY])
        plan = eng.ed25519_batch_plan(u, 32, MSM)
        clear = m[2] < l[1] or l[2] < m[1]
        say(f"n {size_name(u):9s} MSM {m[0]:9.3f} ms [{m[1]:.3f} .. {m[2]:.3f}] {u / m[0] / 1e3:8.3f} M sig/s   LANES {l[0]:9.3f} ms [{l[1]:.3f} .. {l[2]:.3f}] "
            f"{u / l[0] / 1e3:8.3f} M sig/s   ed25519_verify {v[0]:9.3f} ms [{v[1]:.3f} .. {v[2]:.3f}] {u / v[0] / 1e3:8.3f} M sig/s   LANES / MSM {l[0] / m[0]:5.2f}"
            f"{'' if clear else ' (inside the repeat spread)'}   ed25519_verify / MSM {v[0] / m[0]:5.2f}   LANES / ed25519_verify {l[0] / v[0]:6.3f}   "
            f"MSM launches {plan['launches']} workspace {plan['workspace_bytes'] / 2**20:.0f} MiB")
        if m[2] < l[1]:
            faster_from = u if faster_from is None else faster_from
        else:
            faster_from = None
    if faster_from is None:
        say("threshold by the header's rule: none -- the MSM route's slowest repeat was not below the LANES route's fastest at the largest size timed: "
            "above ECSIMD_MSM_MAX_N, AUTO is always LANES")
    else:
        say(f"threshold by the header's rule: n = {size_name(faster_from)} = {faster_from}: from there on, at every size timed, the MSM route's slowest repeat is below the LANES route's fastest")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
