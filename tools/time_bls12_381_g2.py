"""Times BLS12-381 G2 on one MI355X:

    python tools/time_bls12_381_g2.py [--sizes 12,16,17,18,19,20] [--reps 5] [--out profiles/r22/bls12_381_g2.txt]

time_bls12_381.py's twin.  The run is a sequence of STEPS, each a child process of its own under `timeout`; the chain stops at the first step that does not exit
0 (a step that faults, aborts or runs out of time ends the run: nothing more is started on the GPU).  One step per n: ecsimd_bls381_g2_msm on the EXPLICIT routes
BUCKETS and LANES at bits = 255 (AUTO is never timed: it is one of the two), and ecsimd_bls12_381_g1_msm on the same routes at the same n as the yardstick the
prediction is held to (about three times G1 per term on either route); a last step times g2_decompress, g2_compress, g2_check, g2_mul and
g2_point_sum (both encodings) at 2^18.  HIP events on the engine's stream.  Per measurement: two warm-up calls of each route, then `reps` rounds that ALTERNATE
the routes, so that clock and temperature drift falls on both alike; the median, with the fastest and the slowest in brackets: that bracket is the repeat spread
a comparison is held to.  The two routes' results are compared at every size (the same 192 bytes, or the step fails).  Terms: random 256-bit scalars and
lane-distinct points Q_i = s_i G2 made on the device by g2_mul.  At the end: the measured crossover, beside the ECSIMD_BLS381_G2_MSM_AUTO_THRESHOLD the header
ships.  Prints one line per measurement and writes the same text to --out.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BUCKETS, LANES = 1, 2
STEP_SECONDS = 240
LANES_STEP_N = 1 << 18


def shipped_threshold():
    m = re.search(r"#define ECSIMD_BLS381_G2_MSM_AUTO_THRESHOLD \(\(size_t\)1 << (\d+)\)", open(os.path.join(ROOT, "include", "ecsimd_bls12_381_g2.h")).read())
    return 1 << int(m.group(1))


def step(kind, n, reps):
    import torch
    from ecsimd_amd import Engine
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bls12_381_g2_model as model
    import bls12_381_model as g1_model
    eng = Engine(0)

    def once(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(); out = fn(); t1.record(); t1.synchronize()
        return t0.elapsed_time(t1), out

    def stats(ms):
        return statistics.median(ms), min(ms), max(ms)

    def alternate(run):
        for alg in run:
            for _ in range(2):
                run[alg]()
        ms, out = {alg: [] for alg in run}, {}
        for _ in range(reps):
            for alg in run:
                t, out[alg] = once(run[alg])
                ms[alg].append(t)
        return {alg: stats(v) for alg, v in ms.items()}, out

    def line(name, n, t, unit):
        return f"{name:28s} n 2^{n.bit_length() - 1:<2d} {t[0]:10.3f} ms [{t[1]:.3f} .. {t[2]:.3f}] {n / t[0] / 1e3:9.3f} M {unit}/s"

    torch.manual_seed(3812)
    g = torch.tensor(list(model.encode192(model.G)), dtype=torch.uint8, device=eng.tdev).repeat(n, 1)
    s = torch.randint(-2**63, 2**63 - 1, (n, 4), dtype=torch.int64, device=eng.tdev)
    pts, ok = eng.bls12_381_g2_mul(s, g)                                     # lane-distinct points of G2
    k = torch.randint(-2**63, 2**63 - 1, (n, 4), dtype=torch.int64, device=eng.tdev)
    torch.cuda.synchronize()
    assert bool(ok.all())
    if kind == "msm":
        t, out = alternate({alg: (lambda alg=alg: eng.bls12_381_g2_msm(k, pts, bits=255, alg=alg)) for alg in (BUCKETS, LANES)})
        assert torch.equal(out[BUCKETS][0], out[LANES][0]) and int(out[BUCKETS][1][0]) == 1, f"the routes disagree at n = {n}"
        plan = eng.bls12_381_g2_msm_plan(n, 255, BUCKETS)
        b, l = t[BUCKETS], t[LANES]
        clear = b[2] < l[1] or l[2] < b[1]
        print(line("g2_msm bits 255 BUCKETS", n, b, "terms"))
        print(line("g2_msm bits 255 LANES", n, l, "terms"))
        print(f"  LANES / BUCKETS {l[0] / b[0]:7.2f}{'' if clear else '  (inside the repeat spread)'}   c {plan['c']} windows {plan['windows']} L {plan['L']} m {plan['m']} "
              f"launches {plan['launches']} workspace {plan['workspace_bytes']}   VERDICT n={n} {'BUCKETS' if b[2] < l[1] else 'LANES' if l[2] < b[1] else 'SPREAD'}")
        g1 = torch.tensor(list(g1_model.encode96(g1_model.G)), dtype=torch.uint8, device=eng.tdev).repeat(n, 1)
        pts1, ok1 = eng.bls12_381_g1_mul(s, g1)
        t, out = alternate({alg: (lambda alg=alg: eng.bls12_381_g1_msm(k, pts1, bits=255, alg=alg)) for alg in (BUCKETS, LANES)})
        assert torch.equal(out[BUCKETS][0], out[LANES][0])
        print(line("g1_msm bits 255 BUCKETS", n, t[BUCKETS], "terms"))
        print(line("g1_msm bits 255 LANES", n, t[LANES], "terms"))
        print(f"  g2_msm / g1_msm: BUCKETS {b[0] / t[BUCKETS][0]:6.2f}   LANES {l[0] / t[LANES][0]:6.2f}   (predicted before timing: about 3 on both)")
    else:
        comp, ok = eng.bls12_381_g2_compress(pts)
        torch.cuda.synchronize()
        for name, fn, unit in (("g2_decompress", lambda: eng.bls12_381_g2_decompress(comp), "points"), ("g2_compress", lambda: eng.bls12_381_g2_compress(pts), "points"),
                               ("g2_check ([r] Q)", lambda: eng.bls12_381_g2_check(pts), "points"), ("g2_mul", lambda: eng.bls12_381_g2_mul(k, pts), "products"),
                               ("g2_point_sum uncompressed", lambda: eng.bls12_381_g2_point_sum(pts), "points"), ("g2_point_sum compressed", lambda: eng.bls12_381_g2_point_sum(comp), "points")):
            t, out = alternate({0: fn})
            print(line(name, n, t[0], unit))
        back, ok = eng.bls12_381_g2_decompress(comp)
        on, sub = eng.bls12_381_g2_check(pts)
        a, b = eng.bls12_381_g2_point_sum(pts)[0], eng.bls12_381_g2_point_sum(comp)[0]
        assert torch.equal(back, pts) and bool(on.all()) and bool(sub.all()) and torch.equal(a, b)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="12,16,17,18,19,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "bls12_381_g2.txt"))
    ap.add_argument("--step", default=None, help="internal: kind:n")
    a = ap.parse_args()
    if a.step:
        kind, n = a.step.split(":")
        return step(kind, int(n), a.reps)
    lines = [f"ECSIMD_BLS381_G2_MSM_AUTO_THRESHOLD as shipped = {shipped_threshold()}; bits = 255; {a.reps} alternating repeats after 2 warm-up calls per route; "
             f"each step a process of its own under timeout {STEP_SECONDS} s"]
    print(lines[0], flush=True)
    steps = [("msm", 1 << int(s)) for s in a.sizes.split(",")] + [("lanes", LANES_STEP_N)]
    verdicts = {}
    for kind, n in steps:
        r = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", f"{kind}:{n}", "--reps", str(a.reps)],
                           capture_output=True, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        for m in re.finditer(r"VERDICT n=(\d+) (\w+)", r.stdout):
            verdicts[int(m.group(1))] = m.group(2)
        if r.returncode != 0:
            lines.append(f"step {kind}:{n} ended with status {r.returncode}: the run stops here\n{r.stderr[-2000:]}")
            print(lines[-1], flush=True)
            break
    faster = sorted(n for n, v in verdicts.items() if v == "BUCKETS" and all(verdicts[m] == "BUCKETS" for m in verdicts if m >= n))
    lines.append(f"crossover: BUCKETS is faster than LANES by more than the spread from n = {'2^%d' % (faster[0].bit_length() - 1) if faster else '(never, of the sizes timed)'} on "
                 f"(sizes timed: {', '.join('2^%d' % (n.bit_length() - 1) for n in sorted(verdicts))})")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if len(verdicts) == len(steps) - 1 else 1


if __name__ == "__main__":
    sys.exit(main())
