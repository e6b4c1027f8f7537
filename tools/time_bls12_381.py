"""Times BLS12-381 G1 or G2 on one MI355X:

    python tools/time_bls12_381.py --group g1|g2 [--sizes 12,16,18,...] [--reps 5] [--out FILE] [--against OTHER_LIBRARY]

The run is a sequence of STEPS, each a child process of its own under `timeout`; the chain stops at the first step that does not exit 0 (a step that faults,
aborts or runs out of time ends the run: nothing more is started on the GPU).  One step per n: the group's msm on the EXPLICIT routes BUCKETS and LANES at
bits = 255 (AUTO is never timed: it is one of the two), and a yardstick at the same n: ecsimd_msm on secp256k1 for G1, ecsimd_bls12_381_g1_msm for G2 (DESIGN.md
4n predicted about three times G1 per term on either route).  A last step times decompress, compress, check, mul and point_sum (both encodings) at 2^20 (G1) or
2^18 (G2).  HIP events on the engine's stream.  Per measurement: two warm-up calls of each route, then `reps` rounds that ALTERNATE the routes, so that clock and
temperature drift falls on both alike; the median, with the fastest and the slowest in brackets: that bracket is the repeat spread a comparison is held to.  The
two routes' results are compared at every size (the same bytes, or the step fails).  Terms: random 256-bit scalars and lane-distinct points s_i G made on the
device by the group's mul.  At the end: the measured crossover, beside the AUTO threshold the header ships.  Prints one line per measurement and writes the same
text to --out (default: profiles/r21/bls12_381.txt, profiles/r22/bls12_381_g2.txt).

--against OTHER_LIBRARY: instead, every call of the group (both msm routes, decompress, compress, check, mul, both point sums) at each size, ALTERNATING this
tree's library and the other build of it (ECSIMD_HIP_LIBRARY's mechanism), the same inputs, the same repeats.  A call PASSES where this library's median is no
later than the other's slowest repeat; the results must be the same bytes.  This is how a change that moves a unit's listing is held to its parent commit.
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
GROUPS = {
    "g1": dict(method="bls12_381_g1", model="bls12_381_model", encode="encode96", seed=381, header="ecsimd_bls12_381.h", threshold="ECSIMD_BLS12_381_MSM_AUTO_THRESHOLD",
               sizes="12,16,18,20,22", lanes_n=1 << 20, point="P", out=os.path.join("profiles", "r21", "bls12_381.txt")),
    "g2": dict(method="bls12_381_g2", model="bls12_381_g2_model", encode="encode192", seed=3812, header="ecsimd_bls12_381_g2.h", threshold="ECSIMD_BLS381_G2_MSM_AUTO_THRESHOLD",
               sizes="12,16,17,18,19,20", lanes_n=1 << 18, point="Q", out=os.path.join("profiles", "r22", "bls12_381_g2.txt")),
}


def shipped_threshold(G):
    m = re.search(r"#define %s \(\(size_t\)1 << (\d+)\)" % G["threshold"], open(os.path.join(ROOT, "include", G["header"])).read())
    return 1 << int(m.group(1))


def step(group, kind, n, reps, against):
    import torch
    from ecsimd_amd import Engine, SECP256K1
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    G = GROUPS[group]
    eng = Engine(0)
    call = lambda e, name: getattr(e, G["method"] + "_" + name)

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

    def terms(group, e):
        """Lane-distinct points of the group, made on the device, and the scalars of the sums."""
        H = GROUPS[group]
        m = __import__(H["model"])
        torch.manual_seed(G["seed"])
        g = torch.tensor(list(getattr(m, H["encode"])(m.G)), dtype=torch.uint8, device=e.tdev).repeat(n, 1)
        s = torch.randint(-2**63, 2**63 - 1, (n, 4), dtype=torch.int64, device=e.tdev)
        pts, ok = getattr(e, H["method"] + "_mul")(s, g)
        k = torch.randint(-2**63, 2**63 - 1, (n, 4), dtype=torch.int64, device=e.tdev)
        torch.cuda.synchronize()
        assert bool(ok.all())
        return s, k, pts

    s, k, pts = terms(group, eng)
    if kind == "against":
        os.environ["ECSIMD_HIP_LIBRARY"] = against
        other = Engine(0)
        del os.environ["ECSIMD_HIP_LIBRARY"]
        comp, ok = call(eng, "compress")(pts)
        torch.cuda.synchronize()
        failed = []
        for name, fn, unit in (("msm BUCKETS", lambda e: call(e, "msm")(k, pts, bits=255, alg=BUCKETS), "terms"), ("msm LANES", lambda e: call(e, "msm")(k, pts, bits=255, alg=LANES), "terms"),
                               ("decompress", lambda e: call(e, "decompress")(comp), "points"), ("compress", lambda e: call(e, "compress")(pts), "points"),
                               ("check", lambda e: call(e, "check")(pts), "points"), ("mul", lambda e: call(e, "mul")(k, pts), "products"),
                               ("point_sum uncompressed", lambda e: call(e, "point_sum")(pts), "points"), ("point_sum compressed", lambda e: call(e, "point_sum")(comp), "points")):
            t, out = alternate({"this": lambda: fn(eng), "other": lambda: fn(other)})
            assert all(torch.equal(a, b) for a, b in zip(out["this"], out["other"])), f"{group}_{name}: the two libraries disagree at n = {n}"
            ok_ = t["this"][0] <= t["other"][2]
            failed += [] if ok_ else [name]
            print(line(f"{group}_{name} this", n, t["this"], unit))
            print(line(f"{group}_{name} other", n, t["other"], unit) + f"   this / other {t['this'][0] / t['other'][0]:6.3f}  {'PASS' if ok_ else 'FAIL'}")
        other.close()
        eng.close()
        return 1 if failed else 0
    if kind == "msm":
        t, out = alternate({alg: (lambda alg=alg: call(eng, "msm")(k, pts, bits=255, alg=alg)) for alg in (BUCKETS, LANES)})
        assert torch.equal(out[BUCKETS][0], out[LANES][0]) and int(out[BUCKETS][1][0]) == 1, f"the routes disagree at n = {n}"
        plan = call(eng, "msm_plan")(n, 255, BUCKETS)
        b, l = t[BUCKETS], t[LANES]
        clear = b[2] < l[1] or l[2] < b[1]
        print(line(f"{group}_msm bits 255 BUCKETS", n, b, "terms"))
        print(line(f"{group}_msm bits 255 LANES", n, l, "terms"))
        print(f"  LANES / BUCKETS {l[0] / b[0]:7.2f}{'' if clear else '  (inside the repeat spread)'}   c {plan['c']} windows {plan['windows']} L {plan['L']} m {plan['m']} "
              f"launches {plan['launches']} workspace {plan['workspace_bytes']}   VERDICT n={n} {'BUCKETS' if b[2] < l[1] else 'LANES' if l[2] < b[1] else 'SPREAD'}")
        if group == "g1":
            x, y = eng.scalar_mult_base(SECP256K1, s, flags=2 | 8)
            t, out = alternate({alg: (lambda alg=alg: eng.msm(SECP256K1, k, x, y, bits=255, alg=alg)) for alg in (BUCKETS, LANES)})
            assert all(torch.equal(p, q) for p, q in zip(out[BUCKETS], out[LANES]))
            print(line("ecsimd_msm secp256k1 BUCKETS", n, t[BUCKETS], "terms"))
            print(line("ecsimd_msm secp256k1 LANES", n, t[LANES], "terms"))
            print(f"  g1_msm BUCKETS / ecsimd_msm secp256k1 BUCKETS {b[0] / t[BUCKETS][0]:6.2f}   LANES / LANES {l[0] / t[LANES][0]:6.2f}")
        else:
            pts1 = terms("g1", eng)[2]
            t, out = alternate({alg: (lambda alg=alg: eng.bls12_381_g1_msm(k, pts1, bits=255, alg=alg)) for alg in (BUCKETS, LANES)})
            assert torch.equal(out[BUCKETS][0], out[LANES][0])
            print(line("g1_msm bits 255 BUCKETS", n, t[BUCKETS], "terms"))
            print(line("g1_msm bits 255 LANES", n, t[LANES], "terms"))
            print(f"  g2_msm / g1_msm: BUCKETS {b[0] / t[BUCKETS][0]:6.2f}   LANES {l[0] / t[LANES][0]:6.2f}   (predicted before timing: about 3 on both)")
    else:
        comp, ok = call(eng, "compress")(pts)
        torch.cuda.synchronize()
        for name, fn, unit in (("decompress", lambda: call(eng, "decompress")(comp), "points"), ("compress", lambda: call(eng, "compress")(pts), "points"),
                               (f"check ([r] {G['point']})", lambda: call(eng, "check")(pts), "points"), ("mul", lambda: call(eng, "mul")(k, pts), "products"),
                               ("point_sum uncompressed", lambda: call(eng, "point_sum")(pts), "points"), ("point_sum compressed", lambda: call(eng, "point_sum")(comp), "points")):
            t, out = alternate({0: fn})
            print(line(f"{group}_{name}", n, t[0], unit))
        back, ok = call(eng, "decompress")(comp)
        on, sub = call(eng, "check")(pts)
        a, b = call(eng, "point_sum")(pts)[0], call(eng, "point_sum")(comp)[0]
        assert torch.equal(back, pts) and bool(on.all()) and bool(sub.all()) and torch.equal(a, b)
    eng.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", choices=sorted(GROUPS), required=True)
    ap.add_argument("--sizes", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--against", default=None, help="another build of the library: time every call of the group against it")
    ap.add_argument("--step", default=None, help="internal: kind:n")
    a = ap.parse_args()
    G = GROUPS[a.group]
    if a.step:
        kind, n = a.step.split(":")
        return step(a.group, kind, int(n), a.reps, a.against)
    lines = [f"{G['threshold']} as shipped = {shipped_threshold(G)}; bits = 255; {a.reps} alternating repeats after 2 warm-up calls per route; "
             f"each step a process of its own under timeout {STEP_SECONDS} s" + (f"; `this` is the tree's library, `other` is {os.path.basename(a.against)}" if a.against else "")]
    print(lines[0], flush=True)
    sizes = [1 << int(s) for s in (a.sizes or G["sizes"]).split(",")]
    steps = [("against", n) for n in sizes] if a.against else [("msm", n) for n in sizes] + [("lanes", G["lanes_n"])]
    verdicts, status = {}, 0
    for kind, n in steps:
        r = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--group", a.group, "--step", f"{kind}:{n}", "--reps", str(a.reps)]
                           + (["--against", os.path.abspath(a.against)] if a.against else []), capture_output=True, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        for m in re.finditer(r"VERDICT n=(\d+) (\w+)", r.stdout):
            verdicts[int(m.group(1))] = m.group(2)
        if r.returncode != 0:
            status = 1
            if r.returncode != 1 or "FAIL" not in r.stdout:
                lines.append(f"step {kind}:{n} ended with status {r.returncode}: the run stops here\n{r.stderr[-2000:]}")
                print(lines[-1], flush=True)
                break
    if not a.against:
        faster = sorted(n for n, v in verdicts.items() if v == "BUCKETS" and all(verdicts[m] == "BUCKETS" for m in verdicts if m >= n))
        lines.append(f"crossover: BUCKETS is faster than LANES by more than the spread from n = {'2^%d' % (faster[0].bit_length() - 1) if faster else '(never, of the sizes timed)'} on "
                     f"(sizes timed: {', '.join('2^%d' % (n.bit_length() - 1) for n in sorted(verdicts))})")
        print(lines[-1], flush=True)
        status = status or (0 if len(verdicts) == len(sizes) else 1)
    out = os.path.join(ROOT, a.out or G["out"])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
