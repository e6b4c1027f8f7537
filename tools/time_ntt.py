"""Times the number-theoretic transform over BLS12-381's scalar field on one MI355X against its two floors, in one process and run:

    python tools/time_ntt.py [--sizes 12,16,20,22,24] [--reps 5] [--out profiles/r24/ntt.txt]

HIP events on the engine's stream (torch's current stream).  Per size: two warm-up calls of each of the four things timed, then `reps` rounds that ALTERNATE
them -- forward, inverse, copy, product, forward, ... -- so that clock and temperature drift falls on all alike; the median, with the fastest and the slowest in
brackets.  Sizes: n = 2^12 .. 2^24 with one array, and 2^12 with a batch of 2^8.  At the same byte counts, in the same run:
  * ecsimd_hip_memcpy_d2d of one array (batch arrays): a pass reads and writes every element once, so the MEMORY floor of a transform is passes x that copy;
  * ecsimd_hip_mgry_mul of as many elements on the same field: with (n / 2) log2 n butterfly products per array, the ARITHMETIC floor is that many products at the
    per-product time of mgry_mul -- itself read beside peak_mad32's rate, at 128 multiply-adds a product (64 for the product, 64 for the reduction).
The line says which floor is the higher one -- the roof the transform sits under at that size -- and how far above it the transform is.  inverse(forward(x)) is
compared with x at every size (or the run stops).  Prints one line per measurement and writes the same text to --out.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MADS_PER_PRODUCT = 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="12,16,20,22,24")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "ntt.txt"))
    a = ap.parse_args()
    import ctypes as C
    import torch
    from ecsimd_amd import Engine, BLS12_381_FR_ROOT
    eng = Engine(0)
    field, root = Engine.ntt_bls12_381_fr()
    assert root == BLS12_381_FR_ROOT
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

    mads, ms = eng.peak_mad32()
    peak = mads / ms / 1e9                                                    # 10^12 multiply-adds per second
    say(f"device: {torch.cuda.get_device_name(0)}; peak_mad32 {peak:.2f} T mad32/s; {a.reps} alternating repeats after 2 warm-up calls; field Fr, root 7^((r - 1) / 2^32)")
    cases = [(int(s), 1) for s in a.sizes.split(",")] + [(12, 256)]
    for log_n, batch in cases:
        n = 1 << log_n
        total = n * batch
        plan = Engine.ntt_plan(log_n, batch)
        dom = eng.ntt_domain(field, log_n, root)
        x = torch.randint(0, 2**62, (total, 4), dtype=torch.int64, device=eng.tdev)          # below 2^254 < r
        y, z, w = eng.empty(total), eng.empty(total), eng.empty(total)

        def copy():
            eng._bind_stream()
            eng._check(eng.lib.ecsimd_hip_memcpy_d2d(eng.ctx, C.c_void_p(w.data_ptr()), C.c_void_p(x.data_ptr()), C.c_size_t(total * 32)), "memcpy_d2d")

        run = {"forward": lambda: eng.ntt_forward(dom, x, out=y), "inverse": lambda: eng.ntt_inverse(dom, y, out=z), "copy": copy,
               "mgry_mul": lambda: eng.mgry_mul(field, x, y)}
        for fn in run.values():
            for _ in range(2):
                fn()
        t = {k: [] for k in run}
        for _ in range(a.reps):
            for k, fn in run.items():
                t[k].append(once(fn)[0])
        torch.cuda.synchronize()
        assert torch.equal(z, x), f"inverse(forward(x)) != x at log_n = {log_n}, batch = {batch}"
        f, i, c, m = (stats(t[k]) for k in ("forward", "inverse", "copy", "mgry_mul"))
        products = batch * (n // 2) * log_n
        mem_floor, arith_floor = plan["passes"] * c[0], products * (m[0] / total)
        peak_floor = products * MADS_PER_PRODUCT / (peak * 1e9)                # ms
        roof, name = max((mem_floor, "memory"), (arith_floor, "arithmetic"))
        say(f"log_n {log_n:2d} batch {batch:3d} passes {plan['passes']} ({'+'.join(map(str, plan['log_radix'][:plan['passes']]))})  "
            f"forward {f[0]:9.4f} ms [{f[1]:.4f} .. {f[2]:.4f}]  inverse {i[0]:9.4f} ms [{i[1]:.4f} .. {i[2]:.4f}]  "
            f"copy {c[0]:8.4f} ms [{c[1]:.4f} .. {c[2]:.4f}] ({2 * total * 32 / c[0] / 1e9:.2f} TB/s)  mgry_mul {m[0]:8.4f} ms [{m[1]:.4f} .. {m[2]:.4f}]  "
            f"memory floor {mem_floor:8.4f} ms (forward / floor {f[0] / mem_floor:5.2f})  arithmetic floor {arith_floor:8.4f} ms (forward / floor {f[0] / arith_floor:5.2f}; "
            f"at peak_mad32 and {MADS_PER_PRODUCT} mads a product {peak_floor:.4f} ms)  roof: {name}, forward / roof {f[0] / roof:5.2f}  {total / f[0] / 1e6:7.3f} G elements/s")
        dom.close()
        del x, y, z, w
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
