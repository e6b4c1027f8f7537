"""Times bip39_seed on one MI355X next to its yardsticks, in one process and run:

    python tools/time_bip39.py [--lanes 1048576] [--reps 5]

HIP events on the engine's stream (torch's current stream), two warm-up calls, then `reps` repetitions: the median, with the fastest and the slowest in
brackets.  bip39_seed (24-word sentences of 160 bytes, one passphrase for the call) stands beside bip32_master at 64-byte seeds and sha512 at 128-byte
messages: all three are the same SHA-512 compression, so the time per compression is what compares -- 2 x 2047 + 6 per seed (the sentence is hashed in two
blocks, two key blocks, one salt block, the outer block of U_1, two per further iteration), 2 per master key, 2 per 128-byte message.  Beside the measured
ratio to bip32_master stands the one the listings' VALU counts predict (profiles/r11/bip39_listing.json for the loop, profiles/r10/bip32_listing.json for the yardstick).
Also timed: ONE launch at the call's lane chunk (the figure beside the slice and chunk constants in capi.hip and DESIGN.md section 4d) and one slice of
ECSIMD_HIP_PBKDF2_SLICE iterations at 65 lanes.
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
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from ecsimd_amd import Engine
    eng = Engine(0)
    n = a.lanes
    hdr = open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read()
    capi = open(os.path.join(ROOT, "ecsimd_amd", "csrc", "capi.hip")).read()
    slice_ = int(re.search(r"ECSIMD_HIP_PBKDF2_SLICE\s*=\s*(\d+)", hdr).group(1))
    chunk = 1 << int(re.search(r"PBKDF2_UNITS = \(size_t\)1 << (\d+);", capi).group(1))
    words = torch.randint(97, 123, (n, 160), dtype=torch.uint8, device=eng.tdev)
    phrase = torch.randint(97, 123, (12,), dtype=torch.uint8, device=eng.tdev)
    msgs = torch.randint(0, 256, (n, 128), dtype=torch.uint8, device=eng.tdev)
    seeds = torch.randint(0, 256, (n, 64), dtype=torch.uint8, device=eng.tdev)

    def timed(fn):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record(); t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return statistics.median(ms), min(ms), max(ms)

    # (name, call, lanes, compressions per lane)
    calls = [("sha512_128", lambda: eng.sha512(msgs), n, 2), ("bip32_master_64", lambda: eng.bip32_master(seeds), n, 2),
             ("bip39_seed", lambda: eng.bip39_seed(words, phrase), n, 2 * 2047 + 6),
             ("bip39_seed_one_launch", lambda: eng.bip39_seed(words[:chunk], phrase), min(n, chunk), 2 * 2047 + 6),
             ("pbkdf2_one_slice_65_lanes", lambda: eng.pbkdf2_hmac_sha512(words[:65], phrase, slice_, 64), 65, 2 * (slice_ - 1) + 6)]
    per = {}
    for name, fn, lanes, comp in calls:
        ms, lo, hi = timed(fn)
        per[name] = ms * 1e6 / (lanes * comp)                   # ns per lane and compression
        print(f"{name:28s} {ms:10.3f} ms [{lo:.3f} .. {hi:.3f}]  {lanes / ms / 1e3:10.3f} M/s  {per[name] * 1e3:9.3f} ps per lane and compression  "
              f"({lanes} lanes, {comp} compressions each, median of {a.reps})", flush=True)
    L32 = json.load(open(os.path.join(ROOT, "profiles", "r10", "bip32_listing.json")))
    L39 = json.load(open(os.path.join(ROOT, "profiles", "r11", "bip39_listing.json")))
    loop = L39["loop_valu"] / 2
    for x, y, p, how in (("bip39_seed", "bip32_master_64", loop / (L32["master_valu"] / 2), "half the loop body's VALU count against half of k_bip32_master's"),
                         ("bip39_seed", "sha512_128", None, "no prediction: k_sha512's text is a block loop and a padded tail, its static count is not its work")):
        print(f"{x} / {y}, time per compression = {per[x] / per[y]:.3f}   " + (f"(predicted {p:.3f}: {how})" if p is not None else f"({how})"))
    print(f"VALU instructions issued per second by bip39_seed's loop: {loop / per['bip39_seed'] * 1e-3:.1f} T ({loop:.0f} per compression)")


if __name__ == "__main__":
    main()
