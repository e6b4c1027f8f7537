"""Times the per-lane lengths, the Merkle roots and the Taproot path walk on one MI355X next to their yardsticks, in one process and run:

    python tools/time_btc_tree.py [--lanes 4194304] [--reps 9]

HIP events on the engine's stream (torch's current stream), two warm-up calls, then `reps` repetitions: the median, with the fastest and the slowest in
brackets, as tools/time_btc.py.  Yardsticks: sha256d at 128 bytes for sha256d with every length equal to 128 (what the per-lane loop and the masked tail cost
where nothing diverges), sha256d at 64-byte messages for a Merkle parent (the same three compressions, the padding block's schedule not folded).  The Merkle
call hashes one tree of 2 x lanes leaves: lanes parents on the first level, 2 x lanes - 1 in all.  taproot_merkle_path walks depth 8: 16 compressions a lane.
Prints one line per call and the ratios; profiles/r12/btc_tree.txt keeps the output.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    import torch
    from ecsimd_amd import Engine
    eng = Engine(0)
    n = a.lanes
    msgs = {b: torch.randint(0, 256, (n, b), dtype=torch.uint8, device=eng.tdev) for b in (64, 128)}
    lens128 = torch.full((n,), 128, dtype=torch.int32, device=eng.tdev)
    mixed = torch.randint(0, 129, (n,), dtype=torch.int32, device=eng.tdev)
    leaves = eng.fill_random(2 * n, 9, 1)
    leaf = eng.fill_random(n, 10, 1)
    depth = 8
    path = torch.randint(0, 256, (n, 32 * depth), dtype=torch.uint8, device=eng.tdev)

    def timed(fn):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record(); t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return statistics.median(ms), min(ms), max(ms)

    # (name, call, items per call)
    calls = [("sha256d_128", lambda: eng.sha256d(msgs[128]), n), ("sha256d_lens_all_128", lambda: eng.sha256d(msgs[128], lens128), n),
             ("sha256d_lens_0_to_128", lambda: eng.sha256d(msgs[128], mixed), n), ("sha256d_64", lambda: eng.sha256d(msgs[64]), n),
             ("btc_merkle_root_parents", lambda: eng.btc_merkle_root(leaves, [2 * n]), 2 * n - 1),
             ("tapleaf_hash_128", lambda: eng.tapleaf_hash(msgs[128]), n), (f"taproot_merkle_path_depth_{depth}", lambda: eng.taproot_merkle_path(leaf, path, depth), n)]
    rate = {}
    for name, fn, items in calls:
        ms, lo, hi = timed(fn)
        rate[name] = items / ms / 1e3
        print(f"{name:30s} {ms:9.3f} ms [{lo:.3f} .. {hi:.3f}]  {rate[name]:9.1f} M/s  ({items} items, median of {a.reps})", flush=True)
    ratio = lambda x, y: print(f"{x} / {y} = {rate[x] / rate[y]:.3f}")
    ratio("sha256d_lens_all_128", "sha256d_128")
    ratio("btc_merkle_root_parents", "sha256d_64")
    print(f"taproot_merkle_path: {rate[f'taproot_merkle_path_depth_{depth}'] * 2 * depth:.1f} M compressions/s")


if __name__ == "__main__":
    main()
