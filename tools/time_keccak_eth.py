"""Times keccak256, eth_address and eth_recover on one MI355X next to their yardsticks, in one process and run:

    python tools/time_keccak_eth.py [--lanes 4194304] [--msg-bytes 128] [--reps 11]

HIP events on the engine's stream (torch's current stream), two warm-up calls, the median of `reps` repetitions.  Yardsticks: sha256 at the same message
length for keccak256, ecdsa_recover on secp256k1 for eth_recover.  Prints one line per call and the two ratios; profiles/r08/keccak_eth.txt keeps the output.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1 << 22)
    ap.add_argument("--msg-bytes", type=int, default=128)
    ap.add_argument("--reps", type=int, default=11)
    a = ap.parse_args()
    import torch
    from ecsimd_amd import Engine, SECP256K1
    eng = Engine(0)
    n = a.lanes
    msgs = torch.randint(0, 256, (n, a.msg_bytes), dtype=torch.uint8, device=eng.tdev)
    d = eng.fill_random(n, 7, 1, clear_top_bits=1)
    e = eng.keccak256(msgs)
    sign = 1 << 20                                             # signing keeps 290 B per lane of secrets in the workspace: in slices
    parts = [eng.ecdsa_sign_deterministic(SECP256K1, e[i:i + sign], d[i:i + sign], low_s=True) for i in range(0, n, sign)]
    r, s, v, ok = (torch.cat([p[j] for p in parts]) for j in range(4))
    assert bool(ok.all())
    qx, qy, rok = eng.ecdsa_recover(SECP256K1, e, r, s, v)
    assert bool(rok.all())

    def timed(fn):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record(); t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return statistics.median(ms)

    calls = [("sha256", lambda: eng.sha256(msgs)), ("keccak256", lambda: eng.keccak256(msgs)), ("eth_address", lambda: eng.eth_address(qx, qy)),
             ("ecdsa_recover", lambda: eng.ecdsa_recover(SECP256K1, e, r, s, v)), ("eth_recover", lambda: eng.eth_recover(e, r, s, v)),
             ("eth_recover_low_s_key", lambda: eng.eth_recover(e, r, s, v, require_low_s=True, want_key=True))]
    rate = {}
    for name, fn in calls:
        ms = timed(fn)
        rate[name] = n / ms / 1e3
        print(f"{name:24s} {ms:9.3f} ms  {rate[name]:9.1f} M/s  ({n} lanes, {a.msg_bytes}-byte messages, median of {a.reps})", flush=True)
    print(f"keccak256 / sha256        = {rate['keccak256'] / rate['sha256']:.3f}")
    print(f"eth_recover / ecdsa_recover = {rate['eth_recover'] / rate['ecdsa_recover']:.3f}")


if __name__ == "__main__":
    main()
