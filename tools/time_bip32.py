"""Times SHA-512 and the BIP-32 calls on one MI355X next to their yardsticks, in one process and run:

    python tools/time_bip32.py [--lanes 4194304] [--reps 9]

HIP events on the engine's stream (torch's current stream), two warm-up calls, then `reps` repetitions: the median, with the fastest and the slowest in
brackets.  Yardsticks: sha256 at 128-byte messages for sha512, taproot_tweak_seckey (key path) for bip32_ckd_priv -- the same constant-time comb and inversion
in front of one SHA-256 compression there, four SHA-512 ones here --, xonly_tweak_add for bip32_ckd_pub (the same chain behind a front kernel that lifts
instead of hashing).  Beside each measured ratio stands the one the listings' VALU counts predict (profiles/r10/bip32_listing.json; all of them counts of
straight-line kernels).  The comb and the inversion have loops, so their static counts are not their work: their share is MEASURED in this run (the
constant-time scalar_mult_base with affine output is exactly those two launches) and a SHA-512 instruction is priced by bip32_master's time; where a
yardstick's own kernel has loops (xonly_tweak_add's square root) the output says that there is no prediction.
Prints one line per call and the ratios.
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
    ap.add_argument("--lanes", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    import torch
    from ecsimd_amd import Engine, SECP256K1
    eng = Engine(0)
    n = a.lanes
    OUT_AFFINE, WINDOWED, WINDOWED_SIGNED, CONSTANT_TIME = 2, 4, 8, 128
    H = 1 << 31
    msgs = torch.randint(0, 256, (n, 128), dtype=torch.uint8, device=eng.tdev)
    seeds = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=eng.tdev)
    key = torch.randint(0, 256, (32,), dtype=torch.uint8, device=eng.tdev)
    d = eng.fill_random(n, 7, 1, clear_top_bits=1)
    c = eng.fill_random(n, 8, 1)
    index = torch.randint(0, 2**31 - 1, (n,), dtype=torch.int32, device=eng.tdev)
    qx, qy = eng.scalar_mult_base(SECP256K1, d, OUT_AFFINE | WINDOWED_SIGNED)[:2]
    px = qx
    part = 1 << 20                                             # the secret calls keep 160 B per lane in the workspace: in slices, as tools/time_btc.py times them

    def sliced(fn):
        def run():
            for i in range(0, n, part):
                fn(slice(i, i + part))
        return run

    def timed(fn):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record(); t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return statistics.median(ms), min(ms), max(ms)

    calls = [("sha256_128", lambda: eng.sha256(msgs)), ("sha512_128", lambda: eng.sha512(msgs)), ("hmac_sha512_128", lambda: eng.hmac_sha512(key, msgs)),
             ("bip32_master_32", lambda: eng.bip32_master(seeds)),
             ("ct_comb_and_inversion", sliced(lambda s: eng.scalar_mult_base(SECP256K1, d[s], OUT_AFFINE | WINDOWED | CONSTANT_TIME))),
             ("taproot_tweak_seckey", sliced(lambda s: eng.taproot_tweak_seckey(d[s], None, want_px=False))),
             ("bip32_ckd_priv", sliced(lambda s: eng.bip32_ckd_priv(d[s], c[s], index[s]))),
             ("bip32_ckd_priv_hardened", sliced(lambda s: eng.bip32_ckd_priv(d[s], c[s], H + 44))),
             ("xonly_tweak_add", lambda: eng.xonly_tweak_add(px, c)),
             ("bip32_ckd_pub", lambda: eng.bip32_ckd_pub(qx, qy, c, index))]
    rate, ms_of = {}, {}
    for name, fn in calls:
        ms, lo, hi = timed(fn)
        rate[name], ms_of[name] = n / ms / 1e3, ms
        print(f"{name:30s} {ms:9.3f} ms [{lo:.3f} .. {hi:.3f}]  {rate[name]:9.1f} M/s  ({n} lanes, median of {a.reps})", flush=True)
    L = json.load(open(os.path.join(ROOT, "profiles", "r10", "bip32_listing.json")))
    per_valu = ms_of["bip32_master_32"] / L["master_valu"]     # what one VALU instruction of straight-line SHA-512 code costs the whole batch, measured
    shared = ms_of["ct_comb_and_inversion"]                    # the two launches in front of k_taproot_seckey and of k_bip32_ckd_priv<1>, measured
    t_seckey = shared + per_valu * L["taproot_seckey_key_path_valu"]
    predicted = {("sha512_128", "sha256_128"): (3 * L["sha256_compression_valu"] / (2 * L["sha512_compression_valu"]), "3 SHA-256 compressions against 2 SHA-512 ones"),
                 ("bip32_ckd_priv_hardened", "bip32_master_32"): (L["master_valu"] / L["ckd_priv_hardened_only_valu"], "the two kernels' VALU counts"),
                 ("bip32_ckd_priv", "taproot_tweak_seckey"): (t_seckey / (shared + per_valu * L["ckd_priv_valu"]),
                                                              "the measured comb and inversion plus each final kernel's VALU count at bip32_master's time per instruction"),
                 ("bip32_ckd_priv_hardened", "taproot_tweak_seckey"): (t_seckey / (per_valu * L["ckd_priv_hardened_only_valu"]), "the same, without comb and inversion on the new side"),
                 ("bip32_ckd_pub", "xonly_tweak_add"): (None, "no prediction: both run the same comb, addition and inversion, and the yardstick's front kernel is a square root in loops, "
                                                              "whose static count is not its work; the new front kernel alone is %d VALU" % L["ckd_pub_front_valu"])}
    for (x, y), (p, how) in predicted.items():
        print(f"{x} / {y} = {rate[x] / rate[y]:.3f}   " + (f"(predicted {p:.3f}: {how})" if p is not None else f"({how})"))


if __name__ == "__main__":
    main()
