#!/usr/bin/env python3
"""profiles/r17/ed25519_batch_listing.json: VGPRs and scratch bytes of every kernel of k_msm_ed25519.hip, read from the ISA the build leaves beside the object
(build/csrc/k_msm_ed25519-hip-amdgcn-amd-amdhsa-gfx950.s).  Prints the line the unit's head comment carries; tests/test_ed25519_batch_cpu.py compares all three.

  python tools/ed25519_batch_listing.py            writes the file
"""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISA = os.path.join(ROOT, "build", "csrc", "k_msm_ed25519-hip-amdgcn-amd-amdhsa-gfx950.s")
OUT = os.path.join(ROOT, "profiles", "r17", "ed25519_batch_listing.json")


def kernels(text):
    got = {}
    for block in text.split("- .agpr_count:")[1:]:
        name = re.search(r"(k_ed[mbc]_[a-z]+)", re.search(r"\.name:\s+(\S+)", block).group(1)).group(1)
        field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        assert field("vgpr_spill_count") == 0 and field("private_segment_fixed_size") == 0, name
        got[name] = dict(vgprs=field("vgpr_count"), scratch_bytes=field("private_segment_fixed_size"))
    return got


if __name__ == "__main__":
    got = kernels(open(ISA).read())
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(dict(comment="k_msm_ed25519.hip, gfx950, -O3: VGPRs and scratch bytes per kernel; no kernel spills; 256-thread workgroups (64 for the one-lane kernels)",
                       kernels=got), f, indent=1, sort_keys=True)
        f.write("\n")
    print(", ".join("%s %d / %d" % (k, v["vgprs"], v["scratch_bytes"]) for k, v in got.items()))
