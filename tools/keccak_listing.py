"""What the shipped gfx950 listing of k_keccak.hip says about each of its kernels: scratch, conditional branches, and the size of one permutation.

    python tools/keccak_listing.py [build/csrc/k_keccak-hip-amdgcn-amd-amdhsa-gfx950.s]

Per kernel: private_segment_fixed_size, the VGPR count, and every conditional branch classified as
  exit    the first forward branch (the `if (i >= n) return` of the grid's last workgroup),
  loop    a backward branch (a loop's closing branch),
  guard   a forward branch from in front of a loop to right behind it (the "zero trips" test the compiler puts before a rotated loop),
  other   anything else.
For a kernel with exactly one loop, `loop_valu` / `loop_alignbit` count the VALU / v_alignbit_b32 instructions between the loop's label and its closing
branch: in k_keccak256 that is one block's loads folded into the state plus ONE Keccak-f[1600].  tests/test_keccak_cpu.py holds the listing to
profiles/r08/keccak_eth.txt with these numbers.
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = os.path.join(ROOT, "build", "csrc", "k_keccak-hip-amdgcn-amd-amdhsa-gfx950.s")


def kernels(path=DEFAULT):
    """{demangled-ish name: dict} for every kernel of the listing, in file order."""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        body.append(line.rstrip("\n"))
        if ".end_amdhsa_kernel" in line:
            out[name] = _analyse(body)
            name = None
    return out


def _analyse(body):
    label_at, code = {}, []
    for line in body:
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            label_at[m.group(1)] = len(code)
            continue
        t = line.strip()
        if not t or t.startswith((";", ".")) or ":" in t.split()[0]:
            m = re.match(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", t)
            if m:
                scratch = int(m.group(1))
            m = re.match(r"\.amdhsa_next_free_vgpr\s+(\d+)", t)
            if m:
                vgprs = int(m.group(1))
            continue
        code.append(t.split(";")[0].strip())
    branches = [(i, c.split()[0], c.split()[1]) for i, c in enumerate(code) if c.startswith("s_cbranch")]
    loops = [(label_at[t], i) for i, _, t in branches if label_at.get(t, i + 1) <= i]
    kinds, seen_exit = [], False
    for i, op, t in branches:
        to = label_at.get(t)
        if to is not None and to <= i:
            kinds.append("loop")
        elif not seen_exit:
            kinds.append("exit"); seen_exit = True
        elif any(i < head and to is not None and to > tail for head, tail in loops):
            kinds.append("guard")
        else:
            kinds.append("other")
    info = {"scratch": scratch, "vgprs": vgprs, "branches": kinds, "valu": sum(c.startswith("v_") for c in code),
            "alignbit": sum(c.startswith("v_alignbit_b32") for c in code)}
    if len(loops) == 1:
        inner = code[loops[0][0]:loops[0][1]]
        info["loop_valu"] = sum(c.startswith("v_") for c in inner)
        info["loop_alignbit"] = sum(c.startswith("v_alignbit_b32") for c in inner)
        info["loop_vmem"] = sum(c.startswith(("global_load", "flat_load", "buffer_load")) for c in inner)
    return info


def short(name):
    m = re.search(r"\d+(k_[a-z0-9_]+?)(?:I(.*?)E)?Ev", name)
    if not m:
        return name
    args = re.findall(r"L[ib](\d+)E", m.group(2) or "")
    return m.group(1) + ("<" + ", ".join(args) + ">" if args else "")


if __name__ == "__main__":
    for k, v in kernels(sys.argv[1] if len(sys.argv) > 1 else DEFAULT).items():
        print(f"{short(k):24s} {v}")
