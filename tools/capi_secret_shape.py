"""What the host layer (ecsimd_amd/csrc/capi.hip) promises about a SECRET base-point product, read from its text: the one shared product runs the
constant-time comb and the simultaneous inversion and reads nothing back; the one wipe zeroes the workspace whatever the launches returned, over a size
that comes from the call's carve of the workspace; and an entry point with a secret scalar goes through those two and launches no comb of its own.
tests/test_schnorr_cpu.py, tests/test_btc_cpu.py and tests/test_bip32_cpu.py hold their calls to it."""
import os
import re

CAPI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ecsimd_amd", "csrc", "capi.hip")


def source():
    return open(CAPI).read()


def code(text):
    """`text` without its // comments."""
    return re.sub(r"//[^\n]*", "", text)


def function(src, head):
    """The body of the one function whose definition starts with `head`, braces included, comments removed."""
    assert src.count(head) == 1, head
    at = src.index("{", src.index(head))
    text, depth = code(src[at:]), 0
    for i, ch in enumerate(text):
        depth += (ch == "{") - (ch == "}")
        if depth == 0:
            return text[:i + 1]
    raise AssertionError("unbalanced braces behind " + head)


def check_shared_product(src):
    """1. the shared product; 2. the wipe."""
    body = function(src, "void secret_base_product(")
    assert body.count("launch::") == 2
    assert body.count("launch::base_windowed_signed(ctx->stream, curve, k, ctx->windowct_table[curve], j.x, j.y, j.z, m, true)") == 1     # the constant-time argument
    assert body.count("launch::to_affine_batched(ctx->stream, curve, j.x, j.y, j.z, x, y, m, true)") == 1
    assert "hipMemcpy" not in body and "Synchronize" not in body                                          # nothing is read back
    assert len(re.findall(r"windowct_table\[curve\],", code(src))) == 1                                   # ... and no other launch takes that table
    wipe = function(src, "hipError_t wipe_workspace(ecsimd_hip_ctx* ctx, size_t bytes, hipError_t launches)")
    first = wipe.strip("{} \n").split(";")[0].strip()
    assert first == "const hipError_t wiped = hipMemsetAsync(ctx->workspace, 0, bytes, ctx->stream)", first    # unconditional: the first statement
    assert code(src).count("hipMemsetAsync(ctx->workspace") == 1                                          # ... and the only wipe of the block


def check_secret_entry(src, head, products, route=None):
    """3. the entry point `head` (or, with `route`, the part of it from that text on) calls the shared product `products` times, launches no comb of its own,
    reads nothing back, and ends every scope that holds a product with the shared wipe over its own carve's total."""
    body = function(src, head)
    if route is not None:
        assert body.count(route) == 1, route
        body = body[body.index(route):]
    assert len(re.findall(r"\bsecret_base_product\(", body)) == products, head
    assert "launch::base_windowed" not in body and "windowct_table" not in body, head
    assert "hipMemcpy" not in body and "Synchronize" not in body, head
    wipes = re.findall(r"^.*\bwipe_workspace\(.*$", body, re.M)
    assert len(wipes) == 1, head
    m = re.fullmatch(r"\s*(?:const hipError_t )?err = wipe_workspace\(ctx, (\w+)\.bytes, hipGetLastError\(\)\);\s*", wipes[0])
    assert m, wipes[0]                                                                                   # no `if` in front of it, no literal size
    name = m.group(1)
    # the same carve sized the block and placed the arrays: <name> = <plan>(ctx->workspace, ...) and ensure_workspace(ctx, <plan>(nullptr, ...).bytes)
    placed = re.search(r"\b" + name + r" = (\w+)\(ctx->workspace([^;]*)\);", body)
    assert placed, (head, name)
    plan, args = placed.group(1), placed.group(2)
    assert "ensure_workspace(ctx, " + plan + "(nullptr" + args + ").bytes)" in body, (head, plan)
    assert body.index("ensure_workspace(ctx, " + plan) < placed.start() < body.index("secret_base_product(") < body.index("wipe_workspace("), head
    return body
