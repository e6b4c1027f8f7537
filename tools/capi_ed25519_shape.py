"""What the host layer (ecsimd_amd/csrc/capi.hip) promises about the two SECRET Ed25519 entry points, read from its text -- tools/capi_secret_shape.py's idea
for calls that do not go through secret_base_product: the entry point sizes the workspace and places its arrays with ONE plan function, launches only the
Ed25519 launchers, reads nothing back, and ends every chunk with the shared wipe over that plan's total, whatever the launches said.
tests/test_ed25519_cpu.py holds the calls to it."""
import re

from capi_secret_shape import code, function, source   # noqa: F401


def check_ed25519_secret_entry(src, head, sign):
    body = function(src, head)
    launches = re.findall(r"launch::(\w+)\(", body)
    assert launches and set(launches) <= {"ed25519_secret_front", "ed25519_base_ct", "ed25519_sign_finish"}, (head, launches)
    assert ("ed25519_sign_finish" in launches) == sign and "ed25519_secret_front" in launches and "ed25519_base_ct" in launches, (head, launches)
    assert "hipMemcpy" not in body and "Synchronize" not in body and "hipMemset" not in body, head          # nothing read back, no wipe of its own
    wipes = re.findall(r"^.*\bwipe_workspace\(.*$", body, re.M)
    assert len(wipes) == 1, head
    m = re.fullmatch(r"\s*err = wipe_workspace\(ctx, (\w+)\.bytes, hipGetLastError\(\)\);\s*", wipes[0])     # no `if` in front of it, no literal size
    assert m, wipes[0]
    name = m.group(1)
    placed = re.search(r"\b" + name + r" = (\w+)\(ctx->workspace([^;]*)\);", body)
    assert placed, (head, name)
    plan, args = placed.group(1), placed.group(2)
    assert "ensure_workspace(ctx, " + plan + "(nullptr" + args + ").bytes)" in body, (head, plan)
    loop = body[body.index("FOR_CHUNKS("):]
    assert body.index("ensure_workspace(ctx, " + plan) < placed.start() < body.index("FOR_CHUNKS(")
    assert loop.index("launch::ed25519_secret_front(") < loop.index("launch::ed25519_base_ct(") < loop.index("wipe_workspace("), head      # the wipe is inside the chunk loop, last
    assert "launch::" not in loop[loop.index("wipe_workspace("):], head
    # the plan: every array comes from the carve, and `bytes` is the carve's total
    planned = function(src, "ed25519_secret_layout " + plan + "(")
    assert "carve_from(base)" in planned and re.search(r"\bL\.bytes = c\.bytes;", planned), plan
    return body
