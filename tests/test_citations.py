"""Every `file:line[-line]` citation of a reference file in this repo's sources and documents points INTO that file.  Where the reference's sources
are on the machine the line counts are read from them (and must equal the stored table); elsewhere from tests/golden/reference_line_counts.json,
minted from those sources by `python tests/test_citations.py --mint`.  The citations are how a reader checks a claim of parity against the reference; a stale or mistyped line range is a claim
nobody can check.  (Same-named files exist on both sides by design -- include/ecsimd/*.h keeps the reference's header names: a citation means the reference's.)"""
import collections
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
PATTERN = re.compile(r"(?<![\w/.-])((?:[\w-]+/)*[\w-]+\.(?:h|hpp|cpp|py|txt)):(\d+)(?:-(\d+))?")
SKIP_DIRS = ("/.git", "/build", "/gpurun_out", "/profiles", "/__pycache__", "/.pytest_cache")
LINE_COUNTS = os.path.join(ROOT, "tests", "golden", "reference_line_counts.json")
CITABLE = (".h", ".hpp", ".cpp", ".py", ".txt")
NOT_OURS = ("VERDICT.md", "ADVICE.md", "SURVEY.md", "BASELINE.md", "PAPERS.md", "SNIPPETS.md")        # written by others


def live_line_counts():
    """{path relative to the reference's root: number of lines} of every file a citation can name, from the reference's sources; None where they are absent."""
    if not os.path.isdir(os.path.join(REF, "include", "ecsimd")):
        return None
    counts = {}
    for d, _, fs in os.walk(REF):
        if "/.git" in d:
            continue
        for f in fs:
            if f.endswith(CITABLE):
                path = os.path.join(d, f)
                counts[os.path.relpath(path, REF)] = sum(1 for _ in open(path, errors="ignore"))
    return counts


def test_every_cited_line_range_exists_in_the_reference():
    stored = json.load(open(LINE_COUNTS))["files"]
    live = live_line_counts()
    if live is not None:
        assert live == stored, "tests/golden/reference_line_counts.json is stale: python tests/test_citations.py --mint"
    by_name = collections.defaultdict(list)
    for rel in stored:
        by_name[os.path.basename(rel)].append("/" + rel)
    lines = lambda path: stored[path[1:]]
    checked, bad = 0, []
    for d, _, fs in os.walk(ROOT):
        if any(x in d for x in SKIP_DIRS):
            continue
        for f in fs:
            if f in NOT_OURS or not f.endswith((".h", ".cuh", ".hip", ".inc", ".py", ".md", ".c", ".cpp", ".sh")):
                continue
            path = os.path.join(d, f)
            for m in PATTERN.finditer(open(path, errors="ignore").read()):
                name, first, last = m.group(1), int(m.group(2)), int(m.group(3) or m.group(2))
                base = os.path.basename(name)
                if base not in by_name:
                    continue                                    # one of this repo's own files (capi.hip:123), or not a file of the reference
                cands = [c for c in by_name[base] if c.endswith("/" + name)] or by_name[base]
                checked += 1
                if not any(first <= last <= lines(c) for c in cands):
                    bad.append((os.path.relpath(path, ROOT), m.group(0)))
    assert checked > 400 and not bad, bad[:20]


if __name__ == "__main__" and sys.argv[1:] == ["--mint"]:
    table = live_line_counts()
    assert table is not None, "the reference's sources are not on this machine"
    with open(LINE_COUNTS, "w") as f:
        json.dump({"_about": "line counts of the reference's files that a citation can name (tests/test_citations.py --mint)", "files": dict(sorted(table.items()))}, f, indent=0)
        f.write("\n")
