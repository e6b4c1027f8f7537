"""CPU suite: every function include/ecsimd_hip.h declares is in exactly one class of tests/capture_matrix.py, and tests/test_gpu_graph_capture.py has one
case for every name that claims to be capturable and one for every name that claims to refuse.  An entry point added to the header without a decision about
stream capture fails here, on a machine without a GPU."""
import os
import re

import capture_matrix as matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ecsimd_hip.h")
PREFIX = "ecsimd_hip_"


def declared(text):
    """The function names of the header, as ecsimd_amd.engine.declared_symbols finds them (what tests/test_abi.py holds the library's exports to)."""
    return sorted(set(re.findall(r"\b(ecsimd_hip_[a-z0-9_]+)\s*\(", text)))


def problems(text, classes):
    """What is wrong between a header's text and a classification {class name: names}: a list of sentences, empty when all is well."""
    names = [n[len(PREFIX):] for n in declared(text)]
    where = {}
    for cls, members in classes.items():
        for name in members:
            where.setdefault(name, []).append(cls)
    out = [f"{name} is declared and in no class" for name in names if name not in where]
    out += [f"{name} is in {' and '.join(cls)}" for name, cls in sorted(where.items()) if len(cls) > 1]
    out += [f"{name} ({where[name][0]}) is not declared any more" for name in sorted(where) if name not in names]
    return out


def test_every_declared_function_is_in_exactly_one_class():
    from ecsimd_amd.engine import declared_symbols
    text = open(HEADER).read()
    assert len(declared(text)) >= 100 and declared(text) == declared_symbols(), "this file and the engine read the same declarations out of the header"
    assert len(set(matrix.CAPTURABLE)) == len(matrix.CAPTURABLE), "a name is listed twice in CAPTURABLE"
    assert problems(text, matrix.CLASSES) == []
    assert all(reason.strip() for reason in list(matrix.REFUSES.values()) + list(matrix.NO_STREAM.values())), "every REFUSES / NO_STREAM name says why"


def test_the_check_bites():
    """A name taken out of the matrix, a name in two classes, a stale name, and a declaration added to a copy of the header each fail the check."""
    text = open(HEADER).read()
    without = {cls: [n for n in members if n != "sha512"] for cls, members in matrix.CLASSES.items()}
    assert problems(text, without) == ["sha512 is declared and in no class"]
    twice = dict(matrix.CLASSES, NO_STREAM=list(matrix.NO_STREAM) + ["sync"])
    assert problems(text, twice) == ["sync is in REFUSES and NO_STREAM"]
    stale = dict(matrix.CLASSES, CAPTURABLE=matrix.CAPTURABLE + ["sha3_256"])
    assert problems(text, stale) == ["sha3_256 (CAPTURABLE) is not declared any more"]
    grown = text.replace("int ecsimd_hip_sync(ecsimd_hip_ctx* ctx);", "int ecsimd_hip_sync(ecsimd_hip_ctx* ctx);\nint ecsimd_hip_brand_new(ecsimd_hip_ctx* ctx, size_t n);")
    assert grown != text
    assert problems(grown, matrix.CLASSES) == ["brand_new is declared and in no class"]


def test_the_gpu_file_has_a_case_for_every_capturable_and_every_refusing_name():
    """Importing the GPU file needs no GPU: its case tables are module-level dicts, name -> the graph (or the refused call) that covers it."""
    import test_gpu_graph_capture as gpu
    assert sorted(gpu.CAPTURABLE_CASES) == sorted(matrix.CAPTURABLE)
    assert sorted(gpu.REFUSES_CASES) == sorted(matrix.REFUSES)
    assert set(gpu.CAPTURABLE_CASES.values()) == set(gpu.GRAPHS), "every case names a graph of the file, and every graph of the file covers a name"
    assert all(callable(graph) for graph in gpu.GRAPHS.values()) and all(callable(call) for call in gpu.REFUSES_CASES.values())
