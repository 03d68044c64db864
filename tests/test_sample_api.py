"""The sampling entry points at the C boundary (CPU tier: nothing is launched): include/hehub_amd.h declares the three samplers, the
two seeded key generators and hp_dev_hks_key_expand, hehub_amd/capi.py carries them with the header's argument counts, the library
exports them, and each refuses a NULL context.  What they compute: tests/test_gpu_sample.py."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = {"hp_dev_sample_uniform": 10, "hp_dev_sample_ternary": 6, "hp_dev_sample_cbd": 6, "hp_dev_hks_keygen_seeded": 13,
          "hp_dev_hks_keygen_rot_seeded": 14, "hp_dev_hks_key_expand": 10}
CALLS = tuple(COUNTS)


def header_arguments():
    """{name: number of parameters} of the prototypes, comments stripped"""
    text = open(os.path.join(ROOT, "include", "hehub_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = {}
    for name in CALLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        found[name] = len([a for a in m.group(1).split(",") if a.strip()])
    return found


def test_header_declares_the_calls():
    assert header_arguments() == COUNTS


def test_header_carries_the_stream_table_and_what_is_out_of_scope():
    text = open(os.path.join(ROOT, "include", "hehub_amd.h")).read()
    for phrase in ("attempt (bits 0-15) | kind << 16 (bits 16-23) | limb_id << 24 (bits 24-31)", "RFC 8439", "a wire kind for half keys",
                   "fixed-Hamming-weight", "discrete Gaussians", "sampling inside the inner", "node, sharded and C++ host layers"):
        assert phrase in text, phrase


def test_ctypes_table_has_the_header_argument_counts():
    from hehub_amd import capi

    for name, count in header_arguments().items():
        res, args = capi.SIGNATURES[name]
        assert res is capi.INT and len(args) == count and args[0] is capi.P, name
    # the stream id and the error scale are 64-bit values, not pointers
    assert capi.SIGNATURES["hp_dev_sample_uniform"][1][7] is capi.u64
    assert capi.SIGNATURES["hp_dev_hks_keygen_seeded"][1][10:12] == [capi.u64, capi.u64]
    assert capi.SIGNATURES["hp_dev_hks_keygen_rot_seeded"][1][11:13] == [capi.u64, capi.u64]
    assert capi.SIGNATURES["hp_dev_hks_key_expand"][1][8] is capi.u64


def test_library_exports_the_calls():
    import ctypes

    from hehub_amd.build import build_lib

    lib = ctypes.CDLL(build_lib())
    assert not [n for n in CALLS if not hasattr(lib, n)]


@pytest.mark.parametrize("name", CALLS)
def test_null_context_is_refused(name):
    from hehub_amd import capi

    lib = capi.load()
    _, args = capi.SIGNATURES[name]
    assert getattr(lib, name)(*[None if a is capi.P else 0 for a in args]) == capi.HP_EINVAL


def test_engine_has_the_front_end_methods():
    from hehub_amd.engine import Engine

    for method in ("sample_uniform", "sample_ternary", "sample_cbd", "hks_keygen_seeded", "hks_keygen_rot_seeded", "hks_key_expand"):
        assert callable(getattr(Engine, method))


def test_the_sampling_kernel_is_built_from_its_own_source():
    from hehub_amd import build

    assert "hp_sample.hip" in build.SOURCES and "hp_sample_host.cpp" in build.SOURCES
    text = open(os.path.join(ROOT, "hehub_amd", "csrc", "hp_sample.hip")).read()
    assert "__builtin_rotateleft32" in text and "asm" not in text.replace("assembly", "") and "__shared__" not in text
