"""The sampling entry points at the C boundary (CPU tier: nothing is launched): include/hehub_amd.h declares the three samplers, the
two seeded key generators and hp_dev_hks_key_expand with these argument counts, and hehub_amd/capi.py passes the stream ids and the
error scales as 64-bit values (exported, typed as the header types them, refusing a NULL context: every call,
tests/test_capi_symbols.py).  What they compute: tests/test_gpu_sample.py."""
import os

import abi

ROOT = abi.ROOT
COUNTS = {"hp_dev_sample_uniform": 10, "hp_dev_sample_ternary": 6, "hp_dev_sample_cbd": 6, "hp_dev_hks_keygen_seeded": 13,
          "hp_dev_hks_keygen_rot_seeded": 14, "hp_dev_hks_key_expand": 10}


def test_header_declares_the_calls():
    assert {name: len(abi.parameter_names(name)) for name in COUNTS} == COUNTS


def test_header_carries_the_stream_table_and_what_is_out_of_scope():
    text = abi.header_text()
    for phrase in ("attempt (bits 0-15) | kind << 16 (bits 16-23) | limb_id << 24 (bits 24-31)", "RFC 8439", "a wire kind for half keys",
                   "fixed-Hamming-weight", "discrete Gaussians", "sampling inside the inner", "node, sharded and C++ host layers"):
        assert phrase in text, phrase


def test_ctypes_table_has_the_header_argument_counts():
    from hehub_amd import capi

    for name in COUNTS:
        res, args = capi.SIGNATURES[name]
        assert res is capi.INT and len(args) == len(abi.parameter_names(name)) and args[0] is capi.P, name
    # the stream id and the error scale are 64-bit values, not pointers
    assert capi.SIGNATURES["hp_dev_sample_uniform"][1][7] is capi.u64
    assert capi.SIGNATURES["hp_dev_hks_keygen_seeded"][1][10:12] == [capi.u64, capi.u64]
    assert capi.SIGNATURES["hp_dev_hks_keygen_rot_seeded"][1][11:13] == [capi.u64, capi.u64]
    assert capi.SIGNATURES["hp_dev_hks_key_expand"][1][8] is capi.u64


def test_engine_has_the_front_end_methods():
    from hehub_amd.engine import Engine

    for method in ("sample_uniform", "sample_ternary", "sample_cbd", "hks_keygen_seeded", "hks_keygen_rot_seeded", "hks_key_expand"):
        assert callable(getattr(Engine, method))


def test_the_sampling_kernel_is_built_from_its_own_source():
    from hehub_amd import build

    assert "hp_sample.hip" in build.SOURCES and "hp_sample_host.cpp" in build.SOURCES
    text = open(os.path.join(ROOT, "hehub_amd", "csrc", "hp_sample.hip")).read()
    assert "__builtin_rotateleft32" in text and "asm" not in text.replace("assembly", "") and "__shared__" not in text
