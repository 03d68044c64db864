"""The seeded ciphertext entry points at the C boundary (CPU tier: nothing is launched): include/hehub_amd.h declares
hp_dev_sample_small_ntt, hp_dev_rlwe_encrypt_seeded and hp_dev_rlwe_encrypt_pk_seeded, hehub_amd/capi.py carries them with the
header's argument counts, the library exports them, and each refuses a NULL context.  What they compute:
tests/test_gpu_rlwe_seeded.py."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = {"hp_dev_sample_small_ntt": 10, "hp_dev_rlwe_encrypt_seeded": 12, "hp_dev_rlwe_encrypt_pk_seeded": 11}
CALLS = tuple(COUNTS)


def header_text():
    return open(os.path.join(ROOT, "include", "hehub_amd.h")).read()


def header_arguments():
    """{name: number of parameters} of the prototypes, comments stripped"""
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    found = {}
    for name in CALLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        found[name] = len([a for a in m.group(1).split(",") if a.strip()])
    return found


def test_header_declares_the_calls():
    assert header_arguments() == COUNTS


def test_header_carries_the_contract_the_ids_and_what_is_out_of_scope():
    text = header_text()
    for phrase in ("CANONICAL residue", "stream .. stream + 2 * batch - 1", "stream .. stream + batch - 1", "c0 plus the 40 bytes",
                   "2 * L * N, d_ct + L * N", "public-key generation", "a wire kind for seeded ciphertexts",
                   "node, sharded and C++ host layers; CKKS encoding; discrete Gaussians"):
        assert phrase in text, phrase
    # the sampling block it sits next to is as it was
    assert text.index("hp_dev_hks_key_expand(hp_ctx") < text.index("Fresh ciphertexts from a seed") < text.index("BGV over the hybrid key switch")


def test_ctypes_table_has_the_header_argument_counts():
    from hehub_amd import capi

    for name, count in header_arguments().items():
        res, args = capi.SIGNATURES[name]
        assert res is capi.INT and len(args) == count and args[0] is capi.P, name
    # kind, stream, the scales and with_c1 are values, not pointers
    assert capi.SIGNATURES["hp_dev_sample_small_ntt"][1][5:9] == [capi.C.c_uint32, capi.P, capi.u64, capi.u64]
    assert capi.SIGNATURES["hp_dev_rlwe_encrypt_seeded"][1][8:11] == [capi.u64, capi.u64, capi.INT]
    assert capi.SIGNATURES["hp_dev_rlwe_encrypt_pk_seeded"][1][8:10] == [capi.u64, capi.u64]


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

    for method in ("sample_small_ntt", "rlwe_encrypt_seeded", "rlwe_encrypt_pk_seeded"):
        assert callable(getattr(Engine, method))
