"""The seeded ciphertext entry points at the C boundary (CPU tier: nothing is launched): include/hehub_amd.h declares
hp_dev_sample_small_ntt, hp_dev_rlwe_encrypt_seeded and hp_dev_rlwe_encrypt_pk_seeded with these argument counts, and
hehub_amd/capi.py passes the kind, the stream, the scales and with_c1 by value (exported, typed as the header types them, refusing
a NULL context: every call, tests/test_capi_symbols.py).  What they compute: tests/test_gpu_rlwe_seeded.py."""
import abi

COUNTS = {"hp_dev_sample_small_ntt": 10, "hp_dev_rlwe_encrypt_seeded": 12, "hp_dev_rlwe_encrypt_pk_seeded": 11}


def test_header_declares_the_calls():
    assert {name: len(abi.parameter_names(name)) for name in COUNTS} == COUNTS


def test_header_carries_the_contract_the_ids_and_what_is_out_of_scope():
    text = abi.header_text()
    for phrase in ("CANONICAL residue", "stream .. stream + 2 * batch - 1", "stream .. stream + batch - 1", "c0 plus the 40 bytes",
                   "2 * L * N, d_ct + L * N", "public-key generation", "a wire kind for seeded ciphertexts",
                   "node, sharded and C++ host layers; CKKS encoding; discrete Gaussians"):
        assert phrase in text, phrase
    # the sampling block it sits next to is as it was
    assert text.index("hp_dev_hks_key_expand(hp_ctx") < text.index("Fresh ciphertexts from a seed") < text.index("BGV over the hybrid key switch")


def test_ctypes_table_has_the_header_argument_counts():
    from hehub_amd import capi

    for name in COUNTS:
        res, args = capi.SIGNATURES[name]
        assert res is capi.INT and len(args) == len(abi.parameter_names(name)) and args[0] is capi.P, name
    # kind, stream, the scales and with_c1 are values, not pointers
    assert capi.SIGNATURES["hp_dev_sample_small_ntt"][1][5:9] == [capi.C.c_uint32, capi.P, capi.u64, capi.u64]
    assert capi.SIGNATURES["hp_dev_rlwe_encrypt_seeded"][1][8:11] == [capi.u64, capi.u64, capi.INT]
    assert capi.SIGNATURES["hp_dev_rlwe_encrypt_pk_seeded"][1][8:10] == [capi.u64, capi.u64]


def test_engine_has_the_front_end_methods():
    from hehub_amd.engine import Engine

    for method in ("sample_small_ntt", "rlwe_encrypt_seeded", "rlwe_encrypt_pk_seeded"):
        assert callable(getattr(Engine, method))
