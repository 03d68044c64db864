"""The key-generation entry points at the C boundary (CPU tier: nothing is launched): include/hehub_amd.h declares
hp_dev_poly_from_signed, hp_dev_hks_keygen and hp_dev_hks_keygen_rot with these argument counts, and the Engine has the front-end
methods (exported, typed as the header types them, refusing a NULL context: every call, tests/test_capi_symbols.py).  What they
compute: tests/test_gpu_hks_keygen.py."""
import abi

COUNTS = {"hp_dev_poly_from_signed": 7, "hp_dev_hks_keygen": 12, "hp_dev_hks_keygen_rot": 13}


def test_header_declares_the_calls():
    assert {name: len(abi.parameter_names(name)) for name in COUNTS} == COUNTS


def test_engine_has_the_front_end_methods():
    from hehub_amd.engine import Engine

    for method in ("poly_from_signed", "hks_keygen", "hks_keygen_rot"):
        assert callable(getattr(Engine, method))
