"""The lazy-relinearisation entry points at the C boundary (CPU tier: nothing is launched): include/hehub_amd.h declares
hp_dev_ckks_tensor_sum, hp_dev_ckks_relin_rescale_hks and hp_dev_ckks_dot_relin_rescale_hks with these argument counts, and the
Engine has the front-end methods (exported, typed as the header types them, refusing a NULL context: every call,
tests/test_capi_symbols.py).  What they compute: tests/test_gpu_tensor_sum.py and tests/test_gpu_hks_dot.py."""
import abi

COUNTS = {"hp_dev_ckks_tensor_sum": 9, "hp_dev_ckks_relin_rescale_hks": 10, "hp_dev_ckks_dot_relin_rescale_hks": 12}


def test_header_declares_the_calls():
    assert {name: len(abi.parameter_names(name)) for name in COUNTS} == COUNTS


def test_engine_has_the_front_end_methods():
    from hehub_amd.engine import Engine

    for method in ("ckks_tensor_sum", "ckks_relin_rescale_hks", "ckks_dot_hks"):
        assert callable(getattr(Engine, method))
