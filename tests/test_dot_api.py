"""The lazy-relinearisation entry points at the C boundary (CPU tier: nothing is launched): include/hehub_amd.h declares
hp_dev_ckks_tensor_sum, hp_dev_ckks_relin_rescale_hks and hp_dev_ckks_dot_relin_rescale_hks, hehub_amd/capi.py carries them with the
header's argument counts, the library exports them, and each refuses a NULL context.  What they compute: tests/test_gpu_tensor_sum.py
and tests/test_gpu_hks_dot.py."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("hp_dev_ckks_tensor_sum", "hp_dev_ckks_relin_rescale_hks", "hp_dev_ckks_dot_relin_rescale_hks")


def header_arguments():
    """{name: number of parameters} of the three prototypes, comments stripped"""
    text = open(os.path.join(ROOT, "include", "hehub_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = {}
    for name in CALLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        found[name] = len([a for a in m.group(1).split(",") if a.strip()])
    return found


def test_header_declares_the_calls():
    assert header_arguments() == {"hp_dev_ckks_tensor_sum": 9, "hp_dev_ckks_relin_rescale_hks": 10, "hp_dev_ckks_dot_relin_rescale_hks": 12}


def test_ctypes_table_has_the_header_argument_counts():
    from hehub_amd import capi

    for name, count in header_arguments().items():
        res, args = capi.SIGNATURES[name]
        assert res is capi.INT and len(args) == count and args[0] is capi.P, name


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

    for method in ("ckks_tensor_sum", "ckks_relin_rescale_hks", "ckks_dot_hks"):
        assert callable(getattr(Engine, method))
