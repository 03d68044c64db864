"""The discrete Gaussian entry points at the C boundary (CPU tier: nothing is launched, and a context needs a device): include/hehub_amd.h
declares hp_dev_sample_gauss and the error-sampler setting, hehub_amd/capi.py carries them with the header's argument counts, the
library exports them, each refuses a NULL context, the header states the rule and the Engine has the front-end methods.  What needs a
context -- the refusals on a live one, the default, the fork -- is in tests/test_gpu_gauss.py."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = {"hp_dev_sample_gauss": 6, "hp_ctx_set_error_sampler": 2, "hp_ctx_get_error_sampler": 1}
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
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    # the twin of hp_dev_sample_cbd: the same parameter list
    lists = [re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % n, text).group(1) for n in ("hp_dev_sample_cbd", "hp_dev_sample_gauss")]
    assert " ".join(lists[0].split()) == " ".join(lists[1].split())


def test_header_states_the_rule_and_the_scope():
    text = header_text()
    flat = " ".join(text.replace("\n *", " ").split())
    for phrase in ("4 discrete Gaussian", "rho(k) = exp(-25 k^2 / 512)", "floor(2^63 * (P(0) + ... + P(m)))", "m = 0 .. 29",
                   "sign = v_c & 1, u = v_c >> 1", "#{ i in 0..29 : u >= C[i] }", "Range +-30, variance 10.24", "below 2^-57",
                   "hp_ctx_set_error_sampler", "Kind 4 is not taken here", "a kind outside {2, 3}", "no environment variable", "hp_ctx_fork copies it",
                   "ternary whatever the error sampler"):
        assert phrase in flat, phrase
    # the seeded calls no longer promise a centred-binomial error, and what stays out of scope is another width, not the distribution
    assert "centred-binomial sample" not in flat
    assert "discrete Gaussians;" not in flat and flat.count("discrete Gaussians of any other width") == 2
    assert "Gaussian secrets" in flat and "fixed-Hamming-weight" in flat


def test_refusal_text_of_the_setting_names_the_two_kinds():
    assert "error sampler: kind is 3 (centred binomial) or 4 (discrete Gaussian)" in open(os.path.join(ROOT, "hehub_amd", "csrc", "hp_ctx.cpp")).read()


def test_ctypes_table_has_the_header_argument_counts():
    from hehub_amd import capi

    for name, count in header_arguments().items():
        res, args = capi.SIGNATURES[name]
        assert res is capi.INT and len(args) == count and args[0] is capi.P, name
    assert capi.SIGNATURES["hp_dev_sample_gauss"] == capi.SIGNATURES["hp_dev_sample_cbd"]
    assert capi.SIGNATURES["hp_ctx_set_error_sampler"][1][1] is capi.C.c_uint32


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
    for value in (0, 3, 4):   # (no kind makes a NULL context acceptable; the getter answers HP_EINVAL, not a kind)
        assert getattr(lib, name)(*[None if a is capi.P else value for a in args]) == capi.HP_EINVAL
    assert capi.HP_EINVAL not in (3, 4)


def test_there_is_no_environment_variable():
    text = open(os.path.join(ROOT, "hehub_amd", "csrc", "hp_ctx.cpp")).read()
    assert not [m for m in re.findall(r'getenv\("([^"]+)"\)', text) if "SAMPL" in m or "GAUSS" in m or "ERROR" in m]


def test_engine_has_the_front_end_methods():
    from hehub_amd.engine import Engine

    for method in ("sample_gauss", "set_error_sampler", "get_error_sampler", "sample_small_ntt"):
        assert callable(getattr(Engine, method))


def test_the_kernels_take_the_table_from_the_header():
    text = open(os.path.join(ROOT, "hehub_amd", "csrc", "hp_sample.hip")).read()
    assert "k_sample_signed<HP_SAMPLE_GAUSS>" in text and "k_gauss_spread" in text and "sample_spread_item<HP_SAMPLE_GAUSS>" in text
    assert "__shared__" not in text and "__constant__" not in text and "__device__ const" not in text
