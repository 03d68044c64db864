"""The discrete Gaussian entry points at the C boundary (CPU tier: nothing is launched, and a context needs a device): include/hehub_amd.h
declares hp_dev_sample_gauss and the error-sampler setting, no kind makes a NULL context acceptable, the header states the rule and
the Engine has the front-end methods (exported, typed as the header types them, refusing a NULL context with zeros: every call,
tests/test_capi_symbols.py).  What needs a context -- the refusals on a live one, the default, the fork -- is in
tests/test_gpu_gauss.py."""
import os
import re

import pytest

import abi

ROOT = abi.ROOT
COUNTS = {"hp_dev_sample_gauss": 6, "hp_ctx_set_error_sampler": 2, "hp_ctx_get_error_sampler": 1}
CALLS = tuple(COUNTS)


def test_header_declares_the_calls():
    assert {name: len(abi.parameter_names(name)) for name in CALLS} == COUNTS
    # the twin of hp_dev_sample_cbd: the same parameter list
    assert abi.parameter_list_text("hp_dev_sample_cbd") == abi.parameter_list_text("hp_dev_sample_gauss")


def test_header_states_the_rule_and_the_scope():
    text = abi.header_text()
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

    for name in CALLS:
        res, args = capi.SIGNATURES[name]
        assert res is capi.INT and len(args) == len(abi.parameter_names(name)) and args[0] is capi.P, name
    assert capi.SIGNATURES["hp_dev_sample_gauss"] == capi.SIGNATURES["hp_dev_sample_cbd"]
    assert capi.SIGNATURES["hp_ctx_set_error_sampler"][1][1] is capi.C.c_uint32


@pytest.mark.parametrize("name", CALLS)
def test_null_context_is_refused(name):
    from hehub_amd import capi

    for value in (0, 3, 4):   # (no kind makes a NULL context acceptable; the getter answers HP_EINVAL, not a kind)
        assert abi.null_context_call(capi.load(), name, fill=value) == capi.HP_EINVAL
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
