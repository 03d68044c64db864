"""The BGV hybrid entry points at the C boundary (CPU tier: nothing is launched): include/hehub_amd.h declares the four calls and their
_at twins -- the plain call's parameters with key_L0 after L, plain_modulus directly after moduli_ext -- hehub_amd/capi.py carries them
as their CKKS twins with a 64-bit plain modulus, and the Engine methods take key_L0 and out (exported, typed as the header types them,
refusing a NULL context: every call, tests/test_capi_symbols.py).
What the calls compute: tests/test_gpu_hks_bgv.py; the arithmetic they are held to: tests/test_hks_bgv_model.py."""
import inspect

import abi

PLAIN = ("hp_dev_bgv_hks_switch", "hp_dev_bgv_rotate_hoisted_hks", "hp_dev_bgv_relin_modswitch_hks",
         "hp_dev_bgv_mult_relin_modswitch_hks")
CALLS = PLAIN + tuple(name + "_at" for name in PLAIN)
CKKS_TWIN = {"hp_dev_bgv_hks_switch": "hp_dev_hks_switch", "hp_dev_bgv_rotate_hoisted_hks": "hp_dev_ckks_rotate_hoisted_hks",
             "hp_dev_bgv_relin_modswitch_hks": "hp_dev_ckks_relin_rescale_hks",
             "hp_dev_bgv_mult_relin_modswitch_hks": "hp_dev_ckks_mult_relin_rescale_hks"}
METHODS = ("bgv_hks_switch", "bgv_rotate_hoisted_hks", "bgv_relin_modswitch_hks", "bgv_mult_hks")


def test_header_declares_the_eight_calls():
    params = {name: abi.parameter_names(name) for name in CALLS + tuple(CKKS_TWIN.values())}
    for name in PLAIN:
        plain, at = params[name], params[name + "_at"]
        i = plain.index("L")
        assert at == plain[:i + 1] + ["key_L0"] + plain[i + 1:], name                       # key_L0 after L
        for p in (plain, at):
            assert p[p.index("moduli_ext") + 1] == "plain_modulus", name                   # as in hp_dev_bgv_mult_relin_modswitch
        assert [a for a in plain if a != "plain_modulus"] == params[CKKS_TWIN[name]], name  # otherwise the CKKS call's arguments


def test_ctypes_table_has_the_header_argument_counts():
    from hehub_amd import capi

    params = {name: abi.parameter_names(name) for name in CALLS}
    for name in PLAIN:
        res, args = capi.SIGNATURES[name]
        res_at, args_at = capi.SIGNATURES[name + "_at"]
        assert res is capi.INT and res_at is capi.INT and args[0] is capi.P, name
        assert len(args) == len(params[name]) and len(args_at) == len(params[name + "_at"]) == len(args) + 1, name
        assert args_at == args[:3] + [capi.szt] + args[3:], name   # (ctx, logn, L, key_L0, ...)
        assert args[params[name].index("plain_modulus")] is capi.u64, name
        twin = capi.SIGNATURES[CKKS_TWIN[name]][1]
        i = params[name].index("plain_modulus")
        assert args[:i] + args[i + 1:] == twin, name


def test_engine_methods_take_key_L0_and_out():
    from hehub_amd.engine import Engine

    for method in METHODS:
        sig = inspect.signature(getattr(Engine, method)).parameters
        for kw in ("key_L0", "out"):
            assert kw in sig and sig[kw].default is None, (method, kw)
        assert list(sig)[1:5] == ["moduli_ext", "t", "k", "alpha"], method
