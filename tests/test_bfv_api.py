"""The BFV entry points at the C boundary (CPU tier: nothing is launched): include/hehub_amd.h declares the six calls -- the
relinearising pair as a plain call and its _at twin with key_L0 after L --, hehub_amd/capi.py carries them with the header's argument
counts and types, and the Engine has a method for each (exported, typed as the header types them, refusing a NULL context: every
call, tests/test_capi_symbols.py).  The refusals that need
a context (every rule of the header comment, with its code, nothing enqueued): tests/test_gpu_bfv.py; what the calls compute: the same
file; the arithmetic they are held to: tests/test_bfv_model.py; the host's base-size decision and constants: tests/test_bfv_host.py."""
import inspect

import abi

PARAMS = {
    "hp_dev_bfv_lift": ["ctx", "logn", "L", "M", "moduli_qb", "polys", "d_in", "d_out"],
    "hp_dev_bfv_scale_round": ["ctx", "logn", "L", "M", "moduli_qb", "t", "polys", "d_in", "d_out"],
    "hp_dev_bfv_mult_low_level": ["ctx", "logn", "L", "M", "moduli_qb", "t", "batch", "d_ct1", "d_ct2", "d_quad"],
    "hp_dev_bfv_mult_relin_hks": ["ctx", "logn", "L", "k", "alpha", "moduli_ext", "M", "aux_moduli", "t", "batch", "d_ct1", "d_ct2", "d_key",
                                  "d_out"],
    "hp_dev_bfv_mult_relin_hks_at": ["ctx", "logn", "L", "key_L0", "k", "alpha", "moduli_ext", "M", "aux_moduli", "t", "batch", "d_ct1", "d_ct2",
                                     "d_key", "d_out"],
    "hp_dev_bfv_decrypt_round": ["ctx", "n", "L", "moduli", "t", "polys", "d_x", "d_m"],
}
CALLS = tuple(PARAMS)
METHODS = ("bfv_lift", "bfv_scale_round", "bfv_mult_low_level", "bfv_mult_hks", "bfv_decrypt_round")


def test_header_declares_the_six_calls():
    assert {name: abi.parameter_names(name) for name in CALLS} == PARAMS


def test_ctypes_table_matches_the_header():
    from hehub_amd import capi

    for name, params in PARAMS.items():
        res, args = capi.SIGNATURES[name]
        assert res is capi.INT and len(args) == len(params), name
        for p, a in zip(params, args):
            want = capi.u64 if p == "t" else capi.szt if p in ("logn", "n", "L", "M", "k", "alpha", "key_L0", "polys", "batch") else capi.P
            assert a is want, (name, p)
    plain, at = capi.SIGNATURES["hp_dev_bfv_mult_relin_hks"][1], capi.SIGNATURES["hp_dev_bfv_mult_relin_hks_at"][1]
    assert at == plain[:3] + [capi.szt] + plain[3:]   # (ctx, logn, L, key_L0, ...)


def test_engine_has_a_method_for_every_call():
    from hehub_amd.engine import Engine

    for method in METHODS:
        sig = inspect.signature(getattr(Engine, method)).parameters
        assert "out" in sig and sig["out"].default is None, method
    sig = inspect.signature(Engine.bfv_mult_hks).parameters
    assert sig["key_L0"].default is None and list(sig)[1:6] == ["moduli_ext", "aux_moduli", "t", "k", "alpha"]
