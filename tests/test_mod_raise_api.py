"""hp_dev_ckks_mod_raise at the C boundary (CPU tier: nothing is launched): include/hehub_amd.h declares it, hehub_amd/capi.py
carries it with these types, it refuses a NULL context whatever else it is given, the header states its refusals, its bound and
what it leaves out, and the engine has the front-end method (exported, typed as the header types it: every call,
tests/test_capi_symbols.py).  The refusals that need a context -- every HP_EINVAL and HP_EUNSUPPORTED of the header, each leaving
d_out untouched -- and what the call computes: tests/test_gpu_mod_raise.py."""
import re

import abi

CALL = "hp_dev_ckks_mod_raise"


def test_header_declares_the_call():
    assert abi.parameter_names(CALL) == ["ctx", "logn", "L", "moduli", "in_limbs", "batch", "d_ct", "d_out"]


def test_header_states_refusals_and_bound():
    m = re.search(r"/\* %s:(.*?)\*/" % CALL, abi.header_text(), flags=re.S)
    assert m
    text = " ".join(m.group(1).replace("*", " ").split())
    for what in ("HP_EINVAL", "L < 2 or L > 32", "in_limbs == 0 or > 32", "batch == 0", "misaligned", "overlapping", "repeated modulus",
                 "HP_EUNSUPPORTED", "59 bits", "q_0 + q < 2^64", "Workspace", "(N, batch)", "parity level A", "below 2 q_m", "Out of scope", "SubSum", "single C entry",
                 "node, sharded", "device encoder", "sparse-secret", "arcsine", "iterated", "hoisting across factors"):
        assert what in text, what


def test_ctypes_table_has_the_header_argument_count():
    from hehub_amd import capi

    assert capi.SIGNATURES[CALL] == (capi.INT, [capi.P, capi.szt, capi.szt, capi.P, capi.szt, capi.szt, capi.P, capi.P])


def test_null_context_is_refused():
    from hehub_amd import capi

    lib = capi.load()
    assert abi.null_context_call(lib, CALL) == capi.HP_EINVAL
    buf = (capi.u64 * 4)(97, 193, 0, 0)
    assert getattr(lib, CALL)(None, 3, 2, buf, 1, 1, buf, buf) == capi.HP_EINVAL


def test_engine_has_the_front_end_method():
    from hehub_amd.engine import Engine

    assert callable(getattr(Engine, "ckks_mod_raise"))
