"""The C-ABI library loads and exports every symbol include/hehub_amd.h declares (no compute calls:
this runs without a GPU), and the ctypes table in hehub_amd/capi.py matches the header."""
import ctypes
import os
import re

import pytest

import abi
from hehub_amd import capi

ROOT = abi.ROOT
# every entry point that returns a status and takes a context first (the hp_wire_ calls take a descriptor)
TAKES_CONTEXT = [name for name, (res, args) in capi.SIGNATURES.items()
                 if res is capi.INT and args and args[0] is capi.P and not name.startswith("hp_wire_")]


def test_library_exports_every_declared_symbol():
    from hehub_amd.build import build_lib

    lib = ctypes.CDLL(build_lib())
    names = sorted(abi.prototypes())
    assert len(names) >= 40
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.hp_version is not None
    lib.hp_version.restype = ctypes.c_char_p
    assert b"gfx950" in lib.hp_version()


def test_ctypes_table_matches_header():
    """the same names, and for every one the restype and every argtypes entry of the header's type class (abi.CTYPES)"""
    assert sorted(capi.SIGNATURES) == sorted(abi.prototypes())
    for name, (ret, params) in abi.prototypes().items():
        res, args = capi.SIGNATURES[name]
        assert abi.agrees(res, ret), f"{name}: restype {res} for the header's `{ret}`"
        assert len(args) == len(params), f"{name}: {len(args)} argtypes for the header's {[p for _, p in params]}"
        for a, (cls, param) in zip(args, params):
            assert abi.agrees(a, cls), f"{name}, parameter {param}: argtypes {a} for the header's `{cls}`"
            assert param != "ctx" or a is capi.P, f"{name}: the context is passed as {a}"
    capi.load()


def test_engine_fails_loudly_without_gpu():
    import pytest
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from hehub_amd import capi
    from hehub_amd.engine import Engine

    with pytest.raises(capi.EngineMissing):
        Engine(0)


def test_product_never_touches_the_oracle():
    """hehub_amd/ must not import, link or execute anything under oracle/."""
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "hehub_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".hpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                if re.search(r"hehub_oracle|pyoracle|oracle/|from oracle|import oracle|orc_[a-z]", text):
                    bad.append(os.path.join(dirpath, f))
    assert not bad, bad


def test_public_header_is_plain_c(tmp_path):
    """include/hehub_amd.h must be usable from C (the boundary is a C ABI) and from C++."""
    import subprocess

    src = tmp_path / "use.c"
    src.write_text('#include "hehub_amd.h"\nint main(void) { hp_wire_desc d; hp_ctx *c = 0; (void)d; (void)c; return HP_OK; }\n')
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{inc}", "-fsyntax-only", str(src)], check=True)
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", f"-I{inc}", "-fsyntax-only", "-x", "c++", str(src)], check=True)


@pytest.mark.parametrize("name", TAKES_CONTEXT)
def test_null_context_is_an_argument_error_everywhere(name):
    """every entry point that takes a context rejects NULL with HP_EINVAL before touching HIP: runs without a GPU"""
    assert abi.null_context_call(capi.load(), name) == capi.HP_EINVAL


def test_null_context_special_cases():
    lib = capi.load()
    assert len(TAKES_CONTEXT) >= 60
    assert lib.hp_ctx_create(0, None) == capi.HP_EINVAL
    assert lib.hp_last_error(None) == b"null context"
    assert lib.hp_ctx_workspace_bytes(None) == 0 and lib.hp_ctx_get_stream(None) is None
    lib.hp_ctx_destroy(None)


def test_shipped_kernel_sources_have_no_experiment_switches():
    """no result-changing or A/B preprocessor switches in the shipped sources; the only conditional
    block left is the HP_TRACE instrumentation (shader-clock stamps, results unchanged), which build.py never defines"""
    csrc = os.path.join(ROOT, "hehub_amd", "csrc")
    found = []
    for f in sorted(os.listdir(csrc)):
        text = open(os.path.join(csrc, f), errors="ignore").read()
        found += [(f, m) for m in re.findall(r"^\s*#\s*if(?:n?def)?\s+(?:defined\()?(\w+)", text, flags=re.M)]
    allowed = {"HP_TRACE", "HP_TRACE_ALL", "HP_TRACE_WAVES", "__cplusplus"}   # (all three: which waves the instrumentation records)
    assert not [x for x in found if x[1] not in allowed], found
    assert "ABLATE" not in open(os.path.join(csrc, "hp_ntt_fast.hip")).read()
    build = open(os.path.join(ROOT, "hehub_amd", "build.py")).read()
    assert "-D" not in build
