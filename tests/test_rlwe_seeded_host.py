"""hp_sample_residue (hehub_amd/csrc/hp_sample.h) and hpi::sample_small_host (hp_sample_host.cpp) against Python integers (CPU tier,
through tests/cpp/rlwe_seeded_shim.cpp, built with g++).  k_sample_spread calls the same constexpr rule on the same block, so what holds
here holds for the residues the device writes, up to the kernel's own indexing (tests/test_gpu_rlwe_seeded.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rlwe_seeded_cases as RC
import rlwe_seeded_model as R
import sample_cases as K
import sample_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "cpp", "librlwe_seeded_shim.so")
CSRC = os.path.join(ROOT, "hehub_amd", "csrc")


@pytest.fixture(scope="module")
def rs():
    src = [os.path.join(ROOT, "tests", "cpp", "rlwe_seeded_shim.cpp"), os.path.join(CSRC, "hp_sample_host.cpp")]
    dep = src + [os.path.join(CSRC, "hp_sample.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in dep):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", SO] + src, check=True)
    lib = C.CDLL(SO)
    lib.rs_residue.argtypes = [C.c_longlong, C.c_uint64]
    lib.rs_residue.restype = C.c_uint64
    lib.rs_small.argtypes = [C.c_uint, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_char_p, C.c_uint64, C.c_uint64, C.c_longlong,
                             C.c_void_p]
    lib.rs_small.restype = None
    return lib


@pytest.mark.parametrize("q", K.PLANT_MODULI, ids=lambda q: f"{q.bit_length()}b")
def test_residue_rule_at_the_edges(rs, q):
    for scale in RC.SMALL_SCALES:
        values = [0, 1, -1, 21 * scale, -21 * scale, scale, -scale, 20 * scale + 1]
        values += [q, -q, q - 1, 1 - q, q + 1, -q - 1] if q < 1 << 62 else []     # (multiples of q: -q is 0, not q)
        for v in values:
            assert abs(v) < 1 << 63
            got = rs.rs_residue(v, q)
            assert got == v % q and got < q, (v, q)


@pytest.mark.parametrize("kind", [S.TERNARY, S.CBD])
@pytest.mark.parametrize("logn", [3, 5, 11])
def test_host_sample_small_equals_the_model(rs, kind, logn):
    moduli, batch, stream = RC.HEAVY, 2, (1 << 32) - 1
    L, n = len(moduli), 1 << logn
    marr = (C.c_uint64 * L)(*moduli)
    for scale in RC.SMALL_SCALES:
        for step in (1, 2):
            out = np.zeros((batch, L, n), dtype=np.uint64)
            rs.rs_small(kind, logn, L, marr, batch, K.SEED, stream, step, scale, out.ctypes.data)
            for b in range(batch):
                row = R.small_row(kind, logn, K.SEED, stream + b * step)
                assert np.array_equal(out[b], R.residues(moduli, [scale * int(v) for v in row])), (scale, step, b)
