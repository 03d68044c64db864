"""hehub_amd/csrc/hp_sample.h and hp_sample_host.cpp against tests/sample_model.py (CPU tier, through tests/cpp/sample_shim.cpp, built
with g++).  The header's constexpr functions -- the word-13 packing, the block, the candidates, the uniform word rule, the ternary and
binomial rules -- are the very functions the kernels of hp_sample.hip call, so what holds here holds for the code the device runs, up
to the kernel's own indexing, which tests/test_gpu_sample.py covers on the same shapes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sample_cases as K
import sample_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "cpp", "libsample_shim.so")
CSRC = os.path.join(ROOT, "hehub_amd", "csrc")
U = np.uint64


@pytest.fixture(scope="module")
def ss():
    src = [os.path.join(ROOT, "tests", "cpp", "sample_shim.cpp"), os.path.join(CSRC, "hp_sample_host.cpp")]
    dep = src + [os.path.join(CSRC, "hp_sample.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in dep):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", SO] + src, check=True)
    lib = C.CDLL(SO)
    lib.ss_word13.restype = C.c_uint
    lib.ss_block.argtypes = [C.c_char_p, C.c_uint, C.c_uint, C.c_uint64, C.c_void_p]
    lib.ss_block_of_state.argtypes = [C.c_void_p, C.c_void_p]
    lib.ss_candidate.argtypes = [C.c_void_p, C.c_uint]
    lib.ss_candidate.restype = C.c_uint64
    lib.ss_uniform_word.argtypes = [C.c_uint64, C.c_void_p, C.POINTER(C.c_uint)]
    lib.ss_uniform_word.restype = C.c_uint64
    lib.ss_ternary_word.argtypes = lib.ss_cbd_word.argtypes = [C.c_uint64]
    lib.ss_ternary_word.restype = lib.ss_cbd_word.restype = C.c_longlong
    lib.ss_uniform.argtypes = [C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_uint64, C.c_size_t, C.c_void_p]
    lib.ss_uniform.restype = None
    lib.ss_signed.argtypes = [C.c_uint, C.c_size_t, C.c_size_t, C.c_char_p, C.c_uint64, C.c_longlong, C.c_void_p]
    lib.ss_signed.restype = None
    return lib


def host_uniform(ss, logn, moduli, batch, stream, ids=None, stride=0, out=None, seed=K.SEED):
    L, n = len(moduli), 1 << logn
    out = np.zeros((batch, L, n), dtype=U) if out is None else out
    marr = (C.c_uint64 * L)(*moduli)
    iarr = None if ids is None else (C.c_uint32 * L)(*ids)
    ss.ss_uniform(logn, L, marr, iarr, batch, seed, stream, stride, out.ctypes.data)
    return out


def test_layout_constants_and_block(ss):
    assert ss.ss_word13(5, 3, 200) == S.word13(5, 3, 200) and ss.ss_word13(0x1FFFF, 1, 0) == S.word13(0x1FFFF, 1, 0)
    state = np.array(list(S.CONSTANTS) + S.seed_words(bytes(range(32))) + [1, 0x09000000, 0x4A000000, 0], dtype=np.uint32)
    out = np.zeros(16, dtype=np.uint32)
    ss.ss_block_of_state(state.ctypes.data, out.ctypes.data)
    assert [int(w) for w in out[:4]] == [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3]     # RFC 8439 section 2.3.2
    for j, w13, stream in ((0, S.word13(0, 1, 0), 0), (8191, S.word13(63, 1, 255), (1 << 64) - 1), (7, S.word13(0, 3, 0), 1 << 32)):
        ss.ss_block(K.SEED, j, w13, stream, out.ctypes.data)
        exp = S.chacha20_blocks(S.states(K.SEED, [j], w13, stream))
        assert np.array_equal(out, exp[0])
        assert [ss.ss_candidate(out.ctypes.data, c) for c in range(8)] == [int(v) for v in S.candidates(exp)[0]]


@pytest.mark.parametrize("q", K.PLANT_MODULI, ids=lambda q: f"{q.bit_length()}b")
def test_planted_candidates_through_the_shared_word_rule(ss, q):
    for cands, word, used in K.planted_sequences(q):
        seen = C.c_uint(0)
        assert ss.ss_uniform_word(q, (C.c_uint64 * 64)(*cands), C.byref(seen)) == word == S.uniform_word(q, cands)
        assert seen.value == used


def test_ternary_and_binomial_rules(ss):
    m = (1 << 21) - 1
    words = [0, 1, 2, 3, 0b0111, 0b1011, 0b0011, S.M64, S.M64 >> 2, (2 << 62) | (S.M64 >> 2), (1 << 62) | (S.M64 >> 2),
             m, m << 21, m | m << 21, ~(m | m << 21) & S.M64, 0b101 | 1 << 21]
    words += [int(v) for v in S.candidates(S.chacha20_blocks(S.states(K.SEED, np.arange(64), 0, 1))).reshape(-1)]
    for v in words:
        assert ss.ss_ternary_word(v) == S.ternary_word(v), hex(v)
        assert ss.ss_cbd_word(v) == S.cbd_word(v), hex(v)
    assert ss.ss_cbd_word(m) == 21 and ss.ss_cbd_word(m << 21) == -21 and ss.ss_ternary_word(S.M64) == 0


@pytest.mark.parametrize("name", sorted(K.UNIFORM_CASES))
def test_host_uniform_equals_the_model(ss, name):
    logn, moduli, batch, stream, ids = K.UNIFORM_CASES[name]
    got = host_uniform(ss, logn, moduli, batch, stream, ids)
    assert np.array_equal(got, K.model_uniform(logn, moduli, stream, ids, batch))
    assert bool((got < np.array(moduli, dtype=U)[None, :, None]).all())


def test_host_uniform_with_a_stride(ss):
    logn, moduli, batch, stream = K.STRIDE_CASE
    L, n = len(moduli), 1 << logn
    stride = L * n + 64
    buf = np.full(batch * stride + 64, 0x5A5A5A5A5A5A5A5A, dtype=U)
    host_uniform(ss, logn, moduli, batch, stream, stride=stride, out=buf)
    exp = K.model_uniform(logn, moduli, stream, None, batch)
    for b in range(batch):
        assert np.array_equal(buf[b * stride:b * stride + L * n].reshape(L, n), exp[b])
        assert bool((buf[b * stride + L * n:(b + 1) * stride] == 0x5A5A5A5A5A5A5A5A).all())
    assert bool((buf[batch * stride:] == 0x5A5A5A5A5A5A5A5A).all())


@pytest.mark.parametrize("logn", K.SIGNED_LOGN)
def test_host_ternary_and_binomial_equal_the_model(ss, logn):
    for kind in (S.TERNARY, S.CBD):
        for scale in (1, 65537):
            out = np.zeros((K.SIGNED_BATCH, 1 << logn), dtype=np.int64)
            ss.ss_signed(kind, logn, K.SIGNED_BATCH, K.SEED, K.SIGNED_STREAM, scale, out.ctypes.data)
            assert np.array_equal(out, scale * K.model_signed(kind, logn))
