"""hp_dev_ckks_lincomb (hp_lincomb.hip: k_ct_lincomb) against the exact model (tests/polyeval_model.py: Python integers modulo each
q_m), WORD for word -- the output is canonical, so there is nothing to reduce first.  Operands are stored with MORE limbs than the
call's L (a wrong row stride reads another limb's words), hold strict words, words in [q, 2q) and 2q - 1 (moduli.lazy_rows), and the
term counts cover one launch, a full table and a second, accumulating launch.  Then the largest sum the range function
(hpi::lincomb_max_terms, tests/test_lincomb_host.py) is about, the optional arguments, the chain of single calls the kernel replaces,
and the refusals."""
import ctypes as C

import numpy as np
import pytest

import moduli as M
import params as P
from oracle.pyoracle import SplitMix
from polyeval_model import model_lincomb

pytestmark = pytest.mark.gpu
U = np.uint64
EXTRA = (0, 1, 3)   # limbs an operand has beyond L, by term


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def operands(rng, q_top, L, n, T, B):
    """T ciphertext batches [B][2][L + extra][n] over the first moduli of q_top, lazy words"""
    return [M.lazy_rows(rng, (B, 2, L + EXTRA[j % 3], n), q_top[:L + EXTRA[j % 3]]) for j in range(T)]


def check(eng, q, cts, coefs, cst):
    d = [eng.to_device(x) for x in cts]
    got = eng.to_host(eng.ckks_lincomb(q, d, coefs, cst))
    B, n = cts[0].shape[0], cts[0].shape[-1]
    assert got.shape == (B, 2, len(q), n)
    for p in range(B):
        exp = model_lincomb(q, [x[p] for x in cts], coefs, cst)
        assert np.array_equal(got[p].astype(object), exp), p      # canonical words: equal as they are
    return got


@pytest.mark.parametrize("T", [1, 2, 32, 33])
@pytest.mark.parametrize("logn,L,B", [(3, 1, 1), (5, 3, 2), (11, 4, 2), (13, 2, 1)])
def test_lincomb_matches_the_integer_model(eng, logn, L, B, T):
    """(3, 1): a row shorter than one pair tile; (11, 4): the 512-word workgroup; (13, 2): full 2048-word tiles; 33 terms: two launches"""
    q_top, n = P.P40[:L + 3], 1 << logn
    q = q_top[:L]
    rng = SplitMix(9100 + 10 * logn + T)
    cts = operands(rng, q_top, L, n, T, B)
    coefs = [[int(rng.words(1, m)[0]) for m in q] for _ in range(T)]
    cst = [int(rng.words(1, m)[0]) for m in q]
    got = check(eng, q, cts, coefs, cst)
    assert (got < np.array(q, dtype=U)[:, None]).all()


@pytest.mark.parametrize("name,chain", [("P50", P.P50), ("W59", M.W59)])
@pytest.mark.parametrize("logn", [4, 11, 13])
def test_largest_sum_the_range_function_allows(eng, name, chain, logn):
    """a full table of 32 terms, EVERY operand word 2q - 1, every coefficient and the constant q - 1: the largest sum one launch forms,
    at 50-bit moduli and on the chain with a 59-bit q0; then one more term, which a second launch accumulates"""
    L, n, T = 2, 1 << logn, 32
    q = chain[:L]
    if name == "W59":
        assert q[0] == M.Q59 and q[0].bit_length() == 59
    x = np.stack([np.stack([np.full(n, 2 * m - 1, dtype=U) for m in q]) for _ in range(2)])[None]
    dx = eng.to_device(x)
    top = [m - 1 for m in q]
    for terms in (T, T + 1):
        got = eng.to_host(eng.ckks_lincomb(q, [dx] * terms, [top] * terms, top))
        for i, m in enumerate(q):
            assert (got[0, 0, i] == U((terms * (2 * m - 1) * (m - 1) + m - 1) % m)).all(), (terms, i)
            assert (got[0, 1, i] == U((terms * (2 * m - 1) * (m - 1)) % m)).all(), (terms, i)
    assert T * (q[0] - 1) * (2 * q[0] - 1) + 3 * q[0] <= ((1 << 64) - q[0]) * (1 << 64) - 1   # the host function's premise


def test_optional_arguments(eng):
    """coefs None (a plain sum), one coefficient None (1), cst None, and an operand of exactly L limbs"""
    logn, L = 11, 3
    q_top, n = P.P40[:L + 3], 1 << logn
    q = q_top[:L]
    rng = SplitMix(9200)
    cts = operands(rng, q_top, L, n, 3, 1)
    check(eng, q, cts, None, None)
    c1 = [int(rng.words(1, m)[0]) for m in q]
    check(eng, q, cts, [c1, None, c1], None)
    check(eng, q, cts[:1], [None], [m - 1 for m in q])
    check(eng, q, cts[:1], None, None)     # a reduced copy of the first L limbs


@pytest.mark.parametrize("logn,L,T", [(5, 3, 4), (12, 2, 8)])
def test_equals_the_chain_of_single_calls(eng, logn, L, T):
    """sum_j c_j x_j by hp_dev_poly_scalar_mul and hp_dev_poly_add, term after term, then hp_dev_poly_reduce_strict: the same words"""
    q, n = P.P40[:L], 1 << logn
    rng = SplitMix(9300 + logn)
    cts = [M.lazy_rows(rng, (2, 2, L, n), q) for _ in range(T)]
    coefs = [[int(rng.words(1, m)[0]) for m in q] for _ in range(T)]
    d = [eng.to_device(x) for x in cts]
    rows = lambda t: t.reshape(4, L, n)
    acc = eng.poly_scalar_mul(q, rows(d[0]), coefs[0])
    for j in range(1, T):
        acc = eng.poly_add(q, acc, eng.poly_scalar_mul(q, rows(d[j]), coefs[j]))
    chain = eng.to_host(eng.poly_reduce_strict_(q, acc)).reshape(2, 2, L, n)
    assert np.array_equal(eng.to_host(eng.ckks_lincomb(q, d, coefs)), chain)


def test_refusals_enqueue_nothing(eng):
    from hehub_amd import capi

    logn, L = 4, 2
    q, n = P.P40[:L], 1 << logn
    rng = SplitMix(9400)
    x = eng.to_device(rng.poly((1, 2, L + 1, n), P.P40[:L + 1]))
    out = eng.empty((1, 2, L, n))
    out.fill_(7)
    mod = (capi.u64 * L)(*q)
    good = (capi.u64 * L)(*[m - 1 for m in q])
    bad = (capi.u64 * L)(q[0] - 1, q[1])

    def call(terms, cts, limbs, coefs, cst, dst, L_=L, batch=1):
        cp = None if cts is None else (capi.P * len(cts))(*cts)
        kp = None if coefs is None else (capi.P * len(coefs))(*[None if c is None else C.addressof(c) for c in coefs])
        return eng.lib.hp_dev_ckks_lincomb(eng.h, logn, L_, mod, batch, terms, cp, (C.c_size_t * len(limbs))(*limbs), kp, cst, C.c_void_p(dst))

    xp, op = x.data_ptr(), out.data_ptr()
    assert call(1, [xp], [L + 1], [good], good, op) == capi.HP_OK       # the call as such is fine
    eng.sync()
    out.fill_(7)
    assert call(0, [xp], [L + 1], None, None, op) == capi.HP_EINVAL
    assert call(1, None, [L + 1], None, None, op) == capi.HP_EINVAL
    assert call(2, [xp, None], [L + 1, L + 1], None, None, op) == capi.HP_EINVAL
    assert call(1, [xp + 8], [L + 1], None, None, op) == capi.HP_EINVAL
    assert call(1, [xp], [L - 1], None, None, op) == capi.HP_EINVAL      # fewer limbs than L
    assert call(1, [xp], [33], None, None, op) == capi.HP_EINVAL
    assert call(1, [xp], [L + 1], [bad], None, op) == capi.HP_EINVAL     # a residue that is its modulus
    assert call(1, [xp], [L + 1], None, bad, op) == capi.HP_EINVAL
    assert call(1, [xp], [L + 1], None, None, None) == capi.HP_EINVAL
    assert call(1, [xp], [L + 1], None, None, op + 8) == capi.HP_EINVAL
    assert call(1, [xp], [L + 1], None, None, xp) == capi.HP_EINVAL      # the output is the operand
    assert call(1, [xp], [L + 1], None, None, xp + (2 * (L + 1) * n - 2) * 8) == capi.HP_EINVAL
    assert call(1, [xp], [L + 1], None, None, op, L_=0) == capi.HP_EINVAL
    assert call(1, [xp], [L + 1], None, None, op, batch=0) == capi.HP_EINVAL
    eng.sync()
    assert (eng.to_host(out) == 7).all()
