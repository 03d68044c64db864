"""Lazy relinearisation over the hybrid key switch: hp_dev_ckks_dot_relin_rescale_hks -- a sum of T ciphertext products that pays ONE
switch and one rescale -- and hp_dev_ckks_relin_rescale_hks, the tail of the hybrid multiplication on a caller's quadratic ciphertext.

Pinned three ways:
  * against the exact model (tests/dot_model.py: the quadratic sum in Python integers, then model_switch, the oracle's poly_add and
    ckks_rescale), on strict residues with every word below 2q -- the device and the model hand the switch different representatives
    of sum d2 (tests/test_dot_model.py);
  * against the calls it is composed of and replaces, word for word where it is the same code on the same quad;
  * by decryption: q_last (out0 + out1 s) - sum_t (a0 + a1 s)(b0 + b1 s) is small."""
import numpy as np
import pytest

import moduli as M
import params as P
from dot_model import below_2q, model_dot, strict_rows
from hks_model import centred, centred_error, keygen
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def chain(L, k):
    return P.P40[:L] + P.P50[:k]


def operands(rng, mext, logn, L, k, alpha, T, B):
    """T terms of B ciphertexts each (strict words, words in [q, 2q), some 2q - 1) and a key of any words"""
    n, q = 1 << logn, mext[:L]
    a = [M.lazy_rows(rng, (B, 2, L, n), q) for _ in range(T)]
    b = [M.lazy_rows(rng, (B, 2, L, n), q) for _ in range(T)]
    key = rng.poly(((L + alpha - 1) // alpha, 2, L + k, n), mext)
    return a, b, key


def matches_model(orc, got, logn, mext, L, k, alpha, a, b, key):
    qm = mext[:L - 1]
    assert below_2q(got, qm)
    for p in range(got.shape[0]):
        exp = model_dot(orc, logn, mext, L, k, alpha, [x[p] for x in a], [x[p] for x in b], key)
        assert got[p].shape == exp.shape
        assert np.array_equal(strict_rows(got[p], qm), strict_rows(exp, qm)), p


@pytest.mark.parametrize("logn,L,k,alpha,T,B", [
    (4, 2, 1, 1, 1, 1),
    (5, 4, 2, 2, 3, 2),
    (11, 3, 2, 2, 5, 1),      # merged ModDown + rescale
    (11, 4, 2, 2, 33, 1),     # two launches of the sum
    (12, 5, 1, 3, 2, 2),
    (13, 3, 2, 1, 4, 1),
])
def test_dot_matches_the_exact_model(eng, orc, logn, L, k, alpha, T, B):
    mext = chain(L, k)
    rng = SplitMix(8300 + logn + L + T)
    a, b, key = operands(rng, mext, logn, L, k, alpha, T, B)
    d_a, d_b, d_key = [eng.to_device(x) for x in a], [eng.to_device(x) for x in b], eng.to_device(key)
    got = eng.to_host(eng.ckks_dot_hks(mext, k, alpha, d_a, d_b, d_key))
    matches_model(orc, got, logn, mext, L, k, alpha, a, b, key)
    # the two halves, called one after the other: the same code on the same quad, the same WORDS
    quad = eng.ckks_tensor_sum(mext[:L], d_a, d_b)
    assert np.array_equal(eng.to_host(eng.ckks_relin_rescale_hks(mext, k, alpha, quad, d_key)), got)
    if T == 1:   # one term: the residues of the fused multiplication
        mult = eng.to_host(eng.ckks_mult_hks(mext, k, alpha, d_a[0], d_b[0], d_key))
        assert np.array_equal(strict_rows(got, mext[:L - 1]), strict_rows(mult, mext[:L - 1]))


@pytest.mark.parametrize("logn,L,k,alpha", [(4, 2, 1, 1), (5, 4, 2, 2), (11, 3, 2, 2), (12, 5, 1, 3)])
def test_one_term_is_the_fused_multiplication(eng, logn, L, k, alpha):
    """T = 1: the strict residues of ckks_mult_hks on the same operands; and the exposed tail fed the output of mult_low_level returns
    the WORDS of ckks_mult_hks -- the same function after the same tensor product"""
    mext = chain(L, k)
    rng = SplitMix(8400 + logn + L)
    a, b, key = operands(rng, mext, logn, L, k, alpha, 1, 2)
    d_a, d_b, d_key = eng.to_device(a[0]), eng.to_device(b[0]), eng.to_device(key)
    mult = eng.to_host(eng.ckks_mult_hks(mext, k, alpha, d_a, d_b, d_key))
    dot = eng.to_host(eng.ckks_dot_hks(mext, k, alpha, [d_a], [d_b], d_key))
    qm = mext[:L - 1]
    assert below_2q(dot, qm) and np.array_equal(strict_rows(dot, qm), strict_rows(mult, qm))
    tail = eng.to_host(eng.ckks_relin_rescale_hks(mext, k, alpha, eng.mult_low_level(mext[:L], d_a, d_b), d_key))
    assert np.array_equal(tail, mult)


@pytest.mark.parametrize("logn,L,k,alpha,T,B", [(11, 4, 2, 2, 3, 1), (13, 6, 3, 3, 2, 1)])
def test_dot_at_parity_level_a(eng, orc, logn, L, k, alpha, T, B):
    """the sum is integer arithmetic at both levels; the tail runs its transforms and drops on the FP64 kernels: the residues of the
    level-B model, every word below 2q, and the range guard stays quiet (sync would report HP_ERANGE)"""
    mext = chain(L, k)
    rng = SplitMix(8500 + logn + L)
    a, b, key = operands(rng, mext, logn, L, k, alpha, T, B)
    d_a, d_b, d_key = [eng.to_device(x) for x in a], [eng.to_device(x) for x in b], eng.to_device(key)
    eng.set_parity_level("A")
    try:
        assert eng.parity_level() == "A"
        got = eng.to_host(eng.ckks_dot_hks(mext, k, alpha, d_a, d_b, d_key))
        eng.sync()
    finally:
        eng.set_parity_level("B")
    matches_model(orc, got, logn, mext, L, k, alpha, a, b, key)


def test_workspace_does_not_depend_on_the_number_of_terms():
    from hehub_amd.engine import Engine

    logn, L, k, alpha = 11, 3, 2, 2
    mext = chain(L, k)
    rng = SplitMix(8600)
    a, b, key = operands(rng, mext, logn, L, k, alpha, 1, 1)
    sizes = []
    for T in (2, 40):
        e = Engine(0)
        try:
            assert e.workspace_bytes() == 0
            x, y = e.to_device(a[0]), e.to_device(b[0])
            e.ckks_dot_hks(mext, k, alpha, [x] * T, [y] * T, e.to_device(key))
            e.sync()
            sizes.append(e.workspace_bytes())
        finally:
            e.close()
    assert sizes[0] == sizes[1] > 0, sizes


@pytest.mark.parametrize("logn,L,k,alpha,T", [(5, 4, 2, 2, 4), (11, 4, 2, 2, 3)])
def test_dot_decrypts_to_the_sum_of_products(eng, orc, logn, L, k, alpha, T):
    """With a ternary secret s and a relinearisation key for s^2 (keygen of tests/hks_model.py), over q_0 .. q_{L-2}:
        err = q_last (out0 + out1 s) - sum_t (a0 + a1 s)(b0 + b1 s)
    The rescale rounds each coefficient of out0 and of out1 by at most 1/2; out1's rounding meets a ternary s of N coefficients:
    q_last (N + 1) / 2.  The switch's noise is below 2^24 (test_switch_decrypts_to_pt_times_s_from, tests/test_hks.py).  Together
    below q_last (N + 2): a bound from the arithmetic, not a measurement."""
    mext = chain(L, k)
    n, q, qm, q_last = 1 << logn, mext[:L], mext[:L - 1], mext[L - 1]
    rng = SplitMix(8700 + logn + L)
    s = rng.words(n, 3).astype(np.int64) - 1
    s_ntt = orc.poly_reduce_strict(q, orc.poly_ntt(q, np.stack([(s % m).astype(U) for m in q])))
    s2 = centred(orc, q, orc.poly_mul(q, s_ntt, s_ntt))
    key = keygen(orc, rng, logn, mext, L, k, alpha, s, s2)
    a = [rng.poly((1, 2, L, n), q) for _ in range(T)]
    b = [rng.poly((1, 2, L, n), q) for _ in range(T)]
    out = eng.to_host(eng.ckks_dot_hks(mext, k, alpha, [eng.to_device(x) for x in a], [eng.to_device(x) for x in b], eng.to_device(key)))[0]
    sm = np.ascontiguousarray(s_ntt[:L - 1])
    low = lambda x: np.ascontiguousarray(x[:L - 1])
    dec = lambda c: orc.poly_add(qm, low(c[0]), orc.poly_mul(qm, low(c[1]), sm))
    lhs = orc.poly_rns_scalar_mul(qm, dec(out), [q_last % m for m in qm])
    rhs = None
    for x, y in zip(a, b):
        term = orc.poly_mul(qm, dec(x[0]), dec(y[0]))
        rhs = term if rhs is None else orc.poly_add(qm, rhs, term)
    worst = centred_error(orc, logn, qm, orc.poly_sub(qm, lhs, rhs))
    print(f"logn {logn} T {T}: |err| <= {worst} = 2^{float(np.log2(max(worst, 1))):.2f}, bound q_last (N + 2) = 2^{float(np.log2(q_last * (n + 2))):.2f}")
    assert worst < q_last * (n + 2)


def test_refusals_enqueue_nothing(eng):
    """the union of the two calls' checks, with HP_EINVAL before anything runs: the output keeps its words"""
    import ctypes as C

    from hehub_amd import capi

    logn, L, k, alpha = 4, 3, 1, 2
    mext = chain(L, k)
    n = 1 << logn
    rng = SplitMix(8800)
    a, b, key = operands(rng, mext, logn, L, k, alpha, 1, 1)
    x, y, d_key = eng.to_device(a[0]), eng.to_device(b[0]), eng.to_device(key)
    out = eng.empty((1, 2, L - 1, n))
    out.fill_(7)
    mod = (capi.u64 * (L + k))(*mext)

    def dot(terms, pa, pb, dst, L_=L, key_=d_key.data_ptr(), batch=1, alpha_=alpha):
        return eng.lib.hp_dev_ckks_dot_relin_rescale_hks(eng.h, logn, L_, k, alpha_, mod, batch, terms, (capi.P * len(pa))(*pa),
                                                         (capi.P * len(pb))(*pb), C.c_void_p(key_), C.c_void_p(dst))

    xp, yp, op = x.data_ptr(), y.data_ptr(), out.data_ptr()
    assert dot(0, [xp], [yp], op) == capi.HP_EINVAL
    assert dot(2, [xp, None], [yp, yp], op) == capi.HP_EINVAL
    assert dot(2, [xp, xp], [yp, yp + 8], op) == capi.HP_EINVAL
    assert dot(1, [xp], [yp], xp) == capi.HP_EINVAL                        # the output is an operand
    assert dot(1, [xp], [yp], yp + 2 * L * n * 8 - 16) == capi.HP_EINVAL   # ... or begins in one's last 16 bytes
    assert dot(1, [xp], [yp], op, key_=None) == capi.HP_EINVAL
    assert dot(1, [xp], [yp], op, batch=0) == capi.HP_EINVAL
    assert dot(1, [xp], [yp], op, alpha_=0) == capi.HP_EINVAL
    assert dot(1, [xp], [yp], op, L_=1) == capi.HP_EINVAL                  # nothing to rescale by
    quad = eng.mult_low_level(mext[:L], x, y)
    relin = lambda q_, dst: eng.lib.hp_dev_ckks_relin_rescale_hks(eng.h, logn, L, k, alpha, mod, 1, C.c_void_p(q_), C.c_void_p(d_key.data_ptr()),
                                                                  C.c_void_p(dst))
    assert relin(quad.data_ptr(), quad.data_ptr()) == capi.HP_EINVAL
    assert relin(quad.data_ptr(), quad.data_ptr() + 3 * L * n * 8 - 16) == capi.HP_EINVAL
    assert relin(None, op) == capi.HP_EINVAL and relin(quad.data_ptr() + 8, op) == capi.HP_EINVAL
    eng.sync()
    assert (eng.to_host(out) == 7).all()
    assert dot(1, [xp], [yp], op) == capi.HP_OK and relin(quad.data_ptr(), op) == capi.HP_OK
    eng.sync()
