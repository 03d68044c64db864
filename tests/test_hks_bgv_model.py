"""The model of the BGV hybrid calls (tests/hks_bgv_model.py) held to plain arithmetic and to decryption -- CPU tier, nothing is
launched.  (a) the remainder ModDown_t subtracts: delta = x mod P, t | delta, |delta| <= t (P + 1) / 2, for random and planted x
(the centring is c = u below floor(P/2) and u - P from there on, as k_hks_moddown has it: u = floor(P/2) = (P - 1)/2 gives
c = -(P + 1)/2, so the bound "t P / 2" holds up to that one half step and t (P + 1) / 2 is the exact one -- asserted, with equality
reached by the planted class u = floor(P/2));
(b) the planted inputs hold every edge class they claim; (c) t = 1 is hks_model.mod_down; (d) with keys whose error is t * e a
switch, a hoisted rotation and mult + relin + mod switch decrypt to the right message mod t.  t in {2, 65537, 2^31 - 1} throughout."""
import numpy as np
import pytest

import hks_bgv_model as B
from hks_model import chain, mod_down
from oracle.pyoracle import SplitMix

U = np.uint64
SHAPES = [(3, 3, 2, 2), (4, 4, 2, 2)]   # (logn, L, k, alpha): P = two 50-bit primes >= every digit of two 40-bit moduli
T = B.PLAIN_MODULI


def planted(seed, logn, L, k, t):
    mext = chain(L, k)
    return mext, B.planted_values(SplitMix(seed), mext, L, k, t, 1 << logn)


@pytest.mark.parametrize("t", T)
@pytest.mark.parametrize("logn,L,k,alpha", SHAPES + [(3, 3, 1, 1), (4, 3, 8, 3)])
def test_delta_is_x_mod_P_a_multiple_of_t_and_centred(logn, L, k, alpha, t):
    mext, w = planted(100 + t, logn, L, k, t)
    Q, Pm = B.prod(mext[:L]), B.prod(mext[L:])
    rng = SplitMix(7 + t)
    xs = [x for row in w for x in row] + [B.crt_all([int(rng.words(1, m)[0]) for m in mext], mext) for _ in range(64)]
    for x in xs:
        assert 0 <= x < Q * Pm
        d = B.delta_of(x, t, Pm)
        assert (x - d) % Pm == 0 and d % t == 0 and 2 * abs(d) <= t * (Pm + 1)
        assert d // t in range(-(Pm - Pm // 2), Pm // 2)          # c = u below floor(P/2), u - P from there on
        assert B.mod_down_int(x, t, Pm) * Pm + d == x
    assert max(2 * abs(B.delta_of(x, t, Pm)) for x in xs) == t * (Pm + 1)   # reached: u = floor(P/2)


@pytest.mark.parametrize("t", T)
@pytest.mark.parametrize("logn,L,k,alpha", SHAPES + [(3, 3, 1, 1), (4, 3, 8, 3)])
def test_every_planted_class_is_present(logn, L, k, alpha, t):
    mext, w = planted(200 + t, logn, L, k, t)
    found = B.planted_classes(w, mext, L, k, t)
    assert len(found) == 12 and all(found.values()), [name for name, ok in found.items() if not ok]


@pytest.mark.parametrize("t", T)
@pytest.mark.parametrize("logn,L,k,alpha", SHAPES)
def test_planted_key_makes_the_accumulator_the_planted_values(orc, logn, L, k, alpha, t):
    """the switch of the constant 1 with the planted key IS ModDown_t of w: the model agrees with plain integer arithmetic"""
    mext, w = planted(300 + t, logn, L, k, t)
    key = B.planted_key(orc, logn, mext, L, k, alpha, w)
    got = B.model_switch_bgv(orc, logn, mext, L, k, alpha, t, B.planted_pt(L, 1 << logn), key)
    assert np.array_equal(got, B.planted_expected(orc, logn, mext, L, k, t, w))


@pytest.mark.parametrize("logn,L,k,alpha", SHAPES + [(3, 3, 1, 1)])
def test_plain_modulus_one_is_the_ckks_moddown(orc, logn, L, k, alpha):
    mext, n = chain(L, k), 1 << logn
    random = SplitMix(400 + logn).poly((2, L + k, n), mext).astype(object)
    _, w = planted(401, logn, L, k, 1)   # and on the edge values: the accumulator whose coefficients are w
    edges = np.array([[orc.ntt(logn, q, np.array([x % q for x in w[h]], dtype=U)).astype(object) % q for q in mext] for h in range(2)],
                     dtype=object)
    for acc in (random, edges):
        assert np.array_equal(B.mod_down_bgv(orc, logn, mext, L, k, 1, acc), mod_down(orc, logn, mext, L, k, acc))


class Party:
    """a chain, a ternary secret and the message space of one decryption case"""

    def __init__(self, orc, seed, logn, L, k, alpha, t):
        self.orc, self.logn, self.L, self.k, self.alpha, self.t, self.n = orc, logn, L, k, alpha, t, 1 << logn
        self.mext, self.rng = chain(L, k), SplitMix(seed)
        self.q = self.mext[:L]
        self.s = B.ternary(self.rng, self.n)

    def message(self):
        return np.array([int(v) for v in self.rng.words(self.n, self.t)], dtype=object)

    def key(self, s_from):
        return B.keygen_bgv(self.orc, self.rng, self.logn, self.mext, self.L, self.k, self.alpha, self.t, self.s, s_from)


@pytest.mark.parametrize("t", T)
@pytest.mark.parametrize("logn,L,k,alpha", SHAPES)
def test_a_switch_decrypts_to_the_same_message(orc, logn, L, k, alpha, t):
    p = Party(orc, 500 + t + logn, logn, L, k, alpha, t)
    s_old = B.ternary(p.rng, p.n)
    msg = p.message()
    ct = B.encrypt_bgv(orc, p.rng, p.q, t, s_old, msg)
    assert np.array_equal(B.decrypt_bgv(orc, p.q, t, s_old, ct), msg)
    sw = B.model_switch_bgv(orc, logn, p.mext, L, k, alpha, t, ct[1], p.key(s_old))
    for m in range(L):
        sw[0, m] = (sw[0, m] + ct[0, m].astype(object)) % p.q[m]
    assert np.array_equal(B.decrypt_bgv(orc, p.q, t, p.s, sw.astype(U)), msg)


@pytest.mark.parametrize("t", T)
@pytest.mark.parametrize("logn,L,k,alpha", SHAPES)
def test_a_hoisted_rotation_decrypts_to_the_moved_message(orc, logn, L, k, alpha, t):
    p = Party(orc, 600 + t + logn, logn, L, k, alpha, t)
    steps, conj = [3, 0, 0], [False, False, True]   # a rotation, step 0, the row swap
    msg = p.message()
    ct = B.encrypt_bgv(orc, p.rng, p.q, t, p.s, msg)
    moved_s = [B.moved_coeffs(orc, p.q, p.s, st, cj) for st, cj in zip(steps, conj)]
    outs = B.model_hoisted_bgv(orc, logn, p.mext, L, k, alpha, t, ct, [p.key(ms) for ms in moved_s], steps, conj)
    for out, st, cj, ms in zip(outs, steps, conj, moved_s):
        moved_ct = np.stack([B.move(orc, ct[0], st, cj), B.move(orc, ct[1], st, cj)])
        want = B.decrypt_bgv(orc, p.q, t, ms, moved_ct)   # what the moved ciphertext decrypts to under the moved secret
        assert np.array_equal(B.decrypt_bgv(orc, p.q, t, p.s, out.astype(U)), want)
    assert np.array_equal(B.decrypt_bgv(orc, p.q, t, p.s, outs[1].astype(U)), msg)   # step 0: the message itself
    assert not np.array_equal(B.decrypt_bgv(orc, p.q, t, p.s, outs[0].astype(U)), msg)


@pytest.mark.parametrize("t", T)
@pytest.mark.parametrize("logn,L,k,alpha", SHAPES)
def test_mult_relin_modswitch_decrypts_to_the_negacyclic_product(orc, logn, L, k, alpha, t):
    p = Party(orc, 700 + t + logn, logn, L, k, alpha, t)
    m1, m2 = p.message(), p.message()
    ct1, ct2 = B.encrypt_bgv(orc, p.rng, p.q, t, p.s, m1), B.encrypt_bgv(orc, p.rng, p.q, t, p.s, m2)
    out = B.model_mult_bgv(orc, logn, p.mext, L, k, alpha, t, ct1, ct2, p.key(B.negacyclic(p.s, p.s)))
    assert out.shape == (2, L - 1, p.n)
    assert np.array_equal(B.decrypt_bgv(orc, p.q[:-1], t, p.s, out.astype(U)), B.negacyclic(m1, m2, t))
