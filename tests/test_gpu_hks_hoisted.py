"""hp_dev_ckks_rotate_hoisted_hks: many rotations of one ciphertext, each under its own hybrid key, over ONE digit decomposition.

The digit rows are those of the UNROTATED c1; a rotation moves them (inside the inner product) instead of decomposing the moved
polynomial.  A moved row is the transform of the moved digit read as a signed integer, so on the lifted limbs the words differ from
hp_dev_ckks_rotate_hks's, with the same magnitude bound.  Pinned
  * word for word (level B) by the exact model of tests/hks_model.py, split where the engine splits it: digit rows from the unrotated
    c1 (model_digits), each row moved with the oracle's cycle / involution, then the unchanged inner product and ModDown (model_rest);
  * against the unhoisted entry point where the two must agree (step 0);
  * by decryption with keys generated here, for the device's words and for the model's."""
import ctypes as C

import numpy as np
import pytest

import params as P
from hks_model import chain, decryption_errors, decryption_setup, model_hoisted, rotations_of, step0_case
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


# ---- (a) the exact model, word for word ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha,B,R", [
    (4, 4, 2, 2, 1, 33),    # more rotations than one argument table; steps 0, a duplicate, N/2 + 1, two conjugations
    (5, 5, 2, 2, 3, 3),     # short last digit; an odd number of ciphertexts for the two-per-thread kernel
    (5, 3, 1, 1, 2, 2),     # every digit one limb, one special prime
    (4, 3, 9, 3, 1, 2),     # one digit: nothing lifted among the q limbs; k > 8: the CRT ModDown
    (11, 3, 2, 2, 2, 3),    # tiled transforms, fused ModDown, full tiles; one conjugation
    (13, 3, 2, 1, 1, 2),    # several chunks per row
    (4, 3, 2, 2, 3, 12),    # several ciphertexts AND several passes over the digit rows: the rotations of a ciphertext are not adjacent in a pass
    (4, 2, 1, 1, 34, 2),    # more ciphertexts than a pass or a gather table holds
])
def test_hoisted_matches_the_exact_model(eng, orc, logn, L, k, alpha, B, R):
    mext = chain(L, k)
    n, q = 1 << logn, mext[:L]
    nd = (L + alpha - 1) // alpha
    rng = SplitMix(5100 + logn + L)
    steps, conj = rotations_of(logn, R)
    ct = np.stack([rng.poly((2, L, n), q) for _ in range(B)])
    nkeys = min(R, 5)
    keys = [rng.poly((nd, 2, L + k, n), mext) for _ in range(nkeys)]          # any words: the model is about arithmetic
    dkeys = [eng.to_device(key) for key in keys]
    which = [(r * 3 + 1) % nkeys for r in range(R)]
    got = eng.to_host(eng.ckks_rotate_hoisted_hks(mext, k, alpha, eng.to_device(ct), [dkeys[w] for w in which], steps, conj))
    assert got.shape == (B, R, 2, L, n)
    for b in range(B):
        exp = model_hoisted(orc, logn, mext, L, k, alpha, ct[b], [keys[w] for w in which], steps, conj)
        for r in range(R):
            assert np.array_equal(got[b, r], exp[r]), (b, r, steps[r], conj[r])


# ---- (b) step 0 is the plain switch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha", [(5, 4, 2, 2), (11, 3, 2, 2)])
def test_step_zero_is_the_unhoisted_rotation(eng, logn, L, k, alpha):
    plain, hoisted = step0_case(eng, logn, L, k, alpha)
    assert np.array_equal(plain, hoisted)


# ---- (c), (d) decryption --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha", [(5, 4, 2, 2), (6, 6, 3, 3), (11, 4, 2, 2)])
def test_hoisted_rotations_decrypt(eng, orc, logn, L, k, alpha):
    """out0 + out1 s = sigma_r(c0 + c1 s) up to the key-switch noise: the bound tests/test_hks.py holds the unhoisted switch to with the
    same key parameters (the signed digit representative has the magnitude bound of the non-negative one).  Below N = 2048 the model's
    words are held to the same bound, so a failure tells a wrong model from a wrong kernel."""
    mext = P.P40[:L] + P.P50[:k]
    n, q = 1 << logn, mext[:L]
    rng = SplitMix(5300 + logn + L)
    rots = [(1, False), (3, False), (0, True)]
    s_ntt, keys = decryption_setup(orc, rng, logn, mext, L, k, alpha, rots)
    ct = rng.poly((2, L, n), q)
    steps, conj = [r[0] for r in rots], [r[1] for r in rots]
    got = eng.to_host(eng.ckks_rotate_hoisted_hks(mext, k, alpha, eng.to_device(ct[None]), [eng.to_device(key) for key in keys], steps, conj))[0]
    Q = 1
    for m in q:
        Q *= m
    if logn <= 6:
        model = model_hoisted(orc, logn, mext, L, k, alpha, ct, keys, steps, conj)
        for worst in decryption_errors(orc, logn, q, ct, s_ntt, rots, model):
            assert worst < (1 << 24) and worst * (1 << 60) < Q, ("model", worst)
    for worst in decryption_errors(orc, logn, q, ct, s_ntt, rots, got):
        assert worst < (1 << 24) and worst * (1 << 60) < Q, worst


@pytest.mark.parametrize("logn,L", [(5, 3), (11, 2)])
def test_one_digit_one_special_prime_decrypts_like_the_unhoisted_path(eng, orc, logn, L):
    """k = 1, alpha = L: every ciphertext modulus is inside the one digit, so only the special prime's limb is lifted -- the one place
    where the hoisted and the unhoisted path hold different representatives (their words may differ there or not: nothing is asserted
    about that).  Both must decrypt to sigma(c0 + c1 s).  One 50-bit special prime is smaller than the digit, so the noise is not
    that of test_hoisted_rotations_decrypt; its bound, for either representative x of the digit (|x| < Q_d = Q), a key error e
    (|e| <= 8) and a ternary secret:  out0 + out1 s - sigma(c0 + c1 s) = (x * e) / P + r0 + r1 * s  with the ModDown roundings
    |r0|, |r1| <= 1/2, so at most N * 8 * Q / P + (N + 1) / 2 in magnitude -- a 2^-38 fraction of Q."""
    k, alpha = 1, L
    mext = P.P40[:L] + P.P50[:k]
    n, q = 1 << logn, mext[:L]
    rng = SplitMix(5400 + logn)
    rots = [(1, False), (0, True)]
    s_ntt, keys = decryption_setup(orc, rng, logn, mext, L, k, alpha, rots)
    ct = rng.poly((2, L, n), q)
    d_ct, dkeys = eng.to_device(ct[None]), [eng.to_device(key) for key in keys]
    hoisted = eng.to_host(eng.ckks_rotate_hoisted_hks(mext, k, alpha, d_ct, dkeys, [1, 0], [False, True]))[0]
    plain = [eng.to_host(eng.ckks_rotate_hks(mext, k, alpha, d_ct, dkeys[0], 1))[0], eng.to_host(eng.ckks_conjugate_hks(mext, k, alpha, d_ct, dkeys[1]))[0]]
    Q = 1
    for m in q:
        Q *= m
    bound = n * 8 * (Q // mext[L] + 1) + n
    for outs in (hoisted, plain):
        for worst in decryption_errors(orc, logn, q, ct, s_ntt, rots, outs):
            assert worst <= bound, (worst, bound)


# ---- (e) parity level A -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha", [(11, 4, 2, 2), (12, 5, 1, 3)])
def test_hoisted_rotations_at_parity_level_a(eng, logn, L, k, alpha):
    """level A runs the digit stage and the drops on the FP64 kernels: the residues of level B, every word below 2q, range guard quiet"""
    mext = chain(L, k)
    n, q = 1 << logn, mext[:L]
    rng = SplitMix(5500 + logn + L)
    B, steps, conj = 2, [1, 0, 5], [False, True, False]
    ct = rng.poly((B, 2, L, n), q)
    dkeys = [eng.to_device(rng.poly(((L + alpha - 1) // alpha, 2, L + k, n), mext)) for _ in range(3)]
    d_ct = eng.to_device(ct)
    b_words = eng.to_host(eng.ckks_rotate_hoisted_hks(mext, k, alpha, d_ct, dkeys, steps, conj))
    eng.set_parity_level("A")
    try:
        a_words = eng.to_host(eng.ckks_rotate_hoisted_hks(mext, k, alpha, d_ct, dkeys, steps, conj))
        eng.sync()
    finally:
        eng.set_parity_level("B")
    qa = np.array(q, dtype=U)[None, None, None, :, None]
    assert (a_words < 2 * qa).all() and (b_words < 2 * qa).all()
    assert np.array_equal(a_words % qa, b_words % qa)


# ---- (f) argument errors ------------------------------------------------------------------------------------------------------------
def test_hoisted_rejects_bad_arguments_before_enqueuing(eng):
    from hehub_amd import capi
    from hehub_amd.engine import InvalidArgument

    logn, L, k, alpha = 5, 4, 2, 2
    n = 1 << logn
    mext = P.P40[:L] + P.P50[:k]
    nd = (L + alpha - 1) // alpha
    ct, key = eng.empty((1, 2, L, n)).zero_(), eng.empty((nd, 2, L + k, n)).zero_()
    with pytest.raises(InvalidArgument):
        eng.ckks_rotate_hoisted_hks(mext, k, alpha, ct, [], [])                                  # no rotations
    with pytest.raises(InvalidArgument):
        eng.ckks_rotate_hoisted_hks(mext, k, alpha, ct, [key, key], [1, 1 << 17])                # step out of range
    eng.ckks_rotate_hoisted_hks(mext, k, alpha, ct, [key, key], [1, 1 << 17], [False, True])     # ... ignored by a conjugation
    with pytest.raises(InvalidArgument):
        eng.ckks_rotate_hoisted_hks(mext, k, 0, ct, [key], [1])                                  # the limits every hybrid call checks
    with pytest.raises(InvalidArgument):
        eng.ckks_rotate_hoisted_hks(mext, k, 9, ct, [key], [1])
    with pytest.raises(InvalidArgument):
        eng.ckks_rotate_hoisted_hks(mext, 0, alpha, ct, [key], [1])
    with pytest.raises(InvalidArgument):
        eng.ckks_rotate_hoisted_hks(mext, 17, alpha, ct, [key], [1])

    def call(batch, R, steps, keys, d_ct, d_out, k_=k):
        st = (C.c_size_t * max(R, 1))(*steps)
        kp = (capi.P * max(R, 1))(*keys)
        return eng.lib.hp_dev_ckks_rotate_hoisted_hks(eng.h, logn, L, k_, alpha, (capi.u64 * (L + k))(*mext), batch, R, st, None,
                                                      C.c_void_p(d_ct), kp, C.c_void_p(d_out))

    out = eng.empty((1, 2, 2, L, n))
    words = 2 * L * n
    assert call(1, 2, [1, 2], [key.data_ptr(), key.data_ptr()], ct.data_ptr(), out.data_ptr()) == capi.HP_OK
    assert call(0, 1, [1], [key.data_ptr()], ct.data_ptr(), out.data_ptr()) == capi.HP_EINVAL            # empty batch
    assert call(1, 2, [1, 2], [key.data_ptr(), None], ct.data_ptr(), out.data_ptr()) == capi.HP_EINVAL    # NULL key
    assert call(1, 2, [1, 2], [key.data_ptr(), key.data_ptr() + 8], ct.data_ptr(), out.data_ptr()) == capi.HP_EINVAL   # misaligned key
    both = eng.empty((3 * words,))                                                                        # ct inside the output's range
    assert call(1, 2, [1, 2], [key.data_ptr()] * 2, both.data_ptr() + 8 * words, both.data_ptr()) == capi.HP_EINVAL
    assert b"overlaps" in eng.lib.hp_last_error(eng.h)
    assert call(1, 2, [1, 2], [key.data_ptr()] * 2, both.data_ptr(), both.data_ptr() + 8 * (words - 2)) == capi.HP_EINVAL
    assert call(1, 2, [1, 2], [key.data_ptr()] * 2, both.data_ptr(), both.data_ptr() + 8 * words) == capi.HP_OK   # adjacent is fine
    eng.sync()
    # nothing was left half done: a valid call still computes what it should
    plain, hoisted = step0_case(eng, logn, L, k, alpha, seed=5600)
    assert np.array_equal(plain, hoisted)
