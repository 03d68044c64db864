"""hp_dev_ckks_rotate_hoisted_hks: many rotations of one ciphertext, each under its own hybrid key, over ONE digit decomposition.

The digit rows are those of the UNROTATED c1; a rotation moves them (inside the inner product) instead of decomposing the moved
polynomial.  A moved row is the transform of the moved digit read as a signed integer, so on the lifted limbs the words differ from
hp_dev_ckks_rotate_hks's, with the same magnitude bound.  Pinned
  * word for word (level B) by the exact model of tests/test_hks.py, split where the engine splits it: digit rows from the unrotated
    c1, each row moved with the oracle's cycle / involution, then the unchanged inner product and ModDown;
  * against the unhoisted entry point where the two must agree (step 0);
  * by decryption with keys generated here, for the device's words and for the model's."""
import ctypes as C

import numpy as np
import pytest

import params as P
from oracle.pyoracle import SplitMix
from test_hks import below_2q, centred_error, crt, digits_of, keygen

pytestmark = pytest.mark.gpu
U = np.uint64
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


# ---- the model of test_hks.model_switch, in two halves -----------------------------------------------------------------------
def model_digits(orc, logn, mext, L, k, alpha, pt):
    """D [nd][E][n]: the digit rows hks_front builds from pt [L][n] -- pt's own words inside the digit, NTT of the exact ModUp value
    (the non-negative integer behind the digit's strict residues) elsewhere"""
    n, E = 1 << logn, L + k
    digs = digits_of(L, alpha)
    coef = orc.poly_reduce_strict(mext[:L], orc.poly_intt(mext[:L], pt))
    D = np.zeros((len(digs), E, n), dtype=U)
    for d, limbs in enumerate(digs):
        ints = [crt([coef[a][i] for a in limbs], [mext[a] for a in limbs])[0] for i in range(n)]
        for m in range(E):
            if m in limbs:
                D[d, m] = pt[m]
            else:
                D[d, m] = orc.ntt(logn, mext[m], np.array([x % mext[m] for x in ints], dtype=U))
    return D


def model_rest(orc, logn, mext, L, k, D, key):
    """inner product (summed in digit order, one Montgomery reduction), ModDown, * P^-1: D [nd][E][n], key [nd][2][E][n] -> [2][L][n]"""
    n, E = 1 << logn, L + k
    Do, Ko = D.astype(object), key.astype(object)
    ks = np.zeros((2, E, n), dtype=U)
    for h in range(2):
        for m in range(E):
            acc = sum(Do[d, m] * Ko[d, h, m] for d in range(D.shape[0]))
            pairs = np.array([[a & M64, (a >> 64) & M64] for a in acc], dtype=U)
            ks[h, m] = orc.montgomery_128_lazy(mext[m], pairs)
    pm = mext[L:]
    Pprod = 1
    for p in pm:
        Pprod *= p
    out = np.zeros((2, L, n), dtype=U)
    for h in range(2):
        yp = orc.poly_reduce_strict(pm, orc.poly_intt(pm, np.ascontiguousarray(ks[h, L:])))
        ys = [crt([yp[j][i] for j in range(k)], pm)[0] for i in range(n)]
        rem = np.zeros((L, n), dtype=U)
        for i_q in range(L):
            q = mext[i_q]
            rem[i_q] = orc.ntt(logn, q, np.array([(y % q) if y < Pprod // 2 else q - ((Pprod - y) % q) for y in ys], dtype=U))
        diff = orc.poly_sub(mext[:L], np.ascontiguousarray(ks[h, :L]), below_2q(rem, mext[:L]))
        out[h] = orc.poly_rns_scalar_mul(mext[:L], diff, [pow(Pprod % q, -1, q) for q in mext[:L]])
    return out


def move(orc, a, step, conj):
    a = np.ascontiguousarray(a)
    return orc.poly_involution(a) if conj else orc.poly_cycle(a, step)


def model_hoisted(orc, logn, mext, L, k, alpha, ct, keys, steps, conj):
    """ct [2][L][n] -> [R][2][L][n]"""
    q = mext[:L]
    D = model_digits(orc, logn, mext, L, k, alpha, ct[1])
    out = []
    for key, step, cj in zip(keys, steps, conj):
        sw = model_rest(orc, logn, mext, L, k, np.stack([move(orc, D[d], step, cj) for d in range(D.shape[0])]), key)
        out.append(np.stack([orc.poly_add(q, sw[0], move(orc, ct[0], step, cj)), sw[1]]))
    return np.stack(out)


def chain(L, k):
    return P.P40[:L] + (P.P50 + P.P40[L:])[:k]


# ---- (a) the exact model, word for word ---------------------------------------------------------------------------------------
def rotations_of(logn, R):
    """R (step, conj) pairs.  The long list: step 0, a duplicate, N/2 + 1 (the same map as step 1), conjugations at two places"""
    n = 1 << logn
    steps = ([0, 1, 1, n // 2 + 1, 3, 2] + list(range(4, 4 + R)))[:R]
    if R == 2:
        steps = [3, 1]
    if R == 3:
        steps = [5, 1, 0]
    conj = [False] * R
    if R >= 3:
        conj[R - 1] = True
    if R >= 6:
        conj[4] = True
    return steps, conj


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
def step0_case(eng, logn, L, k, alpha, seed=5200, mext=None):
    mext = mext or P.P40[:L] + P.P50[:k]
    n = 1 << logn
    rng = SplitMix(seed + logn)
    ct = rng.poly((2, 2, L, n), mext[:L])
    key = rng.poly(((L + alpha - 1) // alpha, 2, L + k, n), mext)
    d_ct, d_key = eng.to_device(ct), eng.to_device(key)
    plain = eng.to_host(eng.ckks_rotate_hks(mext, k, alpha, d_ct, d_key, 0))
    hoisted = eng.to_host(eng.ckks_rotate_hoisted_hks(mext, k, alpha, d_ct, [d_key], [0]))
    return plain, hoisted[:, 0]


@pytest.mark.parametrize("logn,L,k,alpha", [(5, 4, 2, 2), (11, 3, 2, 2)])
def test_step_zero_is_the_unhoisted_rotation(eng, logn, L, k, alpha):
    plain, hoisted = step0_case(eng, logn, L, k, alpha)
    assert np.array_equal(plain, hoisted)


# ---- (c), (d) decryption --------------------------------------------------------------------------------------------------------
def centred(orc, moduli, poly_ntt):
    """the centred integer coefficients of an NTT-form RNS polynomial"""
    c = orc.poly_reduce_strict(moduli, orc.poly_intt(moduli, poly_ntt))
    vals = []
    for i in range(c.shape[1]):
        x, Q = crt([c[a][i] for a in range(len(moduli))], moduli)
        vals.append(x if x < Q // 2 else x - Q)
    return np.array(vals, dtype=object)


def decryption_setup(orc, rng, logn, mext, L, k, alpha, rots):
    """a ternary secret s, and for every (step, conj) the key that switches sigma(s) back to s, plus the NTT form of s"""
    n, q = 1 << logn, mext[:L]
    s = rng.words(n, 3).astype(np.int64) - 1
    s_ntt = orc.poly_reduce_strict(q, orc.poly_ntt(q, np.stack([(s % m).astype(U) for m in q])))
    keys = []
    for step, cj in rots:
        moved_s = centred(orc, q, move(orc, s_ntt, step, cj))
        keys.append(keygen(orc, rng, logn, mext, L, k, alpha, s, moved_s))
    return s_ntt, keys


def decryption_errors(orc, logn, q, ct, s_ntt, rots, outs):
    """max |coefficient| of out0 + out1 s - sigma_r(c0 + c1 s), per rotation"""
    plain = orc.poly_add(q, ct[0], orc.poly_mul(q, ct[1], s_ntt))
    worst = []
    for (step, cj), out in zip(rots, outs):
        lhs = orc.poly_add(q, np.ascontiguousarray(out[0]), orc.poly_mul(q, np.ascontiguousarray(out[1]), s_ntt))
        worst.append(centred_error(orc, logn, q, orc.poly_sub(q, lhs, move(orc, plain, step, cj))))
    return worst


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
        eng.ckks_rotate_hoisted_hks(mext, k, 0, ct, [key], [1])                                  # the limits of hks_args_ok
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
