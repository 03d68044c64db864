"""hp_dev_ckks_lintrans_hks: out = sum_r diag_r * rot_r(ct), one hybrid key per rotation, the weighted sum formed in the extended basis
before ONE ModDown.

The contract is on residues:
    acc[h][m] = sum_r diag_r[m] * ( sum_d move_r(D[d][m]) * key_r[d][h][m] )           for all L + k moduli m
    out[h]    = ModDown(acc[h]) + (h == 0) * sum_r diag_r[:L] * move_r(c0)              (mod each q_i), every word below 2 q_i
with D the digit rows of the unrotated c1 (hks_model.model_digits), the keys in Montgomery form as for every hybrid call
(the inner sum carries their 2^-64) and the diagonals plain words.  Pinned
  (a) by that model written with Python integers (hks_model.model_lintrans), ModDown being hks_model.model_rest's;
  (b) against hp_dev_ckks_rotate_hoisted_hks where the two must agree (one rotation, no diagonal);
  (c) against the weighted sum of the hoisted call's results: one rounding against R;
  (d) by decryption with keys generated here, for the device's words and for the model's;
  (e) at parity level A, (f) by the size of the workspace, (g) by the argument rejections."""
import ctypes as C

import numpy as np
import pytest

import params as P
from hks_model import (centred_error, chain, decryption_setup, model_lintrans, move, random_diagonal, residues_match, rotations_of,
                       single_case)
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


# ---- (a) the exact model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha,B,R", [
    (4, 4, 2, 2, 1, 33),    # more rotations than one table: the accumulate-across-launches path; step 0, a duplicate, N/2 + 1, two conjugations
    (5, 5, 2, 2, 3, 3),     # short last digit, odd batch
    (5, 3, 1, 1, 2, 2),     # every digit one limb, one special prime
    (4, 3, 9, 3, 1, 2),     # k > 8, the CRT ModDown
    (11, 3, 2, 2, 2, 3),    # tiled transforms, fused ModDown
    (13, 3, 2, 1, 1, 2),    # several chunks per row
    (4, 2, 1, 1, 34, 2),    # a large batch
])
def test_lintrans_matches_the_exact_model(eng, orc, logn, L, k, alpha, B, R):
    mext = chain(L, k)
    n, q = 1 << logn, mext[:L]
    nd = (L + alpha - 1) // alpha
    rng = SplitMix(6100 + logn + L)
    steps, conj = rotations_of(logn, R)
    ct = np.stack([rng.poly((2, L, n), q) for _ in range(B)])
    nkeys = min(R, 5)
    keys = [rng.poly((nd, 2, L + k, n), mext) for _ in range(nkeys)]          # any words: the model is about arithmetic
    dkeys = [eng.to_device(key) for key in keys]
    pool = [random_diagonal(rng, mext, n), None] + [random_diagonal(rng, mext, n) for _ in range(3)]
    dpool = [None if d is None else eng.to_device(d) for d in pool]
    which = [(r * 3 + 1) % nkeys for r in range(R)]
    wd = [(r * 2 + 1) % len(pool) for r in range(R)]                         # rotation 0 has no diagonal
    got = eng.to_host(eng.ckks_lintrans_hks(mext, k, alpha, eng.to_device(ct), [dkeys[w] for w in which], steps, [dpool[w] for w in wd], conj))
    assert got.shape == (B, 2, L, n)
    for b in range(B):
        exp = model_lintrans(orc, logn, mext, L, k, alpha, ct[b], [keys[w] for w in which], steps, conj, [pool[w] for w in wd])
        assert residues_match(got[b], exp, q), b


# ---- (b) one rotation without a diagonal is the hoisted rotation ---------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha", [(5, 4, 2, 2), (11, 3, 2, 2)])
def test_one_rotation_without_a_diagonal_is_the_hoisted_rotation(eng, logn, L, k, alpha):
    hoisted, lin, lazy = single_case(eng, logn, L, k, alpha)
    assert lazy and np.array_equal(hoisted, lin)


# ---- (c) one rounding against R ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha,R", [(5, 4, 2, 2, 4), (11, 3, 2, 2, 3)])
def test_one_rounding_against_one_per_rotation(eng, orc, logn, L, k, alpha, R):
    """Integer constants c_r as diagonals (the NTT form of a constant is its residue in every slot).  sum_r c_r hoisted_r and the
    transform differ by (rem - sum_r c_r rem_r) / P, rem_r and rem the centred remainders of the ModDowns (at most P/2 each; the exact
    parts cancel modulo Q P): at most (sum |c_r| + 1) / 2 per coefficient, on both polynomials."""
    mext = P.P40[:L] + P.P50[:k]
    n, q = 1 << logn, mext[:L]
    rng = SplitMix(6300 + logn)
    consts = [int(c) - 8 for c in rng.words(R, 17)]
    steps, conj = [1, 5, 0, 2][:R], [False] * R
    conj[R - 1] = True
    ct = rng.poly((1, 2, L, n), q)
    d_ct = eng.to_device(ct)
    dkeys = [eng.to_device(rng.poly(((L + alpha - 1) // alpha, 2, L + k, n), mext)) for _ in range(R)]
    diags = [eng.to_device(np.repeat(np.array([c % m for m in mext], dtype=U)[:, None], n, axis=1)) for c in consts]
    hoisted = eng.to_host(eng.ckks_rotate_hoisted_hks(mext, k, alpha, d_ct, dkeys, steps, conj))[0].astype(object)
    lin = eng.to_host(eng.ckks_lintrans_hks(mext, k, alpha, d_ct, dkeys, steps, diags, conj))[0].astype(object)
    qcol = np.array(q, dtype=object)[:, None]
    bound2 = sum(abs(c) for c in consts) + 1
    for h in range(2):
        diff = ((sum(c * hoisted[r, h] for r, c in enumerate(consts)) - lin[h]) % qcol).astype(U)
        worst = centred_error(orc, logn, q, diff)
        print(f"logn={logn} poly {h}: constants {consts}, worst |difference| {worst}, bound {bound2}/2")
        assert 2 * worst <= bound2, (h, worst, consts)


# ---- (d) decryption ----------------------------------------------------------------------------------------------------------------
def lintrans_decryption_error(orc, logn, q, ct, s_ntt, rots, diags_q, out):
    """max |coefficient| of out0 + out1 s - sum_r diag_r * sigma_r(c0 + c1 s)"""
    plain = orc.poly_add(q, ct[0], orc.poly_mul(q, ct[1], s_ntt))
    want = None
    for (step, cj), dg in zip(rots, diags_q):
        term = orc.poly_mul(q, np.ascontiguousarray(dg), move(orc, plain, step, cj))
        want = term if want is None else orc.poly_add(q, want, term)
    lhs = orc.poly_add(q, np.ascontiguousarray(out[0]), orc.poly_mul(q, np.ascontiguousarray(out[1]), s_ntt))
    return centred_error(orc, logn, q, orc.poly_sub(q, lhs, want))


@pytest.mark.parametrize("logn,L,k,alpha", [(5, 4, 2, 2), (6, 6, 3, 3), (11, 4, 2, 2)])
def test_lintrans_decrypts(eng, orc, logn, L, k, alpha):
    """Diagonals with coefficients in {-1, 0, 1}: out0 + out1 s = sum_r diag_r sigma_r(c0 + c1 s) up to the key-switch noise of every
    rotation multiplied by its diagonal -- test_hoisted_rotations_decrypt's bound per rotation times the diagonals' l1 weight (a product
    with a polynomial of l1 norm w grows a coefficient bound by at most w).  Below N = 128 the model is held to the same bound."""
    mext = P.P40[:L] + P.P50[:k]
    n, q = 1 << logn, mext[:L]
    rng = SplitMix(6400 + logn + L)
    rots = [(1, False), (3, False), (0, True)]
    s_ntt, keys = decryption_setup(orc, rng, logn, mext, L, k, alpha, rots)
    ct = rng.poly((2, L, n), q)
    coefs = [rng.words(n, 3).astype(np.int64) - 1 for _ in rots]
    weight = int(sum(np.abs(c).sum() for c in coefs))
    diags = [orc.poly_reduce_strict(mext, orc.poly_ntt(mext, np.stack([(c % m).astype(U) for m in mext]))) for c in coefs]
    steps, conj = [r[0] for r in rots], [r[1] for r in rots]
    got = eng.to_host(eng.ckks_lintrans_hks(mext, k, alpha, eng.to_device(ct[None]), [eng.to_device(key) for key in keys], steps,
                                            [eng.to_device(d) for d in diags], conj))[0]
    Q = 1
    for m in q:
        Q *= m
    assert weight > 0
    diags_q = [d[:L] for d in diags]
    if logn <= 6:
        model = model_lintrans(orc, logn, mext, L, k, alpha, ct, keys, steps, conj, diags)
        worst = lintrans_decryption_error(orc, logn, q, ct, s_ntt, rots, diags_q, model.astype(U))
        assert worst < weight * (1 << 24) and worst * (1 << 60) < weight * Q, ("model", worst, weight)
    worst = lintrans_decryption_error(orc, logn, q, ct, s_ntt, rots, diags_q, got)
    print(f"logn={logn}: worst decryption error {worst}, l1 weight {weight}")
    assert worst < weight * (1 << 24) and worst * (1 << 60) < weight * Q, (worst, weight)


# ---- (e) parity level A ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha", [(11, 4, 2, 2), (12, 5, 1, 3)])
def test_lintrans_at_parity_level_a(eng, logn, L, k, alpha):
    """level A runs the digit stage and the drops on the FP64 kernels: the residues of level B, every word below 2q, range guard quiet"""
    mext = chain(L, k)
    n, q = 1 << logn, mext[:L]
    rng = SplitMix(6500 + logn + L)
    B, steps, conj = 2, [1, 0, 5], [False, True, False]
    ct = rng.poly((B, 2, L, n), q)
    dkeys = [eng.to_device(rng.poly(((L + alpha - 1) // alpha, 2, L + k, n), mext)) for _ in range(3)]
    diags = [eng.to_device(random_diagonal(rng, mext, n)), None, eng.to_device(random_diagonal(rng, mext, n))]
    d_ct = eng.to_device(ct)
    b_words = eng.to_host(eng.ckks_lintrans_hks(mext, k, alpha, d_ct, dkeys, steps, diags, conj))
    eng.set_parity_level("A")
    try:
        a_words = eng.to_host(eng.ckks_lintrans_hks(mext, k, alpha, d_ct, dkeys, steps, diags, conj))
        eng.sync()   # (HP_ERANGE here: a level-A kernel was handed a word outside its range)
    finally:
        eng.set_parity_level("B")
    qa = np.array(q, dtype=U)[None, None, :, None]
    assert (a_words < 2 * qa).all() and (b_words < 2 * qa).all()
    assert np.array_equal(a_words % qa, b_words % qa)


# ---- (f) the workspace does not depend on the number of rotations ------------------------------------------------------------------------
def test_workspace_does_not_grow_with_the_rotations(eng):
    logn, L, k, alpha, B = 11, 3, 2, 2, 2
    mext = chain(L, k)
    n = 1 << logn
    rng = SplitMix(6600)
    d_ct = eng.to_device(rng.poly((B, 2, L, n), mext[:L]))
    d_key = eng.to_device(rng.poly(((L + alpha - 1) // alpha, 2, L + k, n), mext))
    d_diag = eng.to_device(random_diagonal(rng, mext, n))
    eng.sync()
    eng.release_workspace()
    eng.ckks_lintrans_hks(mext, k, alpha, d_ct, [d_key] * 2, [1, 2], [d_diag, None])
    small = eng.workspace_bytes()
    eng.ckks_lintrans_hks(mext, k, alpha, d_ct, [d_key] * 40, list(range(40)), [d_diag] * 40)
    eng.sync()
    assert small > 0 and eng.workspace_bytes() == small


# ---- (g) argument errors ------------------------------------------------------------------------------------------------------------------
def test_lintrans_rejects_bad_arguments_before_enqueuing(eng):
    from hehub_amd import capi

    logn, L, k, alpha = 5, 4, 2, 2
    n = 1 << logn
    mext = P.P40[:L] + P.P50[:k]
    nd = (L + alpha - 1) // alpha
    ct, key = eng.empty((1, 2, L, n)).zero_(), eng.empty((nd, 2, L + k, n)).zero_()
    diag = eng.empty((L + k, n)).zero_()
    out = eng.empty((1, 2, L, n))
    kp, dp = key.data_ptr(), diag.data_ptr()

    def call(batch, R, steps, keys, diags, d_ct, d_out, conj=None, k_=k, alpha_=alpha):
        st = (C.c_size_t * max(R, 1))(*steps)
        kk = (capi.P * max(R, 1))(*keys)
        dd = (capi.P * max(R, 1))(*diags)
        cj = (C.c_ubyte * max(R, 1))(*conj) if conj is not None else None
        return eng.lib.hp_dev_ckks_lintrans_hks(eng.h, logn, L, k_, alpha_, (capi.u64 * (L + k))(*mext), batch, R, st, cj, C.c_void_p(d_ct), kk,
                                                dd, C.c_void_p(d_out))

    good = (1, 2, [1, 2], [kp, kp], [dp, None], ct.data_ptr(), out.data_ptr())
    assert call(*good) == capi.HP_OK
    for bad in (dict(alpha_=0), dict(alpha_=9), dict(k_=0), dict(k_=17)):                                   # the limits every hybrid call checks
        assert call(*good, **bad) == capi.HP_EINVAL, bad
    assert call(0, 2, [1, 2], [kp, kp], [dp, None], ct.data_ptr(), out.data_ptr()) == capi.HP_EINVAL          # empty batch
    assert call(1, 0, [], [], [], ct.data_ptr(), out.data_ptr()) == capi.HP_EINVAL                            # no rotations
    assert call(1, 2, [1, 1 << 17], [kp, kp], [dp, None], ct.data_ptr(), out.data_ptr()) == capi.HP_EINVAL    # step out of range
    assert call(1, 2, [1, 1 << 17], [kp, kp], [dp, None], ct.data_ptr(), out.data_ptr(), conj=[0, 1]) == capi.HP_OK   # ... ignored by a conjugation
    assert call(1, 2, [1, 2], [kp, None], [dp, None], ct.data_ptr(), out.data_ptr()) == capi.HP_EINVAL        # NULL key
    assert call(1, 2, [1, 2], [kp, kp + 8], [dp, None], ct.data_ptr(), out.data_ptr()) == capi.HP_EINVAL      # misaligned key
    assert call(1, 2, [1, 2], [kp, kp], [dp, dp + 8], ct.data_ptr(), out.data_ptr()) == capi.HP_EINVAL        # misaligned diagonal
    words = 2 * L * n
    both = eng.empty((2 * words,))
    base = both.data_ptr()
    assert call(1, 2, [1, 2], [kp, kp], [dp, None], base, base) == capi.HP_EINVAL                             # in place
    assert b"overlaps" in eng.lib.hp_last_error(eng.h)
    assert call(1, 2, [1, 2], [kp, kp], [dp, None], base, base + 8 * (words - 2)) == capi.HP_EINVAL           # the output's head on the input's tail
    assert call(1, 2, [1, 2], [kp, kp], [dp, None], base + 8 * 2, base) == capi.HP_EINVAL                     # and the other way round
    assert call(1, 2, [1, 2], [kp, kp], [dp, None], base, base + 8 * words) == capi.HP_OK                     # adjacent is fine
    eng.sync()
    # nothing was left half done: a valid call still computes what it should
    hoisted, lin, lazy = single_case(eng, logn, L, k, alpha, seed=6700)
    assert lazy and np.array_equal(hoisted, lin)
