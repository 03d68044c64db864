"""hp_dev_ckks_lintrans_bsgs_hks: out = sum_g rot_g( sum_i diag_{g,i} * rot_i(ct) ), babies + giants hybrid keys, the baby results kept
in the extended basis, one ModDown per keyed giant and one at the end.

The contract is on residues (include/hehub_amd.h has it line by line): with D(x) the digit rows of x, unmont = 2^-64,
    baby_i[h][m] = unmont * sum_d move_i(D(c1)[d][m]) * key_i[d][h][m]  + (h == 0, m < L) * (P mod q_m) * move_i(c0[m])
    pre_g[h][m]  = sum_i diag_{g,i}[m] * baby_i[h][m]                         (a NULL diagonal: the term is absent)
    identity giant: acc += pre_g;   others: (u0, u1) = ModDown(pre_g), acc += switch_g(u0, u1) in the extended basis
    out[h]       = ModDown(acc[h]),  every word below 2 q_i
Pinned
  (a) by that model written with Python integers (hks_model.model_bsgs; ModDown is hks_model.model_rest's with the unit "key");
  (b) against hp_dev_ckks_lintrans_hks where one identity giant makes the two the same sum;
  (c) against hp_dev_ckks_lintrans_hks on (diag * c0, diag * c1) for one identity baby and one keyed giant: the giant path alone;
  (d) by decryption with keys generated here, for the device's words and for the model's;
  (h) by the caller's convention diag_{g,i} = rot_g^-1(diag_{g+i}), against the flat call with keys for the composite steps;
  (e) at parity level A, (f) by the workspace, (g) by the argument rejections."""
import ctypes as C

import numpy as np
import pytest

import params as P
from hks_model import (centred_error, chain, decryption_setup, dev, flat_case, model_bsgs, move, random_diagonal, residues_match,
                       rotations_of)
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


# ---- running a case ------------------------------------------------------------------------------------------------------------
def run(eng, mext, k, alpha, d_ct, bkeys, bsteps, bconj, gkeys, gsteps, gconj, diags):
    return eng.to_host(eng.ckks_lintrans_bsgs_hks(mext, k, alpha, d_ct, dev(eng, bkeys), bsteps, dev(eng, gkeys), gsteps,
                                                  [dev(eng, row) for row in diags], bconj, gconj))


def entries(logn, cnt, rng, nd, mext, n, identity):
    """cnt (key, step, conj) entries from rotations_of's list -- step 0 first, a duplicate, N/2 + 1, conjugations -- over a pool of
    at most 5 random keys (any words: the model is about arithmetic).  identity: entry 0 (step 0) has no key; a longer list then also
    has a KEYED step 0 at entry 5."""
    steps, conj = rotations_of(logn, cnt)
    pool = [rng.poly((nd, 2, len(mext), n), mext) for _ in range(min(cnt, 5))]
    keys = [pool[(r * 3 + 1) % len(pool)] for r in range(cnt)]
    if identity:
        at = steps.index(0) if 0 in steps and not conj[steps.index(0)] else 0
        steps[at], conj[at], keys[at] = 0, False, None
        if cnt > 5:
            steps[5], conj[5] = 0, False
    return keys, steps, conj


# ---- (a) the exact model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha,B,nb,ng", [
    (4, 4, 2, 2, 1, 33, 2),    # babies past one table: an identity baby, a keyed step 0, a duplicate step, N/2 + 1, conjugations
    (4, 3, 1, 1, 2, 2, 34),    # giants past one table and past one pre-sum launch: an identity giant, conjugating giants
    (5, 5, 2, 2, 3, 3, 3),     # short last digit, odd batch, a third of the diagonals absent
    (4, 3, 9, 3, 1, 2, 2),     # k > 8, the CRT ModDown
    (11, 3, 2, 2, 2, 2, 2),    # tiled transforms, fused ModDown
    (13, 3, 2, 1, 1, 2, 2),    # several chunks per row
])
def test_bsgs_matches_the_exact_model(eng, orc, logn, L, k, alpha, B, nb, ng):
    mext = chain(L, k)
    n, q = 1 << logn, mext[:L]
    nd = (L + alpha - 1) // alpha
    rng = SplitMix(7100 + logn + L)
    bkeys, bsteps, bconj = entries(logn, nb, rng, nd, mext, n, identity=nb > 3)
    gkeys, gsteps, gconj = entries(logn, ng, rng, nd, mext, n, identity=ng > 3)
    if nb > 3:
        assert bkeys[0] is None and bsteps[5] == 0 and bkeys[5] is not None and n // 2 + 1 in bsteps and any(bconj)
    if ng > 3:
        assert gkeys[0] is None and any(gconj)
    pool = [random_diagonal(rng, mext, n) for _ in range(4)]
    diags = [[pool[(g * nb + i) % 4] for i in range(nb)] for g in range(ng)]
    if (L, nb, ng) == (5, 3, 3):
        for g, i in ((0, 1), (1, 2), (2, 0)):
            diags[g][i] = None
    elif nb * ng > 4:
        for g in range(ng):
            for i in range(nb):
                if (g * nb + i) % 7 == 3 and sum(d is not None for d in diags[g]) > 1:
                    diags[g][i] = None
    ct = np.stack([rng.poly((2, L, n), q) for _ in range(B)])
    got = run(eng, mext, k, alpha, eng.to_device(ct), bkeys, bsteps, bconj, gkeys, gsteps, gconj, diags)
    assert got.shape == (B, 2, L, n)
    for b in range(B):
        exp = model_bsgs(orc, logn, mext, L, k, alpha, ct[b], bkeys, bsteps, bconj, gkeys, gsteps, gconj, diags)
        assert residues_match(got[b], exp, q), b


def test_both_entries_the_identity_is_the_product_with_the_diagonal(eng, orc):
    """(5, 4, 2, 2, 2, 1, 1): P * x goes through ModDown without a remainder, so the residues are those of diag * ct exactly"""
    logn, L, k, alpha, B = 5, 4, 2, 2, 2
    mext = chain(L, k)
    n, q = 1 << logn, mext[:L]
    rng = SplitMix(7150)
    ct = np.stack([rng.poly((2, L, n), q) for _ in range(B)])
    dg = random_diagonal(rng, mext, n)
    got = run(eng, mext, k, alpha, eng.to_device(ct), [None], [0], None, [None], [0], None, [[dg]])
    qcol = np.array(q, dtype=object)[:, None]
    for b in range(B):
        exp = np.stack([dg[:L].astype(object) * ct[b, h].astype(object) % qcol for h in range(2)])
        assert residues_match(got[b], exp, q), b
        assert np.array_equal(model_bsgs(orc, logn, mext, L, k, alpha, ct[b], [None], [0], [False], [None], [0], [False], [[dg]]), exp)


# ---- (b) one identity giant: the flat call ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha", [(5, 4, 2, 2), (11, 3, 2, 2)])
def test_one_identity_giant_is_the_flat_call(eng, logn, L, k, alpha):
    flat, bsgs, lazy = flat_case(eng, logn, L, k, alpha)
    assert lazy and np.array_equal(flat, bsgs)


# ---- (c) one identity baby, one keyed giant: the giant path on its own ---------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha,step,cj", [(5, 4, 2, 2, 3, False), (11, 3, 2, 2, 0, True)])
def test_one_identity_baby_and_one_keyed_giant_is_the_flat_call_on_the_product(eng, logn, L, k, alpha, step, cj):
    """ModDown of P * x has no remainder: the giant switches exactly (diag * c0, diag * c1)"""
    mext = P.P40[:L] + P.P50[:k]
    n, q = 1 << logn, mext[:L]
    rng = SplitMix(7300 + logn)
    ct = rng.poly((2, 2, L, n), q)
    dg = random_diagonal(rng, mext, n)
    d_key = eng.to_device(rng.poly(((L + alpha - 1) // alpha, 2, L + k, n), mext))
    qcol = np.array(q, dtype=object)[:, None]
    prod = (dg[:L].astype(object)[None, None] * ct.astype(object) % qcol).astype(U)
    flat = eng.to_host(eng.ckks_lintrans_hks(mext, k, alpha, eng.to_device(prod), [d_key], [step], [None], [cj]))
    bsgs = eng.to_host(eng.ckks_lintrans_bsgs_hks(mext, k, alpha, eng.to_device(ct), [None], [0], [d_key], [step], [[eng.to_device(dg)]],
                                                  None, [cj]))
    qa = np.array(q, dtype=U)[None, None, :, None]
    assert (bsgs < 2 * qa).all() and np.array_equal(flat % qa, bsgs % qa)


# ---- (d) decryption ----------------------------------------------------------------------------------------------------------------
def ternary_diagonal(orc, rng, mext, n):
    c = rng.words(n, 3).astype(np.int64) - 1
    return int(np.abs(c).sum()), orc.poly_reduce_strict(mext, orc.poly_ntt(mext, np.stack([(c % m).astype(U) for m in mext])))


def decrypt(orc, q, out, s_ntt):
    return orc.poly_add(q, np.ascontiguousarray(out[0]), orc.poly_mul(q, np.ascontiguousarray(out[1]), s_ntt))


def bsgs_decryption_error(orc, logn, q, ct, s_ntt, brots, grots, diags_q, out):
    """max |coefficient| of out0 + out1 s - sum_g sigma_g( sum_i diag_{g,i} * sigma_i(c0 + c1 s) )"""
    plain = decrypt(orc, q, ct, s_ntt)
    babies = [move(orc, plain, step, cj) for step, cj in brots]
    want = None
    for (step, cj), row in zip(grots, diags_q):
        inner = None
        for bb, dg in zip(babies, row):
            if dg is not None:
                term = orc.poly_mul(q, np.ascontiguousarray(dg), bb)
                inner = term if inner is None else orc.poly_add(q, inner, term)
        outer = move(orc, inner, step, cj)
        want = outer if want is None else orc.poly_add(q, want, outer)
    return centred_error(orc, logn, q, orc.poly_sub(q, decrypt(orc, q, out, s_ntt), want))


def within(worst, weight, Q):
    """test_lintrans_decrypts' bound per unit of weight"""
    return worst < weight * (1 << 24) and worst * (1 << 60) < weight * Q


@pytest.mark.parametrize("logn,L,k,alpha", [(5, 4, 2, 2), (6, 6, 3, 3), (11, 4, 2, 2)])
def test_bsgs_decrypts(eng, orc, logn, L, k, alpha):
    """Diagonals with coefficients in {-1, 0, 1}.  The error of the result is
        sum_g sigma_g( sum_i diag_{g,i} * e_i ) + sum_{keyed g} ( e'_g + sigma_g(rounding_g) ) + the last rounding
    with e_i the key-switch noise of baby i (none for the identity) and e'_g that of giant g, each under test_lintrans_decrypts'
    per-rotation bound (the noise of a hybrid switch does not depend on the size of what is switched: the digits are bounded by their
    moduli), sigma_g a signed permutation, and a product with a polynomial of l1 norm w growing a coefficient bound by at most w.
    So that bound holds with the weight (l1 weight of all present diagonals + the number of keyed giants); the inner ModDown's
    rounding, at most (1 + |s|_1) / 2 per giant, is far inside a unit of it.  Below N = 128 the model is held to the same bound."""
    mext = P.P40[:L] + P.P50[:k]
    n, q = 1 << logn, mext[:L]
    rng = SplitMix(7400 + logn + L)
    brots, grots = [(0, False), (1, False), (0, True)], [(0, False), (3, False), (2, False)]
    s_ntt, keys = decryption_setup(orc, rng, logn, mext, L, k, alpha, brots + grots)
    bkeys, gkeys = keys[:3], keys[3:]
    bkeys[0] = None      # the identity baby; giant 0 is a KEYED step 0
    ct = rng.poly((2, L, n), q)
    made = [[ternary_diagonal(orc, rng, mext, n) for _ in brots] for _ in grots]
    diags = [[d for _, d in row] for row in made]
    diags[1][2] = None
    weight = sum(w for g, row in enumerate(made) for i, (w, _) in enumerate(row) if diags[g][i] is not None) + len(grots)
    bsteps, bconj = [r[0] for r in brots], [r[1] for r in brots]
    gsteps, gconj = [r[0] for r in grots], [r[1] for r in grots]
    got = run(eng, mext, k, alpha, eng.to_device(ct[None]), bkeys, bsteps, bconj, gkeys, gsteps, gconj, diags)[0]
    Q = 1
    for m in q:
        Q *= m
    diags_q = [[None if d is None else d[:L] for d in row] for row in diags]
    if logn <= 6:
        model = model_bsgs(orc, logn, mext, L, k, alpha, ct, bkeys, bsteps, bconj, gkeys, gsteps, gconj, diags)
        worst = bsgs_decryption_error(orc, logn, q, ct, s_ntt, brots, grots, diags_q, model.astype(U))
        print(f"logn={logn}: the model's worst decryption error {worst}, weight {weight}")
        assert within(worst, weight, Q), ("model", worst, weight)
    worst = bsgs_decryption_error(orc, logn, q, ct, s_ntt, brots, grots, diags_q, got)
    print(f"logn={logn}: worst decryption error {worst}, weight {weight}")
    assert within(worst, weight, Q), (worst, weight)


# ---- (h) the caller's convention ----------------------------------------------------------------------------------------------------
def test_a_matrix_by_its_diagonals_agrees_with_the_flat_call(eng, orc):
    """diag_r, r = g + i over giants {0, 3} x babies {0, 1, 2}: the flat call with keys for the six composite steps against the BSGS
    call with diag_{g,i} = rot_g^-1(diag_{g+i}).  The inverse step is found with the oracle's poly_cycle, not assumed."""
    logn, L, k, alpha = 5, 4, 2, 2
    mext = P.P40[:L] + P.P50[:k]
    n, q = 1 << logn, mext[:L]
    rng = SplitMix(7800)
    bsteps, gsteps = [0, 1, 2], [0, 3]
    flat_steps = [g + i for g in gsteps for i in bsteps]
    rots = [(s, False) for s in flat_steps + bsteps + gsteps]
    s_ntt, keys = decryption_setup(orc, rng, logn, mext, L, k, alpha, rots)
    fkeys, bkeys, gkeys = keys[:6], keys[6:9], keys[9:]
    bkeys[0] = gkeys[0] = None
    probe = rng.poly((L + k, n), mext)
    inverse = {}
    for g in gsteps:
        inverse[g] = next(t for t in range(n) if np.array_equal(orc.poly_cycle(orc.poly_cycle(probe, g), t), probe))
    assert inverse[0] == 0 and inverse[3] != 0 and not np.array_equal(orc.poly_cycle(probe, 3), probe)
    made = [ternary_diagonal(orc, rng, mext, n) for _ in flat_steps]
    fdiags = [d for _, d in made]
    weight = sum(w for w, _ in made)
    bdiags = [[np.ascontiguousarray(orc.poly_cycle(fdiags[gi * 3 + i], inverse[g])) for i in range(3)] for gi, g in enumerate(gsteps)]
    ct = rng.poly((2, L, n), q)
    d_ct = eng.to_device(ct[None])
    flat = eng.to_host(eng.ckks_lintrans_hks(mext, k, alpha, d_ct, dev(eng, fkeys), flat_steps, dev(eng, fdiags)))[0]
    bsgs = run(eng, mext, k, alpha, d_ct, bkeys, bsteps, None, gkeys, gsteps, None, bdiags)[0]
    Q = 1
    for m in q:
        Q *= m
    worst = centred_error(orc, logn, q, orc.poly_sub(q, decrypt(orc, q, flat, s_ntt), decrypt(orc, q, bsgs, s_ntt)))
    both = weight + (weight + 1)      # the flat call's weight + the BSGS call's (the same diagonals, moved, + one keyed giant)
    print(f"worst difference of the two decryptions {worst}, weights {weight} + {weight + 1}")
    assert within(worst, both, Q), (worst, both)
    # and the plaintext is the matrix's: sum_r diag_r * sigma_r(c0 + c1 s)
    plain = decrypt(orc, q, ct, s_ntt)
    want = None
    for s, d in zip(flat_steps, fdiags):
        term = orc.poly_mul(q, np.ascontiguousarray(d[:L]), move(orc, plain, s, False))
        want = term if want is None else orc.poly_add(q, want, term)
    worst = centred_error(orc, logn, q, orc.poly_sub(q, decrypt(orc, q, bsgs, s_ntt), want))
    assert within(worst, weight + 1, Q), (worst, weight + 1)


# ---- (e) parity level A ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha", [(11, 4, 2, 2), (12, 5, 1, 3)])
def test_bsgs_at_parity_level_a(eng, logn, L, k, alpha):
    """level A runs the digit stages and the drops on the FP64 kernels: the residues of level B, every word below 2q, range guard quiet"""
    mext = chain(L, k)
    n, q = 1 << logn, mext[:L]
    rng = SplitMix(7500 + logn + L)
    B = 2
    key = lambda: eng.to_device(rng.poly(((L + alpha - 1) // alpha, 2, L + k, n), mext))
    dg = lambda: eng.to_device(random_diagonal(rng, mext, n))
    bkeys, bsteps, bconj = [None, key(), key()], [0, 1, 0], [False, False, True]
    gkeys, gsteps, gconj = [key(), None, key()], [4, 0, 0], [False, False, True]
    diags = [[dg(), None, dg()], [dg(), dg(), None], [None, dg(), dg()]]
    d_ct = eng.to_device(rng.poly((B, 2, L, n), q))
    call = lambda: eng.to_host(eng.ckks_lintrans_bsgs_hks(mext, k, alpha, d_ct, bkeys, bsteps, gkeys, gsteps, diags, bconj, gconj))
    b_words = call()
    eng.set_parity_level("A")
    try:
        a_words = call()
        eng.sync()   # (HP_ERANGE here: a level-A kernel was handed a word outside its range)
    finally:
        eng.set_parity_level("B")
    qa = np.array(q, dtype=U)[None, None, :, None]
    assert (a_words < 2 * qa).all() and (b_words < 2 * qa).all()
    assert np.array_equal(a_words % qa, b_words % qa)


# ---- (f) the workspace follows the shape alone ---------------------------------------------------------------------------------------
def test_workspace_is_stable_across_steps_keys_and_absent_diagonals(eng):
    logn, L, k, alpha, B = 11, 3, 2, 2, 2
    mext = chain(L, k)
    n = 1 << logn
    rng = SplitMix(7600)
    d_ct = eng.to_device(rng.poly((B, 2, L, n), mext[:L]))
    k1, k2 = (eng.to_device(rng.poly(((L + alpha - 1) // alpha, 2, L + k, n), mext)) for _ in range(2))
    d1, d2 = (eng.to_device(random_diagonal(rng, mext, n)) for _ in range(2))
    eng.sync()
    eng.release_workspace()
    eng.ckks_lintrans_bsgs_hks(mext, k, alpha, d_ct, [None, k1, k1], [0, 1, 2], [k1, k2], [3, 6], [[d1, d1, d1], [d2, d1, d2]])
    eng.sync()
    size, gen = eng.workspace_bytes(), eng.lib.hp_ctx_workspace_generation(eng.h)
    eng.ckks_lintrans_bsgs_hks(mext, k, alpha, d_ct, [k2, k2, k1], [5, 0, 7], [None, k1], [0, 1], [[None, d2, None], [d1, None, None]],
                               [False, True, False], [False, True])
    eng.sync()
    assert size > 0 and eng.workspace_bytes() == size and eng.lib.hp_ctx_workspace_generation(eng.h) == gen


# ---- (g) argument errors ------------------------------------------------------------------------------------------------------------------
def test_bsgs_rejects_bad_arguments_before_enqueuing(eng):
    from hehub_amd import capi

    logn, L, k, alpha = 5, 4, 2, 2
    n = 1 << logn
    mext = P.P40[:L] + P.P50[:k]
    nd = (L + alpha - 1) // alpha
    ct, key = eng.empty((1, 2, L, n)).zero_(), eng.empty((nd, 2, L + k, n)).zero_()
    diag = eng.empty((L + k, n)).zero_()
    out = eng.empty((1, 2, L, n))
    kp, dp, cp, op = key.data_ptr(), diag.data_ptr(), ct.data_ptr(), out.data_ptr()

    def table(cnt, steps, conj, keys):
        return (cnt, (C.c_size_t * max(cnt, 1))(*steps), (C.c_ubyte * max(cnt, 1))(*conj) if conj is not None else None,
                (capi.P * max(cnt, 1))(*keys))

    def call(batch=1, babies=(2, [0, 1], None, [None, kp]), giants=(2, [0, 2], None, [None, kp]), diags=(dp, None, dp, dp), d_ct=cp,
             d_out=op, k_=k, alpha_=alpha):
        dd = (capi.P * max(len(diags), 1))(*diags)
        return eng.lib.hp_dev_ckks_lintrans_bsgs_hks(eng.h, logn, L, k_, alpha_, (capi.u64 * (L + k))(*mext), batch, *table(*babies),
                                                     *table(*giants), dd, C.c_void_p(d_ct), C.c_void_p(d_out))

    assert call() == capi.HP_OK
    for bad in (dict(alpha_=0), dict(alpha_=9), dict(k_=0), dict(k_=17), dict(batch=0)):                   # the limits of hp_dev_hks_switch
        assert call(**bad) == capi.HP_EINVAL, bad
    assert call(babies=(0, [], None, []), diags=()) == capi.HP_EINVAL                                      # no babies
    assert call(giants=(0, [], None, []), diags=()) == capi.HP_EINVAL                                      # no giants
    assert call(babies=(2, [0, 1 << 17], None, [None, kp])) == capi.HP_EINVAL                              # step out of range, baby
    assert call(giants=(2, [0, 1 << 17], None, [None, kp])) == capi.HP_EINVAL                              # ... giant
    assert call(giants=(2, [0, 1 << 17], [0, 1], [None, kp])) == capi.HP_OK                                # ... ignored by a conjugation
    assert call(babies=(2, [0, 1], None, [None, None])) == capi.HP_EINVAL                                  # NULL key, step 1
    assert call(giants=(2, [0, 2], None, [None, None])) == capi.HP_EINVAL
    assert call(babies=(2, [0, 1], [1, 0], [None, kp])) == capi.HP_EINVAL                                  # NULL key on a conjugation at step 0
    assert b"identity" in eng.lib.hp_last_error(eng.h)
    assert call(giants=(2, [0, 2], [1, 0], [None, kp])) == capi.HP_EINVAL
    assert call(babies=(2, [0, 0], None, [None, kp])) == capi.HP_OK                                        # a keyed step 0 is fine
    assert call(babies=(2, [0, 1], None, [None, kp + 8])) == capi.HP_EINVAL                                # misaligned key
    assert call(giants=(2, [0, 2], None, [None, kp + 8])) == capi.HP_EINVAL
    assert call(diags=(dp, None, dp + 8, dp)) == capi.HP_EINVAL                                            # misaligned diagonal
    assert call(diags=(dp, dp, None, None)) == capi.HP_EINVAL                                              # a giant without a diagonal
    assert call(diags=(None, None, dp, dp)) == capi.HP_EINVAL
    words = 2 * L * n
    both = eng.empty((2 * words,))
    base = both.data_ptr()
    assert call(d_ct=base, d_out=base) == capi.HP_EINVAL                                                   # in place
    assert b"overlaps" in eng.lib.hp_last_error(eng.h)
    assert call(d_ct=base, d_out=base + 8 * (words - 2)) == capi.HP_EINVAL                                 # the output's head on the input's tail
    assert call(d_ct=base + 8 * 2, d_out=base) == capi.HP_EINVAL                                           # and the other way round
    assert call(d_ct=base, d_out=base + 8 * words) == capi.HP_OK                                           # adjacent is fine
    eng.sync()
    # nothing was left half done: a valid call still computes what it should
    flat, bsgs, lazy = flat_case(eng, logn, L, k, alpha, seed=7700)
    assert lazy and np.array_equal(flat, bsgs)
