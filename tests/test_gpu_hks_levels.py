"""One top-level hybrid key set at every level: the _at entry points (include/hehub_amd.h) behind the Engine's key_L0 keyword.

The contract is word equality, at either parity level, with the plain call on the extracted sub-key (tests/hks_levels.py: sub_key,
sub_diag) -- the plain calls themselves are pinned by the exact model in the other hybrid tests.  Keys are random words unless
stated: the claim is about addressing.  A top key here is a level key planted into a top-shaped block of words from ANOTHER random
stream (embed_key): the rows and digits the level must not read hold valid residues of other moduli, so a kernel that reads row m
where it should read row km = m + (m >= L ? key_L0 - L : 0) gets wrong words, not shifted ones.

Shapes (logn, key_L0, L, k, alpha): the smallest at which the addressing can go wrong, see SHAPES."""
import numpy as np
import pytest

import moduli as M
from gpu_words import dev_i64
from hks_levels import embed_diag, embed_key, level_chain, level_digits, level_rows, sub_key, top_chain
from hks_model import centred_error, random_diagonal, rotations_of
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64

SHAPES = [
    (4, 4, 4, 2, 2),    # the top level itself
    (5, 5, 3, 2, 2),    # the level's last digit is partial where the top's is full, and the top has one digit more
    (4, 6, 2, 3, 3),    # L < alpha, one digit of two
    (4, 7, 1, 1, 1),    # L = 1
    (5, 8, 5, 2, 8),    # a single digit
    (4, 5, 3, 9, 3),    # k > 8: ModDown by one composition per modulus
    (11, 5, 3, 2, 2),   # the fused-drop path
]
SMALL, FUSED = (5, 5, 3, 2, 2), (11, 5, 3, 2, 2)


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


class Case:
    """the two chains of a shape, and random keys / diagonals in their two forms: at the level, and planted at the top"""

    def __init__(self, seed, logn, key_L0, L, k, alpha):
        self.logn, self.key_L0, self.L, self.k, self.alpha, self.n = logn, key_L0, L, k, alpha, 1 << logn
        self.mtop = top_chain(key_L0, k)
        self.mext = level_chain(self.mtop, key_L0, L, k)
        self.q = self.mext[:L]
        self.rng, self.fill = SplitMix(seed + logn + 16 * key_L0), SplitMix(seed + 7777 + logn)

    def key(self, eng):
        """(device top key, device level key)"""
        c = self
        level = c.rng.poly((level_digits(c.L, c.alpha), 2, c.L + c.k, c.n), c.mext)
        fill = c.fill.poly((level_digits(c.key_L0, c.alpha), 2, c.key_L0 + c.k, c.n), c.mtop)
        return eng.to_device(embed_key(fill, level, c.key_L0, c.L, c.k, c.alpha)), eng.to_device(level)

    def diag(self, eng):
        c = self
        level = random_diagonal(c.rng, c.mext, c.n)
        return eng.to_device(embed_diag(random_diagonal(c.fill, c.mtop, c.n), level, c.key_L0, c.L, c.k)), eng.to_device(level)


def at_both_levels(eng, run):
    """run() -> [(got, expected), ...] as host arrays, at parity level B and at parity level A; every pair must agree word for word"""
    for level in ("B", "A"):
        eng.set_parity_level(level)
        try:
            pairs = run()
            eng.sync()
        finally:
            eng.set_parity_level("B")
        assert pairs
        for i, (got, exp) in enumerate(pairs):
            assert got.shape == exp.shape and np.array_equal(got, exp), (level, i)


# ---- 1. the plain switch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,key_L0,L,k,alpha", SHAPES)
def test_switch_with_a_top_level_key(eng, logn, key_L0, L, k, alpha):
    c = Case(9100, logn, key_L0, L, k, alpha)
    d_pt = eng.to_device(c.rng.poly((2, L, c.n), c.q))
    d_top, d_sub = c.key(eng)

    def run():
        got = eng.to_host(eng.hks_switch(c.mext, k, alpha, d_pt, d_top, key_L0=key_L0))
        pairs = [(got, eng.to_host(eng.hks_switch(c.mext, k, alpha, d_pt, d_sub)))]
        if key_L0 == L:   # the plain call on the same key
            pairs.append((got, eng.to_host(eng.hks_switch(c.mext, k, alpha, d_pt, d_top))))
        return pairs

    at_both_levels(eng, run)


# ---- 2. rotate, conjugate, hoisted rotations -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,key_L0,L,k,alpha", [SMALL, FUSED])
def test_rotations_with_top_level_keys(eng, logn, key_L0, L, k, alpha):
    c = Case(9200, logn, key_L0, L, k, alpha)
    steps, conj = rotations_of(logn, 6)   # step 0, a duplicate, N/2 + 1, two conjugations
    assert 0 in [s for s, cj in zip(steps, conj) if not cj] and any(conj)
    d_ct = eng.to_device(c.rng.poly((3, 2, L, c.n), c.q))   # batch 3: the two-ciphertexts-per-thread kernels have a tail
    keys = [c.key(eng) for _ in steps]
    tops, subs = [t for t, _ in keys], [s for _, s in keys]
    m = c.mext

    def run():
        pairs = [(eng.to_host(eng.ckks_rotate_hoisted_hks(m, k, alpha, d_ct, tops, steps, conj, key_L0=key_L0)),
                  eng.to_host(eng.ckks_rotate_hoisted_hks(m, k, alpha, d_ct, subs, steps, conj)))]
        for r in (0, 3, 4):   # step 0, a step beyond N/2, a conjugation
            if conj[r]:
                pairs.append((eng.to_host(eng.ckks_conjugate_hks(m, k, alpha, d_ct, tops[r], key_L0=key_L0)),
                              eng.to_host(eng.ckks_conjugate_hks(m, k, alpha, d_ct, subs[r]))))
            else:
                pairs.append((eng.to_host(eng.ckks_rotate_hks(m, k, alpha, d_ct, tops[r], steps[r], key_L0=key_L0)),
                              eng.to_host(eng.ckks_rotate_hks(m, k, alpha, d_ct, subs[r], steps[r]))))
        return pairs

    at_both_levels(eng, run)


# ---- 3. the two linear transforms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,key_L0,L,k,alpha", [SMALL, (4, 6, 2, 3, 3), FUSED])
def test_linear_transforms_with_top_level_keys_and_diagonals(eng, logn, key_L0, L, k, alpha):
    c = Case(9300, logn, key_L0, L, k, alpha)
    m = c.mext
    d_ct = eng.to_device(c.rng.poly((2, 2, L, c.n), c.q))
    # flat: three rotations, one a conjugation, one diagonal NULL (the constant 1)
    f_steps, f_conj = [1, 0, 5], [False, True, False]
    f_keys = [c.key(eng) for _ in f_steps]
    f_diags = [c.diag(eng), (None, None), c.diag(eng)]
    # baby-step giant-step: 2 babies (the first the identity: NULL key) x 2 giants (the second conjugating), one term absent
    b_steps, b_keys = [0, 1], [(None, None), c.key(eng)]
    g_steps, g_conj, g_keys = [2, 0], [False, True], [c.key(eng), c.key(eng)]
    g_diags = [[c.diag(eng), (None, None)], [c.diag(eng), c.diag(eng)]]
    top, sub = (lambda xs: [x[0] for x in xs]), (lambda xs: [x[1] for x in xs])

    def run():
        return [
            (eng.to_host(eng.ckks_lintrans_hks(m, k, alpha, d_ct, top(f_keys), f_steps, top(f_diags), f_conj, key_L0=key_L0)),
             eng.to_host(eng.ckks_lintrans_hks(m, k, alpha, d_ct, sub(f_keys), f_steps, sub(f_diags), f_conj))),
            (eng.to_host(eng.ckks_lintrans_bsgs_hks(m, k, alpha, d_ct, top(b_keys), b_steps, top(g_keys), g_steps,
                                                    [top(row) for row in g_diags], giant_conj=g_conj, key_L0=key_L0)),
             eng.to_host(eng.ckks_lintrans_bsgs_hks(m, k, alpha, d_ct, sub(b_keys), b_steps, sub(g_keys), g_steps,
                                                    [sub(row) for row in g_diags], giant_conj=g_conj))),
        ]

    at_both_levels(eng, run)


# ---- 4. the multiplications ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,key_L0,L,k,alpha", [SMALL, FUSED])
def test_multiplications_with_a_top_level_key(eng, logn, key_L0, L, k, alpha):
    c = Case(9400, logn, key_L0, L, k, alpha)
    m, T = c.mext, 3
    d_a = [eng.to_device(M.lazy_rows(c.rng, (2, 2, L, c.n), c.q)) for _ in range(T)]
    d_b = [eng.to_device(M.lazy_rows(c.rng, (2, 2, L, c.n), c.q)) for _ in range(T)]
    d_top, d_sub = c.key(eng)
    quad = eng.ckks_tensor_sum(c.q, d_a, d_b)

    def run():
        pairs = [
            (eng.to_host(eng.ckks_mult_hks(m, k, alpha, d_a[0], d_b[0], d_top, key_L0=key_L0)),
             eng.to_host(eng.ckks_mult_hks(m, k, alpha, d_a[0], d_b[0], d_sub))),
            (eng.to_host(eng.ckks_relin_rescale_hks(m, k, alpha, quad, d_top, key_L0=key_L0)),
             eng.to_host(eng.ckks_relin_rescale_hks(m, k, alpha, quad, d_sub))),
            (eng.to_host(eng.ckks_dot_hks(m, k, alpha, d_a, d_b, d_top, key_L0=key_L0)),
             eng.to_host(eng.ckks_dot_hks(m, k, alpha, d_a, d_b, d_sub))),
        ]
        assert pairs[0][0].shape == (2, 2, L - 1, c.n)
        return pairs

    at_both_levels(eng, run)


# ---- 5. one key set down a chain -------------------------------------------------------------------------------------------------------
def test_one_key_serves_a_chain_of_multiplications(eng):
    """squarings 4 -> 3 -> 2 -> 1 limbs with ONE random "relinearisation" key generated at the top: every stage's words are those of
    the same chain run through the plain call with the three extracted sub-keys"""
    logn, key_L0, k, alpha = 11, 4, 2, 2
    n, mtop = 1 << logn, top_chain(key_L0, k)
    rng = SplitMix(9500)
    top = rng.poly((level_digits(key_L0, alpha), 2, key_L0 + k, n), mtop)
    d_top = eng.to_device(top)
    ct = ref = eng.to_device(rng.poly((1, 2, key_L0, n), mtop[:key_L0]))
    for L in (4, 3, 2):
        mext = level_chain(mtop, key_L0, L, k)
        ct = eng.ckks_mult_hks(mext, k, alpha, ct, ct, d_top, key_L0=key_L0)
        ref = eng.ckks_mult_hks(mext, k, alpha, ref, ref, eng.to_device(sub_key(top, key_L0, L, k, alpha)))
        assert tuple(ct.shape) == (1, 2, L - 1, n)
        assert np.array_equal(eng.to_host(ct), eng.to_host(ref)), L


# ---- 6. the extracted key is the level's key -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,key_L0,L,k,alpha", [SMALL, (4, 6, 2, 3, 3)])
def test_the_extracted_key_is_the_level_key(eng, orc, logn, key_L0, L, k, alpha):
    """hp_dev_hks_keygen at the top and on the level's chain from the same secrets, the same e[d] and the level's rows of a: the
    sub-key of the one is the other, word for word.  Then the top key at work at the level: it switches a random pt to pt * s_from
    within test_hks.py::test_switch_decrypts_to_pt_times_s_from's bound (first shape only: two 40-bit limbs leave Q below 2^84,
    where worst * 2^60 < Q cannot hold)."""
    n, mtop = 1 << logn, top_chain(key_L0, k)
    mext, rows = level_chain(mtop, key_L0, L, k), level_rows(key_L0, L, k)
    ndt, nd = level_digits(key_L0, alpha), level_digits(L, alpha)
    rng = SplitMix(9600 + logn)
    s, s_from = (rng.words(n, 3).astype(np.int64) - 1 for _ in range(2))   # ternary
    a = rng.poly((1, ndt, key_L0 + k, n), mtop)
    e = (rng.words(ndt * n, 17).astype(np.int64) - 8).reshape(1, ndt, n)
    secrets = dev_i64(eng, np.stack([s, s_from]))
    top_rows, level_rows_ = eng.poly_from_signed(mtop, secrets), eng.poly_from_signed(mext, secrets)
    d_top = eng.hks_keygen(mtop, k, alpha, top_rows[0], top_rows[1:], eng.to_device(a), dev_i64(eng, e))
    d_level = eng.hks_keygen(mext, k, alpha, level_rows_[0], level_rows_[1:], eng.to_device(np.ascontiguousarray(a[:, :nd][:, :, rows])),
                             dev_i64(eng, e[:, :nd]))
    top, level = eng.to_host(d_top)[0], eng.to_host(d_level)[0]
    assert np.array_equal(sub_key(top, key_L0, L, k, alpha), level)
    assert (top < np.array(mtop, dtype=U)[:, None]).all() and (level < np.array(mext, dtype=U)[:, None]).all()   # canonical
    if (logn, key_L0, L, k, alpha) != SMALL:
        return
    q = mext[:L]
    pt = rng.poly((L, n), q)
    out = eng.to_host(eng.hks_switch(mext, k, alpha, eng.to_device(pt[None]), d_top[0], key_L0=key_L0))[0]
    s_ntt, from_ntt = (orc.poly_reduce_strict(q, orc.poly_ntt(q, np.stack([(x % m).astype(U) for m in q]))) for x in (s, s_from))
    lhs = orc.poly_add(q, out[0], orc.poly_mul(q, out[1], s_ntt))
    worst = centred_error(orc, logn, q, orc.poly_sub(q, lhs, orc.poly_mul(q, pt, from_ntt)))
    Q = 1
    for m in q:
        Q *= m
    assert worst < (1 << 24) and worst * (1 << 60) < Q, worst   # (Q ~ 2^120)


# ---- 7. argument errors ----------------------------------------------------------------------------------------------------------------
def test_bad_key_levels_are_refused_and_the_context_stays_usable(eng):
    from hehub_amd import capi
    from hehub_amd.engine import InvalidArgument

    logn, key_L0, L, k, alpha = SMALL
    c = Case(9700, logn, key_L0, L, k, alpha)
    d_pt = eng.to_device(c.rng.poly((1, L, c.n), c.q))
    d_top, d_sub = c.key(eng)
    for aa, bad in ((alpha, L - 1),        # key_L0 < L
                    (alpha, 0),
                    (alpha, 32 - k + 1),   # key_L0 + k > 32
                    (alpha, 1 << 62),
                    (1, 17)):              # ceil(key_L0 / alpha) > 16
        with pytest.raises(InvalidArgument) as err:
            eng.hks_switch(c.mext, k, aa, d_pt, d_top, key_L0=bad)
        assert err.value.code == capi.HP_EINVAL, bad
    # the largest key those limits allow is not refused for its size: 16 digits of one limb, key_L0 + k = 18 rows
    eng.hks_switch(c.mext, k, 1, d_pt, eng.empty((16, 2, 16 + k, c.n)).zero_(), key_L0=16)
    got = eng.to_host(eng.hks_switch(c.mext, k, alpha, d_pt, d_top, key_L0=key_L0))
    assert np.array_equal(got, eng.to_host(eng.hks_switch(c.mext, k, alpha, d_pt, d_sub)))
