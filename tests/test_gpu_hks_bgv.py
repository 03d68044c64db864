"""BGV over the hybrid key switch on the device (include/hehub_amd.h: hp_dev_bgv_hks_switch, hp_dev_bgv_rotate_hoisted_hks,
hp_dev_bgv_relin_modswitch_hks, hp_dev_bgv_mult_relin_modswitch_hks and their _at twins) against the exact model of
tests/hks_bgv_model.py, on residues (hks_model.residues_match: the same residues, every word below 2q), at parity level B and at
level A, and by decryption with keys hp_dev_hks_keygen / hp_dev_hks_keygen_rot make from error rows t * e.

Shapes (logn, L, k, alpha): the smallest at which ModDown_t can go wrong -- one special prime, as many as limbs per digit, a partial
last digit, L < alpha, the widest Garner (k = 8), and the ring degree from which ModDown's transform is fused with its epilogue.
Batch 2.  t = 65537 everywhere, t = 2 and t = 2^31 - 1 on the first and the last shape.  The model of a case is computed once and
held against both parity levels."""
import numpy as np
import pytest

import hks_bgv_model as B
from gpu_words import at_both_levels, dev_i64, residues
from hks_levels import embed_key, level_chain, level_digits, sub_key, top_chain
from hks_model import chain, model_digits, residues_match
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64

SHAPES = [
    (3, 3, 1, 1),    # one special prime, one limb per digit
    (3, 3, 3, 3),    # a single digit
    (4, 4, 2, 2),
    (4, 5, 2, 3),    # the last digit is partial
    (4, 2, 3, 3),    # L < alpha
    (4, 3, 8, 3),    # the widest Garner
    (11, 3, 2, 2),   # the fused-drop path
]
DECRYPT = [(4, 4, 2, 2), (11, 3, 2, 2)]
BATCH, T0 = 2, 65537


def plain_moduli(shape):
    return (T0, 2, 2147483647) if shape in (SHAPES[0], SHAPES[-1]) else (T0,)


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def nd_of(L, alpha):
    return (L + alpha - 1) // alpha


# ---- 1. the switch -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha", SHAPES)
def test_switch_matches_the_model(eng, orc, logn, L, k, alpha):
    mext, n = chain(L, k), 1 << logn
    q = mext[:L]
    rng = SplitMix(8100 + logn + 8 * L + k)
    pt = rng.poly((BATCH, L, n), q)
    key = rng.poly((nd_of(L, alpha), 2, L + k, n), mext)
    acc = [B.inner(mext, model_digits(orc, logn, mext, L, k, alpha, pt[b]), key) for b in range(BATCH)]   # (no t before ModDown)
    d_pt, d_key = eng.to_device(pt), eng.to_device(key)
    for t in plain_moduli((logn, L, k, alpha)):
        exp = [B.mod_down_bgv(orc, logn, mext, L, k, t, a) for a in acc]
        got = at_both_levels(eng, lambda: eng.to_host(eng.bgv_hks_switch(mext, t, k, alpha, d_pt, d_key)))
        for level, g in got.items():
            assert g.shape == (BATCH, 2, L, n)
            for b in range(BATCH):
                assert residues_match(g[b], exp[b], q), (level, t, b)


@pytest.mark.parametrize("logn,L,k,alpha", SHAPES)
def test_switch_of_planted_accumulators(eng, orc, logn, L, k, alpha):
    """ModDown_t's input chosen coefficient by coefficient through the public call (hks_bgv_model.planted_values has the classes):
    the output is plain integer arithmetic.  Single-digit and several-digit shapes: the other digits' key rows are zero."""
    mext, n = chain(L, k), 1 << logn
    q = mext[:L]
    d_pt = eng.to_device(np.stack([B.planted_pt(L, n)] * BATCH))
    for t in plain_moduli((logn, L, k, alpha)):
        w = B.planted_values(SplitMix(8200 + t % 1000 + logn), mext, L, k, t, n)
        assert all(B.planted_classes(w, mext, L, k, t).values())
        d_key = eng.to_device(B.planted_key(orc, logn, mext, L, k, alpha, w))
        exp = B.planted_expected(orc, logn, mext, L, k, t, w)
        got = at_both_levels(eng, lambda: eng.to_host(eng.bgv_hks_switch(mext, t, k, alpha, d_pt, d_key)))
        for level, g in got.items():
            for b in range(BATCH):
                assert residues_match(g[b], exp, q), (level, t, b)


@pytest.mark.parametrize("logn,L,k,alpha", SHAPES)
def test_plain_modulus_one_gives_the_residues_of_the_ckks_switch(eng, logn, L, k, alpha):
    mext, n = chain(L, k), 1 << logn
    q = mext[:L]
    rng = SplitMix(8300 + logn + 8 * L + k)
    d_pt = eng.to_device(rng.poly((BATCH, L, n), q))
    d_key = eng.to_device(rng.poly((nd_of(L, alpha), 2, L + k, n), mext))
    got = at_both_levels(eng, lambda: (eng.to_host(eng.bgv_hks_switch(mext, 1, k, alpha, d_pt, d_key)),
                                       eng.to_host(eng.hks_switch(mext, k, alpha, d_pt, d_key))))
    for level, (bgv, ckks) in got.items():
        assert (bgv < 2 * np.array(q, dtype=U)[:, None]).all(), level
        assert np.array_equal(residues(bgv, q), residues(ckks, q)), level


# ---- 2. hoisted rotations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha", SHAPES)
def test_hoisted_rotations_match_the_model(eng, orc, logn, L, k, alpha):
    mext, n = chain(L, k), 1 << logn
    q = mext[:L]
    rng = SplitMix(8400 + logn + 8 * L + k)
    steps, conj = [3, 0, 0], [False, False, True]   # a rotation of the rows, step 0, the row swap
    ct = rng.poly((BATCH, 2, L, n), q)
    keys = [rng.poly((nd_of(L, alpha), 2, L + k, n), mext) for _ in steps]
    D = [model_digits(orc, logn, mext, L, k, alpha, np.ascontiguousarray(ct[b, 1])) for b in range(BATCH)]
    d_ct, d_keys = eng.to_device(ct), [eng.to_device(key) for key in keys]
    for t in plain_moduli((logn, L, k, alpha)):
        exp = [B.model_hoisted_bgv(orc, logn, mext, L, k, alpha, t, ct[b], keys, steps, conj, D[b]) for b in range(BATCH)]
        got = at_both_levels(eng, lambda: (eng.to_host(eng.bgv_rotate_hoisted_hks(mext, t, k, alpha, d_ct, d_keys, steps, conj)),
                                           eng.to_host(eng.bgv_rotate_hoisted_hks(mext, t, k, alpha, d_ct, d_keys[:1], steps[:1]))))
        for level, (g, single) in got.items():
            assert g.shape == (BATCH, 3, 2, L, n) and single.shape == (BATCH, 1, 2, L, n)
            for b in range(BATCH):
                for r in range(3):
                    assert residues_match(g[b, r], exp[b][r], q), (level, t, b, r)
                assert residues_match(single[b, 0], exp[b][0], q), (level, t, b)   # rotations == 1: row 0 of the longer call
                assert np.array_equal(residues(single[b, 0], q), residues(g[b, 0], q)), (level, t, b)


# ---- 3. relinearisation + mod switch, and the multiplication ----------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha", SHAPES)
def test_relin_modswitch_and_mult_match_the_model(eng, orc, logn, L, k, alpha):
    mext, n = chain(L, k), 1 << logn
    q = mext[:L]
    rng = SplitMix(8500 + logn + 8 * L + k)
    d_a, d_b = (eng.to_device(rng.poly((BATCH, 2, L, n), q)) for _ in range(2))
    key = rng.poly((nd_of(L, alpha), 2, L + k, n), mext)
    d_key = eng.to_device(key)
    d_quad = eng.mult_low_level(q, d_a, d_b)
    quad = eng.to_host(d_quad)
    for t in plain_moduli((logn, L, k, alpha)):
        exp = [B.model_relin_modswitch_bgv(orc, logn, mext, L, k, alpha, t, quad[b], key) for b in range(BATCH)]
        got = at_both_levels(eng, lambda: (eng.to_host(eng.bgv_relin_modswitch_hks(mext, t, k, alpha, d_quad, d_key)),
                                           eng.to_host(eng.bgv_mult_hks(mext, t, k, alpha, d_a, d_b, d_key))))
        for level, (tail, mult) in got.items():
            assert tail.shape == (BATCH, 2, L - 1, n)
            for b in range(BATCH):
                assert residues_match(tail[b], exp[b], q[:-1]), (level, t, b)
            assert np.array_equal(mult, tail), (level, t)   # the fused call IS mult_low_level + the tail: word for word


# ---- 4. by decryption, with keys made on the device from error rows t * e -----------------------------------------------------------------
def int64s(values):
    return np.array([int(v) for v in values], dtype=np.int64)


def uniform_rows(eng, rng, R, mext, alpha, k, n):
    return eng.to_device(rng.poly((R, nd_of(len(mext) - k, alpha), len(mext), n), mext))


def error_rows(eng, rng, R, nd, n, t):
    """the BGV recipe: hp_dev_hks_keygen's int64 error rows are t * e"""
    return dev_i64(eng, (t * B.small_errors(rng, R * nd * n)).reshape(R, nd, n))


def device_keys(eng, rng, mext, k, alpha, t, s, sources):
    """one key per source secret (integer coefficients), each switching it to s: [R][nd][2][E][n] on the device"""
    n, R, nd = len(s), len(sources), nd_of(len(mext) - k, alpha)
    rows = eng.poly_from_signed(mext, dev_i64(eng, np.stack([int64s(s)] + [int64s(x) for x in sources])))
    return eng.hks_keygen(mext, k, alpha, rows[0], rows[1:], uniform_rows(eng, rng, R, mext, alpha, k, n), error_rows(eng, rng, R, nd, n, t))


def device_rotation_keys(eng, rng, mext, k, alpha, t, s, steps, conj):
    n, R, nd = len(s), len(steps), nd_of(len(mext) - k, alpha)
    rows = eng.poly_from_signed(mext, dev_i64(eng, int64s(s)[None]))
    return eng.hks_keygen_rot(mext, k, alpha, rows[0], steps, uniform_rows(eng, rng, R, mext, alpha, k, n), error_rows(eng, rng, R, nd, n, t),
                              conj)


def messages(rng, count, n, t):
    return [np.array([int(v) for v in rng.words(n, t)], dtype=object) for _ in range(count)]


@pytest.mark.parametrize("logn,L,k,alpha", DECRYPT)
def test_switch_rotation_and_mult_decrypt(eng, orc, logn, L, k, alpha):
    mext, n, t = chain(L, k), 1 << logn, T0
    q = mext[:L]
    rng = SplitMix(8600 + logn)
    s, s_old = B.ternary(rng, n), B.ternary(rng, n)
    msgs = messages(rng, 2 * BATCH, n, t)
    ct_a = np.stack([B.encrypt_bgv(orc, rng, q, t, s, m) for m in msgs[:BATCH]])
    ct_b = np.stack([B.encrypt_bgv(orc, rng, q, t, s, m) for m in msgs[BATCH:]])
    ct_old = np.stack([B.encrypt_bgv(orc, rng, q, t, s_old, m) for m in msgs[:BATCH]])
    steps, conj = [3, 0], [False, True]
    keys = device_keys(eng, rng, mext, k, alpha, t, s, [s_old, B.negacyclic_ntt(orc, q, s, s)])
    rot_keys = device_rotation_keys(eng, rng, mext, k, alpha, t, s, steps, conj)
    d_a, d_b = eng.to_device(ct_a), eng.to_device(ct_b)
    d_old1 = eng.to_device(np.ascontiguousarray(ct_old[:, 1]))

    def run():
        quad = eng.ckks_tensor_sum(q, [d_a, d_b, d_a], [d_b, d_b, d_a])   # three terms, one switch
        return (eng.to_host(eng.bgv_hks_switch(mext, t, k, alpha, d_old1, keys[0])),
                eng.to_host(eng.bgv_rotate_hoisted_hks(mext, t, k, alpha, d_a, [rot_keys[0], rot_keys[1]], steps, conj)),
                eng.to_host(eng.bgv_mult_hks(mext, t, k, alpha, d_a, d_b, keys[1])),
                eng.to_host(eng.bgv_relin_modswitch_hks(mext, t, k, alpha, quad, keys[1])))

    moved_s = [B.moved_coeffs(orc, q, s, st, cj) for st, cj in zip(steps, conj)]
    for level, (sw, rot, mult, dot) in at_both_levels(eng, run).items():
        for b in range(BATCH):
            ma, mb = msgs[b], msgs[BATCH + b]
            switched = np.stack([orc.poly_add(q, np.ascontiguousarray(sw[b, 0]), ct_old[b, 0]), sw[b, 1]])
            assert np.array_equal(B.decrypt_bgv(orc, q, t, s, switched), ma), (level, b, "switch")
            for r, (st, cj) in enumerate(zip(steps, conj)):
                moved_ct = np.stack([B.move(orc, ct_a[b, 0], st, cj), B.move(orc, ct_a[b, 1], st, cj)])
                want = B.decrypt_bgv(orc, q, t, moved_s[r], moved_ct)   # the moved ciphertext under the moved secret
                assert np.array_equal(B.decrypt_bgv(orc, q, t, s, rot[b, r]), want), (level, b, r, "rotation")
                assert not np.array_equal(want, ma)
            ab = B.negacyclic_ntt(orc, q, ma, mb, t)
            assert np.array_equal(B.decrypt_bgv(orc, q[:-1], t, s, mult[b]), ab), (level, b, "mult")
            total = (ab + B.negacyclic_ntt(orc, q, mb, mb, t) + B.negacyclic_ntt(orc, q, ma, ma, t)) % t
            assert np.array_equal(B.decrypt_bgv(orc, q[:-1], t, s, dot[b]), total), (level, b, "sum of products")


# ---- 5. one top-level key set at every level ------------------------------------------------------------------------------------------------
def test_at_calls_equal_the_plain_calls_on_the_extracted_key(eng):
    """a top key of key_L0 = 5 at L = 3: every _at call equals the plain call on hks_levels.sub_key's extraction, word for word, at
    both parity levels.  Random key words (the claim is about addressing), the level key planted into a top-shaped block of other words"""
    logn, key_L0, L, k, alpha, t = 4, 5, 3, 2, 2, T0
    n, mtop = 1 << logn, top_chain(key_L0, k)
    mext = level_chain(mtop, key_L0, L, k)
    q = mext[:L]
    rng, fill = SplitMix(8700), SplitMix(8777)

    def key_pair():
        level = rng.poly((level_digits(L, alpha), 2, L + k, n), mext)
        top = embed_key(fill.poly((level_digits(key_L0, alpha), 2, key_L0 + k, n), mtop), level, key_L0, L, k, alpha)
        assert np.array_equal(sub_key(top, key_L0, L, k, alpha), level)
        return eng.to_device(top), eng.to_device(level)

    steps, conj = [3, 0, 0], [False, False, True]
    d_pt = eng.to_device(rng.poly((BATCH, L, n), q))
    d_a, d_b = (eng.to_device(rng.poly((BATCH, 2, L, n), q)) for _ in range(2))
    d_quad = eng.mult_low_level(q, d_a, d_b)
    (top, sub), rots = key_pair(), [key_pair() for _ in steps]
    tops, subs = [x[0] for x in rots], [x[1] for x in rots]
    h = eng.to_host

    def run():
        return [(h(eng.bgv_hks_switch(mext, t, k, alpha, d_pt, top, key_L0=key_L0)), h(eng.bgv_hks_switch(mext, t, k, alpha, d_pt, sub))),
                (h(eng.bgv_rotate_hoisted_hks(mext, t, k, alpha, d_a, tops, steps, conj, key_L0=key_L0)),
                 h(eng.bgv_rotate_hoisted_hks(mext, t, k, alpha, d_a, subs, steps, conj))),
                (h(eng.bgv_relin_modswitch_hks(mext, t, k, alpha, d_quad, top, key_L0=key_L0)),
                 h(eng.bgv_relin_modswitch_hks(mext, t, k, alpha, d_quad, sub))),
                (h(eng.bgv_mult_hks(mext, t, k, alpha, d_a, d_b, top, key_L0=key_L0)), h(eng.bgv_mult_hks(mext, t, k, alpha, d_a, d_b, sub)))]

    for level, pairs in at_both_levels(eng, run).items():
        for i, (got, exp) in enumerate(pairs):
            assert got.shape == exp.shape and np.array_equal(got, exp), (level, i)


def test_one_key_serves_a_chain_of_two_multiplications(eng, orc):
    """squarings 4 -> 3 -> 2 limbs under ONE relinearisation key generated at the top with error t * e: the result decrypts to m^4"""
    logn, key_L0, k, alpha, t = 11, 4, 2, 2, T0
    n, mtop = 1 << logn, top_chain(key_L0, k)
    rng = SplitMix(8800)
    s = B.ternary(rng, n)
    (m,) = messages(rng, 1, n, t)
    qtop = mtop[:key_L0]
    d_key = device_keys(eng, rng, mtop, k, alpha, t, s, [B.negacyclic_ntt(orc, qtop, s, s)])[0]
    ct = eng.to_device(B.encrypt_bgv(orc, rng, qtop, t, s, m)[None])
    want = m
    for L in (4, 3):
        ct = eng.bgv_mult_hks(level_chain(mtop, key_L0, L, k), t, k, alpha, ct, ct, d_key, key_L0=key_L0)
        want = B.negacyclic_ntt(orc, qtop, want, want, t)
        assert tuple(ct.shape) == (1, 2, L - 1, n)
        assert np.array_equal(B.decrypt_bgv(orc, qtop[:L - 1], t, s, eng.to_host(ct)[0]), want), L


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_have_the_stated_codes_and_the_context_stays_usable(eng):
    from hehub_amd import capi
    from hehub_amd.engine import HpError, InvalidArgument

    logn, L, k, alpha, t = 4, 4, 2, 2, T0
    mext, n = chain(L, k), 1 << logn
    q = mext[:L]
    rng = SplitMix(8900)
    d_pt = eng.to_device(rng.poly((BATCH, L, n), q))
    d_a, d_b = (eng.to_device(rng.poly((BATCH, 2, L, n), q)) for _ in range(2))
    d_quad = eng.mult_low_level(q, d_a, d_b)
    d_key = eng.to_device(rng.poly((nd_of(L, alpha), 2, L + k, n), mext))

    def calls(mext, t, k, alpha, pt=d_pt, a=d_a, b=d_b, quad=d_quad, key=d_key, **kw):
        return [lambda: eng.bgv_hks_switch(mext, t, k, alpha, pt, key, **kw),
                lambda: eng.bgv_rotate_hoisted_hks(mext, t, k, alpha, a, [key], [1], **kw),
                lambda: eng.bgv_relin_modswitch_hks(mext, t, k, alpha, quad, key, **kw),
                lambda: eng.bgv_mult_hks(mext, t, k, alpha, a, b, key, **kw)]

    def refused(call, code):
        with pytest.raises(HpError) as err:
            call()
        assert err.value.code == code, err.value
        assert isinstance(err.value, InvalidArgument) == (code == capi.HP_EINVAL)

    for bad_t in (0, min(mext), max(mext), (1 << 64) - 1):   # t = 0; t >= a modulus (the smallest one itself, and beyond all)
        for call in calls(mext, bad_t, k, alpha):
            refused(call, capi.HP_EINVAL)
    # k = 9: the conversion by one composition per modulus is not extended
    m9 = chain(3, 9)
    key9 = eng.empty((nd_of(3, 3), 2, 12, n)).zero_()
    small = dict(pt=d_pt[:, :3].contiguous(), a=d_a[:, :, :3].contiguous(), b=d_b[:, :, :3].contiguous(),
                 quad=d_quad[:, :, :3].contiguous(), key=key9)
    for call in calls(m9, t, 9, 3, **small):
        refused(call, capi.HP_EUNSUPPORTED)
    # L = 1 for the two mod-switch calls
    m1 = chain(1, 2)
    one = dict(pt=d_pt[:, :1].contiguous(), a=d_a[:, :, :1].contiguous(), b=d_b[:, :, :1].contiguous(),
               quad=d_quad[:, :, :1].contiguous(), key=eng.empty((1, 2, 3, n)).zero_())
    for call in calls(m1, t, 2, 2, **one)[2:]:
        refused(call, capi.HP_EINVAL)
    # key_L0 < L
    for call in calls(mext, t, k, alpha, key_L0=L - 1):
        refused(call, capi.HP_EINVAL)
    # an output that overlaps the input
    refused(lambda: eng.bgv_rotate_hoisted_hks(mext, t, k, alpha, d_a, [d_key], [1], out=d_a.view(BATCH, 1, 2, L, n)), capi.HP_EINVAL)
    refused(lambda: eng.bgv_relin_modswitch_hks(mext, t, k, alpha, d_quad, d_key,
                                                out=d_quad.view(-1)[: BATCH * 2 * (L - 1) * n].view(BATCH, 2, L - 1, n)), capi.HP_EINVAL)
    # a NULL key in the rotation list
    refused(lambda: eng.bgv_rotate_hoisted_hks(mext, t, k, alpha, d_a, [d_key, None], [1, 2]), capi.HP_EINVAL)
    # nothing was enqueued and the context works
    got = eng.to_host(eng.bgv_hks_switch(mext, 1, k, alpha, d_pt, d_key))
    assert np.array_equal(residues(got, q), residues(eng.to_host(eng.hks_switch(mext, k, alpha, d_pt, d_key)), q))
