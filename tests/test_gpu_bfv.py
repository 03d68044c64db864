"""BFV on the device (include/hehub_amd.h: hp_dev_bfv_lift, hp_dev_bfv_scale_round, hp_dev_bfv_mult_low_level, hp_dev_bfv_mult_relin_hks,
hp_dev_bfv_decrypt_round) against the exact integer model of tests/bfv_model.py -- word for word (np.array_equal) where the contract is
the canonical residue, on residues (hks_model.residues_match) for the relinearising calls --, against the compositions of existing
calls the new ones stand for, and by decryption end to end on the device.  Everything is integer and exact: no tolerance anywhere.

Shapes (logn, L, M, k, alpha): bfv_model.GPU_SHAPES (tests/test_bfv_model.py checks the base-size rule and the planted classes at each
of them on the CPU).  Batch 2.  Parity level B everywhere and, at logn 11 (the only shape with tiled transforms), also level A; the
model of a case is computed once and held against both."""
import numpy as np
import pytest

import bfv_model as F
import params as P
from hks_levels import embed_key, level_digits, sub_key
from hks_model import residues_match
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64
BATCH = 2
SHAPES = F.GPU_SHAPES
SEED = bytes(range(32))


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def at_levels(eng, logn, run):
    """{level: run()} at parity level B and, where the ring degree has tiled transforms, at level A"""
    got = {}
    for level in ("B", "A") if logn >= 11 else ("B",):
        eng.set_parity_level(level)
        try:
            got[level] = run()
            eng.sync()
        finally:
            eng.set_parity_level("B")
    return got


def setup(shape):
    logn, L, M, k, alpha = shape
    mext, aux = F.shape_moduli(shape)
    return logn, L, M, k, alpha, 1 << logn, mext, mext[:L], mext[:L] + aux


def lazy(rng, rows, moduli):
    """canonical rows [..][len(moduli)][n] with q added to about half of the words: the calls take words below 2q"""
    up = rng.words(rows.size, 2).reshape(rows.shape).astype(U)
    return rows + up * np.array(moduli, dtype=U)[:, None]


# ---- 1. the lift --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_lift_matches_the_model_and_the_composed_path(eng, orc, shape):
    logn, L, M, k, alpha, n, mext, q, qb = setup(shape)
    rng = SplitMix(9100 + logn + 8 * L)
    vals = F.lift_planted(rng, qb, L, BATCH * n)
    assert all(F.lift_classes(vals, qb, L).values())
    x = np.stack([F.ntt_rows(orc, logn, q, vals[b * n:(b + 1) * n]) for b in range(BATCH)])
    x = lazy(rng, x, q)
    exp = np.stack([F.lift(orc, logn, qb, L, x[b]) for b in range(BATCH)])
    d_x = eng.to_device(x)

    def composed():   # inverse transform, strict, one exact composition per target modulus, forward transform
        c = eng.poly_reduce_strict_(q, eng.intt_(q, d_x.clone(), strict=True))
        up = eng.ntt_(qb[L:], eng.rns_base_many_to_many(q, qb[L:], c))
        return eng.to_host(up) % np.array(qb[L:], dtype=U)[:, None]

    for level, (got, comp) in at_levels(eng, logn, lambda: (eng.to_host(eng.bfv_lift(qb, L, d_x)), composed())).items():
        assert got.shape == (BATCH, L + M, n)
        assert np.array_equal(got, exp), level
        assert np.array_equal(got[:, L:], comp), level


# ---- 2. the scaling -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_scale_round_of_planted_integers(eng, orc, shape):
    logn, L, M, k, alpha, n, mext, q, qb = setup(shape)
    Q = F.prod(q)
    for t in F.shape_plain_moduli(shape):
        rng = SplitMix(9200 + logn + 8 * L + t % 1000)
        vals = F.scale_planted(rng, qb, L, t, n, BATCH * n)
        assert all(F.scale_classes(vals, qb, L, t, n).values())
        x = lazy(rng, np.stack([F.ntt_rows(orc, logn, qb, vals[b * n:(b + 1) * n]) for b in range(BATCH)]), qb)
        exp = np.stack([F.ntt_rows(orc, logn, q, [F.scale_int(v, t, Q) for v in vals[b * n:(b + 1) * n]]) for b in range(BATCH)])
        assert np.array_equal(np.stack([F.scale(orc, logn, qb, L, t, x[b]) for b in range(BATCH)]), exp)   # the mechanics are the rounding
        d_x = eng.to_device(x)
        for level, got in at_levels(eng, logn, lambda: eng.to_host(eng.bfv_scale_round(qb, L, t, d_x))).items():
            assert got.shape == (BATCH, L, n)
            assert np.array_equal(got, exp), (level, t)


# ---- 3. the quadratic ciphertext --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mult_low_level_matches_the_model_and_the_composition(eng, orc, shape):
    logn, L, M, k, alpha, n, mext, q, qb = setup(shape)
    rng = SplitMix(9300 + logn + 8 * L)
    ct1, ct2 = lazy(rng, rng.poly((BATCH, 2, L, n), q), q), lazy(rng, rng.poly((BATCH, 2, L, n), q), q)
    d1, d2 = eng.to_device(ct1), eng.to_device(ct2)
    for t in F.shape_plain_moduli(shape):
        exp = np.stack([F.mult_low_level(orc, logn, qb, L, t, ct1[b], ct2[b]) for b in range(BATCH)])

        def composed():
            a = eng.bfv_lift(qb, L, d1.reshape(BATCH * 2, L, n)).reshape(BATCH, 2, L + M, n)
            c = eng.bfv_lift(qb, L, d2.reshape(BATCH * 2, L, n)).reshape(BATCH, 2, L + M, n)
            wide = eng.mult_low_level(qb, a, c)
            return eng.to_host(eng.bfv_scale_round(qb, L, t, wide.reshape(BATCH * 3, L + M, n))).reshape(BATCH, 3, L, n)

        for level, (got, comp) in at_levels(eng, logn, lambda: (eng.to_host(eng.bfv_mult_low_level(qb, t, d1, d2)), composed())).items():
            assert got.shape == (BATCH, 3, L, n)
            assert np.array_equal(got, exp), (level, t)
            assert np.array_equal(got, comp), (level, t)


# ---- 4. with relinearisation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mult_relin_matches_the_model_the_composition_and_its_at_twin(eng, orc, shape):
    logn, L, M, k, alpha, n, mext, q, qb = setup(shape)
    aux, t = qb[L:], F.T0
    rng, fill = SplitMix(9400 + logn + 8 * L), SplitMix(9477)
    ct1, ct2 = rng.poly((BATCH, 2, L, n), q), rng.poly((BATCH, 2, L, n), q)
    key = rng.poly((level_digits(L, alpha), 2, L + k, n), mext)
    # the same key inside one generated for L + 1 ciphertext moduli (the extra modulus: a prime of neither base)
    mtop = q + [P.P40[9]] + mext[L:]
    top = embed_key(fill.poly((level_digits(L + 1, alpha), 2, L + 1 + k, n), mtop), key, L + 1, L, k, alpha)
    assert np.array_equal(sub_key(top, L + 1, L, k, alpha), key)
    exp = [F.mult_relin(orc, logn, mext, L, k, alpha, aux, t, ct1[b], ct2[b], key) for b in range(BATCH)]
    d1, d2, d_key, d_top = eng.to_device(ct1), eng.to_device(ct2), eng.to_device(key), eng.to_device(top)

    def run():
        quad = eng.bfv_mult_low_level(qb, t, d1, d2)
        sw = eng.hks_switch(mext, k, alpha, quad[:, 2].contiguous(), d_key)
        comp = eng.poly_add(q, sw.reshape(BATCH * 2, L, n), quad[:, :2].contiguous().reshape(BATCH * 2, L, n)).reshape(BATCH, 2, L, n)
        return (eng.to_host(eng.bfv_mult_hks(mext, aux, t, k, alpha, d1, d2, d_key)), eng.to_host(comp),
                eng.to_host(eng.bfv_mult_hks(mext, aux, t, k, alpha, d1, d2, d_top, key_L0=L + 1)))

    qa = np.array(q, dtype=U)[:, None]
    for level, (got, comp, at) in at_levels(eng, logn, run).items():
        assert got.shape == (BATCH, 2, L, n)
        for b in range(BATCH):
            assert residues_match(got[b], exp[b], q), (level, b)
        assert np.array_equal(got % qa, comp % qa), level
        assert (at < 2 * qa).all() and np.array_equal(at % qa, got % qa), level


# ---- 5. decryption, end to end on the device ------------------------------------------------------------------------------------------------
DECRYPT = [(s, F.T0) for s in F.DECRYPT_SHAPES] + [(F.GPU_SHAPES[3], 2), (F.GPU_SHAPES[3], 2147483647)]


@pytest.mark.parametrize("shape,t", DECRYPT, ids=str)
def test_products_decrypt_on_the_device(eng, shape, t):
    """secret, relinearisation key and both ciphertexts from the device samplers; multiply; decrypt; round: m1 * m2 mod (X^N + 1, t) in
    every coefficient"""
    logn, L, M, k, alpha, n, mext, q, qb = setup(shape)
    assert F.base_ok(qb, L, t, n)
    Q = F.prod(q)
    rng = SplitMix(9500 + logn + t % 1000)
    m = [[[int(x) for x in rng.words(n, t)] for _ in range(BATCH)] for _ in range(2)]
    want = np.array([[x % t for x in F.negacyclic(m[0][b], m[1][b])] for b in range(BATCH)], dtype=U)

    def run():
        s = eng.sample_small_ntt(logn, mext, 2, SEED, 1)                                         # ternary, over q.. and p..
        key = eng.hks_keygen_seeded(mext, k, alpha, s[0], eng.poly_mul(mext, s, s), SEED, 100)[0]   # s_from = s * s, plain errors
        sk = s[0, :L].contiguous()
        cts = []
        for j in range(2):   # the coefficient rows (Delta mod q_i) * m
            rows = eng.to_device(np.stack([F.residue_rows(m[j][b], q) for b in range(BATCH)]))
            pt = eng.poly_reduce_strict_(q, eng.poly_scalar_mul(q, rows, [(Q // t) % qi for qi in q]))
            cts.append(eng.rlwe_encrypt_seeded(q, sk, pt, SEED, 1000 + 10 * j))
        out = eng.bfv_mult_hks(mext, qb[L:], t, k, alpha, cts[0], cts[1], key)
        return eng.to_host(eng.bfv_decrypt_round(q, t, eng.rlwe_decrypt_core(q, out, sk)))

    for level, got in at_levels(eng, logn, run).items():
        assert got.shape == (BATCH, n)
        assert np.array_equal(got, want), (level, t)


# ---- refusals: before anything is enqueued, with the output untouched ---------------------------------------------------------------------
def test_refusals(eng):
    import ctypes as C

    from hehub_amd import capi
    from hehub_amd.engine import _u64arr

    shape = F.GPU_SHAPES[1]
    logn, L, M, k, alpha, n, mext, q, qb = setup(shape)
    aux, t, E = qb[L:], F.T0, L + M
    SENT = -0x123456789
    rng = SplitMix(9700)
    d_x = eng.to_device(rng.poly((BATCH, L, n), q))
    d_w = eng.to_device(rng.poly((BATCH, E, n), qb))
    d_a, d_b = eng.to_device(rng.poly((BATCH, 2, L, n), q)), eng.to_device(rng.poly((BATCH, 2, L, n), q))
    d_key = eng.to_device(rng.poly((level_digits(L, alpha), 2, L + k, n), mext))
    outs = {"lift": eng.empty((BATCH, E, n)).fill_(SENT), "scale": eng.empty((BATCH, L, n)).fill_(SENT),
            "quad": eng.empty((BATCH, 3, L, n)).fill_(SENT), "lin": eng.empty((BATCH, 2, L, n)).fill_(SENT),
            "m": eng.empty((BATCH, n)).fill_(SENT)}
    p = lambda x: C.c_void_p(x.data_ptr())
    lib, h = eng.lib, eng.h

    # every call as a function of what a refusal varies; defaults: the valid call
    def lift(logn=logn, L=L, M=M, qb=qb, polys=BATCH, x=p(d_x), out=p(outs["lift"])):
        return lib.hp_dev_bfv_lift(h, logn, L, M, _u64arr(qb), polys, x, out)

    def scale(logn=logn, L=L, M=M, qb=qb, t=t, polys=BATCH, x=p(d_w), out=p(outs["scale"])):
        return lib.hp_dev_bfv_scale_round(h, logn, L, M, _u64arr(qb), t, polys, x, out)

    def mult(logn=logn, L=L, M=M, qb=qb, t=t, polys=BATCH, x=p(d_a), out=p(outs["quad"])):
        return lib.hp_dev_bfv_mult_low_level(h, logn, L, M, _u64arr(qb), t, polys, x, p(d_b), out)

    def relin(logn=logn, L=L, M=M, qb=qb, t=t, polys=BATCH, x=p(d_a), out=p(outs["lin"]), k=k, alpha=alpha, key_L0=None, key=p(d_key)):
        mx, ax = _u64arr(list(qb[:L]) + mext[len(q):]), _u64arr(qb[L:L + M] if M else [0])
        if key_L0 is None:
            return lib.hp_dev_bfv_mult_relin_hks(h, logn, L, k, alpha, mx, M, ax, t, polys, x, p(d_b), key, out)
        return lib.hp_dev_bfv_mult_relin_hks_at(h, logn, L, key_L0, k, alpha, mx, M, ax, t, polys, x, p(d_b), key, out)

    def dec(n=n, L=L, q=q, t=t, polys=BATCH, x=p(d_x), out=p(outs["m"])):
        return lib.hp_dev_bfv_decrypt_round(h, n, L, _u64arr(q), t, polys, x, out)

    with_base, with_t = (lift, scale, mult, relin), (scale, mult, relin)
    odd = lambda x: C.c_void_p(x.data_ptr() + 8)
    INV, UNS = capi.HP_EINVAL, capi.HP_EUNSUPPORTED
    for call in with_base + (dec,):
        assert call(x=None) == INV and call(out=None) == INV, call.__name__
        assert call(x=odd(d_a)) == INV and call(out=odd(outs["quad"])) == INV, call.__name__   # misaligned
        assert call(polys=0) == INV and call(L=0) == INV, call.__name__
    for call in with_base:
        assert call(logn=2) == INV and call(logn=17) == INV and call(M=0) == INV, call.__name__
        assert call(L=17, M=1, qb=list(range(3, 39, 2))) == UNS and call(L=1, M=17, qb=list(range(3, 39, 2))) == UNS, call.__name__
        assert call(qb=q + [q[0]] + aux[1:]) == INV, call.__name__                 # a modulus of Q in B
        assert call(qb=q + [aux[0] - 1] + aux[1:]) == INV, call.__name__           # an even modulus
        assert call(qb=[q[0] + 1] + q[1:] + aux) == INV, call.__name__
    assert lift(L=16, M=16, qb=[3] * 32) == INV   # (the largest shape the limits admit reaches the moduli checks)
    assert dec(n=4) == INV and dec(n=24) == INV and dec(n=1 << 17) == INV and dec(L=17, q=list(range(3, 37, 2))) == UNS
    for call in with_t:
        for bad in (0, 1, min(qb), max(qb), (1 << 64) - 1):   # t < 2; t >= a modulus (the smallest one itself, and beyond all)
            assert call(t=bad) == INV, (call.__name__, bad)
    for bad in (0, 1, min(q), (1 << 64) - 1):
        assert dec(t=bad) == INV, bad
    for call in with_t:   # B >= 4 t N Q fails with one aux prime less
        assert not F.base_ok(qb[:-1], L, t, n)
        assert call(M=M - 1, qb=qb[:-1]) == INV, call.__name__
    # an output overlapping an input
    assert lift(out=p(d_x)) == INV and scale(out=p(d_w)) == INV and mult(out=p(d_a)) == INV and relin(out=p(d_b)) == INV and dec(out=p(d_x)) == INV
    # what the switch refuses, with its code
    assert relin(k=0) == INV and relin(alpha=0) == INV and relin(alpha=9) == INV and relin(key_L0=L - 1) == INV and relin(key=None) == INV
    eng.sync()
    for name, out in outs.items():
        assert bool((out == SENT).all()), name
    # nothing was enqueued, and the context works
    assert lift() == 0 and scale() == 0 and mult() == 0 and relin() == 0 and relin(key_L0=L) == 0 and dec() == 0
    eng.sync()
    for name, out in outs.items():
        assert not bool((out == SENT).any()), name


# ---- 6. the decryption rounding alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_decrypt_round_of_planted_values(eng, shape):
    logn, L, M, k, alpha, n, mext, q, qb = setup(shape)
    Q = F.prod(q)
    for t in F.shape_plain_moduli(shape):
        vals = F.decrypt_planted(SplitMix(9600 + logn + t % 1000), q, t, BATCH * n)
        assert all(F.decrypt_classes(vals, q, t).values())
        x = np.stack([F.residue_rows(vals[b * n:(b + 1) * n], q) for b in range(BATCH)])
        exp = np.array([F.decrypt_int(v, t, Q) for v in vals], dtype=U).reshape(BATCH, n)
        got = eng.to_host(eng.bfv_decrypt_round(q, t, eng.to_device(x)))
        assert np.array_equal(got, exp), t
