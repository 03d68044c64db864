"""BFV on the device at the Garner widths, chunk counts and modulus widths tests/test_gpu_bfv.py does not reach (tests/bfv_edges.py
has the tables, tests/test_bfv_edges.py their conditions): k_bfv_lift / k_bfv_scale / k_bfv_decrypt_round at the fenced widths 5, 6, 7
and at the guarded width 16 with 9, 10, 12, 13 and 16 moduli; rows of two and four chunks in a batch of two; 59-bit digits composed
into 20-, 36- and 40-bit moduli and the reverse; plain moduli 2, 4, 2^19, 2^58 and min(q) - 1.

Against the exact integer model of tests/bfv_model.py, word for word (np.array_equal); no tolerance anywhere.  Batch 2.  Two kinds of
input rows per transforming call: the transforms of the planted coefficients with q added to about half of the words, held to the
plain rounding of the planted integers; and rows that hold the word 2q - 1 (bfv_edges.edge_rows), held to the model's residue
mechanics, which are defined for any residues.  Parity level B everywhere and, at logn 12, also level A: the same words."""
import numpy as np
import pytest

import bfv_edges as E
import bfv_model as F
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64
BATCH = E.BATCH
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


def seed_of(shape, base):
    return base + 97 * E.SHAPES.index(shape)


# ---- 1. the lift --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", E.SHAPES, ids=str)
def test_lift_matches_the_model_and_the_composed_path(eng, orc, shape):
    logn, L, M, n, q, qb = shape.logn, shape.L, shape.M, shape.n, shape.q, shape.qb
    rng = SplitMix(seed_of(shape, 19100))
    vals = E.plant_last(F.lift_planted(rng, qb, L, BATCH * n), E.digit_wrap_values(q))
    assert all(F.lift_classes(vals, qb, L).values())
    planted = E.lazy(rng, np.stack([F.ntt_rows(orc, logn, q, vals[b * n:(b + 1) * n]) for b in range(BATCH)]), q)
    qa, ba = np.array(q, dtype=U)[:, None], np.array(qb[L:], dtype=U)[:, None]
    for kind, x in (("planted", planted), ("edge", E.edge_rows(rng, (BATCH, L, n), q))):
        exp = np.stack([F.lift(orc, logn, qb, L, x[b]) for b in range(BATCH)])
        d_x = eng.to_device(x)

        def composed():   # inverse transform, strict, one exact composition per target modulus, forward transform
            c = eng.poly_reduce_strict_(q, eng.intt_(q, d_x.clone(), strict=True))
            up = eng.ntt_(qb[L:], eng.rns_base_many_to_many(q, qb[L:], c))
            return eng.to_host(up) % ba

        for level, (got, comp) in at_levels(eng, logn, lambda: (eng.to_host(eng.bfv_lift(qb, L, d_x)), composed())).items():
            assert got.shape == (BATCH, L + M, n)
            assert np.array_equal(got[:, :L], x % qa), (kind, level)
            assert np.array_equal(got, exp), (kind, level)
            assert np.array_equal(got[:, L:], comp), (kind, level)


# ---- 2. the scaling -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,t", [(s, t) for s in E.SHAPES for t in s.ts], ids=str)
def test_scale_round_of_planted_integers(eng, orc, shape, t):
    logn, L, n, q, qb = shape.logn, shape.L, shape.n, shape.q, shape.qb
    Q = F.prod(q)
    assert F.base_ok(qb, L, t, n)
    rng = SplitMix(seed_of(shape, 19200) + t % 1000)
    vals = E.plant_last(F.scale_planted(rng, qb, L, t, n, BATCH * n), E.digit_wrap_inputs(q, t))
    assert all(F.scale_classes(vals, qb, L, t, n).values())
    x = E.lazy(rng, np.stack([F.ntt_rows(orc, logn, qb, vals[b * n:(b + 1) * n]) for b in range(BATCH)]), qb)
    exp = np.stack([F.ntt_rows(orc, logn, q, [F.scale_int(v, t, Q) for v in vals[b * n:(b + 1) * n]]) for b in range(BATCH)])
    assert np.array_equal(np.stack([F.scale(orc, logn, qb, L, t, x[b]) for b in range(BATCH)]), exp)   # the mechanics are the rounding
    # any residues below 2q, the word 2q - 1 among them: the mechanics themselves
    edge = E.edge_rows(rng, (BATCH, len(qb), n), qb)
    exp_edge = np.stack([F.scale(orc, logn, qb, L, t, edge[b]) for b in range(BATCH)])
    d_x, d_edge = eng.to_device(x), eng.to_device(edge)
    run = lambda: (eng.to_host(eng.bfv_scale_round(qb, L, t, d_x)), eng.to_host(eng.bfv_scale_round(qb, L, t, d_edge)))
    for level, (got, got_edge) in at_levels(eng, logn, run).items():
        assert got.shape == (BATCH, L, n)
        assert np.array_equal(got, exp), (level, t)
        assert np.array_equal(got_edge, exp_edge), (level, t)


# ---- 3. the quadratic ciphertext --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", E.MULT_SHAPES, ids=str)
def test_mult_low_level_matches_the_model_and_the_composition(eng, orc, shape):
    logn, L, M, n, q, qb, t = shape.logn, shape.L, shape.M, shape.n, shape.q, shape.qb, E.T0
    assert t in shape.ts
    rng = SplitMix(seed_of(shape, 19300))
    ct1, ct2 = E.edge_rows(rng, (BATCH, 2, L, n), q), E.edge_rows(rng, (BATCH, 2, L, n), q)
    d1, d2 = eng.to_device(ct1), eng.to_device(ct2)
    exp = np.stack([F.mult_low_level(orc, logn, qb, L, t, ct1[b], ct2[b]) for b in range(BATCH)])

    def composed():
        a = eng.bfv_lift(qb, L, d1.reshape(BATCH * 2, L, n)).reshape(BATCH, 2, L + M, n)
        c = eng.bfv_lift(qb, L, d2.reshape(BATCH * 2, L, n)).reshape(BATCH, 2, L + M, n)
        wide = eng.mult_low_level(qb, a, c)
        return eng.to_host(eng.bfv_scale_round(qb, L, t, wide.reshape(BATCH * 3, L + M, n))).reshape(BATCH, 3, L, n)

    for level, (got, comp) in at_levels(eng, logn, lambda: (eng.to_host(eng.bfv_mult_low_level(qb, t, d1, d2)), composed())).items():
        assert got.shape == (BATCH, 3, L, n)
        assert np.array_equal(got, exp), level
        assert np.array_equal(got, comp), level


# ---- 4. the decryption rounding alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dset", E.DECRYPT_SETS, ids=str)
def test_decrypt_round_of_planted_values(eng, dset):
    q, n = dset.q, dset.n
    Q = F.prod(q)
    for t in dset.ts:
        vals = E.plant_last(F.decrypt_planted(SplitMix(19600 + 97 * E.DECRYPT_SETS.index(dset) + t % 1000), q, t, BATCH * n), E.digit_wrap_inputs(q, t))
        assert all(F.decrypt_classes(vals, q, t).values())
        x = np.stack([F.residue_rows(vals[b * n:(b + 1) * n], q) for b in range(BATCH)])
        exp = np.array([F.decrypt_int(v, t, Q) for v in vals], dtype=U).reshape(BATCH, n)
        got = eng.to_host(eng.bfv_decrypt_round(q, t, eng.to_device(x)))
        assert got.shape == (BATCH, n) and (got < U(t)).all(), t
        assert np.array_equal(got, exp), (t, int((got != exp).sum()))


# ---- 5. decryption, end to end on the device ------------------------------------------------------------------------------------------------
def test_products_decrypt_on_the_device_at_a_fenced_width(eng):
    """as test_gpu_bfv.test_products_decrypt_on_the_device, at L = 6, M = 7: secret, relinearisation key and both ciphertexts from the
    device samplers; multiply; decrypt; round: m1 * m2 mod (X^N + 1, t) in every coefficient"""
    logn, L, M, k, alpha = E.HYBRID
    n, mext, aux, t = 1 << logn, E.HYBRID_MEXT, E.HYBRID_AUX, E.HYBRID_T
    q = mext[:L]
    assert F.base_ok(q + aux, L, t, n) and not set(mext[L:]) & set(q + aux)
    Q = F.prod(q)
    rng = SplitMix(19500)
    m = [[[int(x) for x in rng.words(n, t)] for _ in range(BATCH)] for _ in range(2)]
    want = np.array([[x % t for x in F.negacyclic(m[0][b], m[1][b])] for b in range(BATCH)], dtype=U)
    s = eng.sample_small_ntt(logn, mext, 2, SEED, 1)                                         # ternary, over q.. and p..
    key = eng.hks_keygen_seeded(mext, k, alpha, s[0], eng.poly_mul(mext, s, s), SEED, 100)[0]   # s_from = s * s, plain errors
    sk = s[0, :L].contiguous()
    cts = []
    for j in range(2):   # the coefficient rows (Delta mod q_i) * m
        rows = eng.to_device(np.stack([F.residue_rows(m[j][b], q) for b in range(BATCH)]))
        pt = eng.poly_reduce_strict_(q, eng.poly_scalar_mul(q, rows, [(Q // t) % qi for qi in q]))
        cts.append(eng.rlwe_encrypt_seeded(q, sk, pt, SEED, 1000 + 10 * j))
    out = eng.bfv_mult_hks(mext, aux, t, k, alpha, cts[0], cts[1], key)
    got = eng.to_host(eng.bfv_decrypt_round(q, t, eng.rlwe_decrypt_core(q, out, sk)))
    assert got.shape == (BATCH, n)
    assert np.array_equal(got, want)
