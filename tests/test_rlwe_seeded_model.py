"""tests/rlwe_seeded_model.py checked against what a ciphertext must satisfy (CPU tier): the model that pins every word of
hp_dev_rlwe_encrypt_seeded / _pk_seeded on the device (tests/test_gpu_rlwe_seeded.py) decrypts to exactly the error it drew.
Everything is Python integers; products of polynomials are schoolbook negacyclic convolutions."""
import numpy as np
import pytest

import rlwe_seeded_cases as RC
import rlwe_seeded_model as R
import sample_cases as K
import sample_model as S
from oracle.pyoracle import SplitMix

LOGNS = (3, 5, 6)
SCALES = (1, 65537)


def test_every_chain_of_the_cases_supports_its_ring_degree(orc):
    for name, (logn, moduli, *_rest) in RC.CASES.items():
        assert R.chain_supports(orc, logn, moduli), name
    for logn in LOGNS + (11,):
        assert R.chain_supports(orc, logn, RC.TABLE) and R.chain_supports(orc, logn, RC.HEAVY), logn
    assert not R.chain_supports(orc, 11, [RC.TABLE[0], 257])   # (what the check refuses: 257 - 1 has no factor 4096)


def _inputs(orc, logn, moduli, batch, seed):
    s_ntt = RC.secret_ntt(orc, logn, moduli)
    pt = SplitMix(seed).poly((batch, len(moduli), 1 << logn), moduli)
    return s_ntt, pt


def _error(orc, moduli, ct, s_ntt, pt):
    """(c0 + c1 s - pt) mod q, [L][n] Python integers"""
    dec = R.decrypt_coefficients(orc, moduli, ct, s_ntt)
    return [[(int(d) - int(p)) % q for d, p in zip(drow, prow)] for drow, prow, q in zip(dec, pt, moduli)]


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("logn", LOGNS)
@pytest.mark.parametrize("chain", ["TABLE", "HEAVY"])
def test_secret_key_ciphertext_decrypts_to_exactly_its_error(orc, chain, logn, scale):
    moduli, batch, stream = getattr(RC, chain), 2, 40 + logn
    s_ntt, pt = _inputs(orc, logn, moduli, batch, 17 * logn + scale)
    ct = R.encrypt_seeded(orc, logn, moduli, s_ntt, pt, K.SEED, stream, scale)
    assert ct.shape == (batch, 2, len(moduli), 1 << logn)
    assert bool((ct < np.array(moduli, dtype=np.uint64)[None, None, :, None]).all())
    for b in range(batch):
        e = S.cbd_row(logn, K.SEED, stream + b)
        err = _error(orc, moduli, ct[b], s_ntt, pt[b])
        for row, q in zip(err, moduli):
            assert row == [scale * int(v) % q for v in e]
            if 2 * 21 * scale < q:
                assert [R.centred(x, q) for x in row] == [scale * int(v) for v in e]
        assert np.array_equal(ct[b][1], S.sample_uniform(logn, moduli, K.SEED, stream + b)[0])
    # the compressed form: the same c0, nothing else
    c0 = R.encrypt_seeded(orc, logn, moduli, s_ntt, pt, K.SEED, stream, scale, with_c1=False)
    assert c0.shape == (batch, len(moduli), 1 << logn) and np.array_equal(c0, ct[:, 0])
    # a zero plaintext is no plaintext
    zero = np.zeros_like(pt)
    assert np.array_equal(R.encrypt_seeded(orc, logn, moduli, s_ntt, zero, K.SEED, stream, scale),
                          R.encrypt_seeded(orc, logn, moduli, s_ntt, None, K.SEED, stream, scale, batch=batch))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("logn", LOGNS)
def test_public_key_ciphertext_decrypts_to_the_error_of_its_three_draws(orc, logn, scale):
    moduli, batch, stream = RC.TABLE, 2, 90 + logn
    s_ntt, pt = _inputs(orc, logn, moduli, batch, 23 * logn + scale)
    s = RC.secret(logn)
    pk = R.encrypt_seeded(orc, logn, moduli, s_ntt, None, K.SEED2, RC.PK_STREAM, scale)[0]
    e_pk = S.cbd_row(logn, K.SEED2, RC.PK_STREAM)
    ct = R.encrypt_pk_seeded(orc, logn, moduli, pk, pt, K.SEED, stream, scale)
    assert ct.shape == (batch, 2, len(moduli), 1 << logn)
    for b in range(batch):
        u = S.ternary_row(logn, K.SEED, stream + 2 * b)
        e0, e1 = S.cbd_row(logn, K.SEED, stream + 2 * b), S.cbd_row(logn, K.SEED, stream + 2 * b + 1)
        ue, es = R.negacyclic(u, e_pk), R.negacyclic(e1, s)
        exp = [scale * (int(x) + int(y) + int(z)) for x, y, z in zip(ue, e0, es)]
        assert max(abs(v) for v in exp) <= scale * 21 * (2 * (1 << logn) + 1)
        err = _error(orc, moduli, ct[b], s_ntt, pt[b])
        for row, q in zip(err, moduli):
            assert [R.centred(x, q) for x in row] == exp


def test_batch_elements_and_their_ids(orc):
    logn, moduli, stream, batch = 5, RC.TABLE, (1 << 64) - 3, 3   # (the ids wrap: 64-bit arithmetic)
    s_ntt, pt = _inputs(orc, logn, moduli, batch, 5)
    assert R.ids_used("encrypt_seeded", stream, batch) == [(1 << 64) - 3, (1 << 64) - 2, (1 << 64) - 1]
    pk_ids = R.ids_used("encrypt_pk_seeded", stream, batch)
    assert len(set(pk_ids)) == 2 * batch and pk_ids[3:] == [0, 1, 2]
    ct = R.encrypt_seeded(orc, logn, moduli, s_ntt, pt, K.SEED, stream)
    pk = RC.model_pk(orc, "n32_L3_B1_t")
    pct = R.encrypt_pk_seeded(orc, logn, moduli, pk, pt, K.SEED, stream)
    for b in range(batch):
        assert np.array_equal(ct[b], R.encrypt_seeded(orc, logn, moduli, s_ntt, pt[b:b + 1], K.SEED, (stream + b) & S.M64)[0])
        assert np.array_equal(pct[b], R.encrypt_pk_seeded(orc, logn, moduli, pk, pt[b:b + 1], K.SEED, (stream + 2 * b) & S.M64)[0])
    # the draws of one public-key ciphertext: u_b and e0_b share an id and no keystream, e1_b has the next id
    rows = [S.ternary_row(logn, K.SEED, 8), np.sign(S.cbd_row(logn, K.SEED, 8)), np.sign(S.cbd_row(logn, K.SEED, 9))]
    assert not any(np.array_equal(rows[i], rows[j]) for i in range(3) for j in range(i + 1, 3))


def test_small_ntt_is_the_transform_of_the_residues(orc):
    logn, moduli = 5, RC.HEAVY
    for kind in (S.TERNARY, S.CBD):
        for scale in RC.SMALL_SCALES:
            got = R.small_ntt(orc, logn, moduli, kind, K.SEED, 11, scale, batch=2)
            for b in range(2):
                row = R.small_row(kind, logn, K.SEED, 11 + b)
                back = orc.poly_intt(moduli, np.ascontiguousarray(got[b]))
                assert [[int(w) % q for w in r] for r, q in zip(back, moduli)] == [[scale * int(v) % q for v in row] for q in moduli]
