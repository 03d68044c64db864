"""tests/sample_model.py, the model every device sample is pinned by: its ChaCha20 block against RFC 8439 and the local openssl, the
state layout, the three rules on planted words, and what the distributions look like under the fixed seeds (CPU tier)."""
import shutil
import subprocess

import numpy as np
import pytest

import moduli as M
import params as P
import sample_cases as K
import sample_model as S

N15 = 15


def test_rfc8439_block_vector():
    """section 2.3.2: key 00..1f, counter 1, nonce words 0x09000000, 0x4a000000, 0"""
    state = np.array([list(S.CONSTANTS) + S.seed_words(bytes(range(32))) + [1, 0x09000000, 0x4A000000, 0]], dtype=np.uint32)
    out = S.chacha20_blocks(state)[0]
    assert [int(w) for w in out[:4]] == [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3]
    assert int(out[15]) == 0x4E3C50A2
    # the same state through the sampler's own layout: word 13 = 0x09000000, stream = 0x4a000000
    assert np.array_equal(S.chacha20_blocks(S.states(bytes(range(32)), [1], 0x09000000, 0x4A000000)), out[None])


def test_state_layout():
    st = S.states(K.SEED, [0, 7], S.word13(5, S.CBD, 200), 0x1122334455667788)
    assert [int(w) for w in st[1, :4]] == list(S.CONSTANTS) and [int(w) for w in st[1, 4:12]] == S.seed_words(K.SEED)
    assert int(st[0, 12]) == 0 and int(st[1, 12]) == 7
    assert int(st[1, 13]) == 5 | 3 << 16 | 200 << 24 == S.word13(5, 3, 200)
    assert int(st[1, 14]) == 0x55667788 and int(st[1, 15]) == 0x11223344
    assert S.word13(0x1FFFF, 1, 0) == 0xFFFF | 1 << 16   # (only 16 bits of the attempt)
    assert (S.UNIFORM, S.TERNARY, S.CBD) == (1, 2, 3)


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl binary on this machine")
@pytest.mark.parametrize("kind,limb_id,stream", [(S.UNIFORM, 2, 6), (S.CBD, 0, (1 << 32) - 1), (S.TERNARY, 0, 0xFEDCBA9876543210)])
def test_whole_attempt0_row_against_openssl(kind, limb_id, stream):
    """openssl's chacha20 takes the 16 bytes of -iv as state words 12 .. 15: the keystream of a whole attempt-0 row in one call"""
    logn = 11
    w13 = S.word13(0, kind, limb_id)
    ks = S.keystream_bytes(K.SEED, w13, stream, (1 << logn) // 8)
    r = subprocess.run(["openssl", "enc", "-chacha20", "-K", K.SEED.hex(), "-iv", S.openssl_iv(w13, stream).hex()], input=bytes(len(ks)),
                       capture_output=True)
    if r.returncode != 0:
        pytest.skip("this openssl has no chacha20 cipher")
    assert r.stdout == ks
    # and the candidates are those bytes, 8 to a coefficient, little-endian
    cands = np.frombuffer(r.stdout, dtype="<u8")
    if kind == S.UNIFORM:
        q = P.P40[2]
        row, redraws = S.uniform_row(1 << logn, q, K.SEED, stream, limb_id)
        first = cands & np.uint64((1 << q.bit_length()) - 1)
        assert np.array_equal(row[redraws == 0], first[redraws == 0]) and bool((first[redraws > 0] >= q).all())
    elif kind == S.CBD:
        assert [S.cbd_word(int(v)) for v in cands] == list(S.cbd_row(logn, K.SEED, stream))
    else:
        assert [S.ternary_word(int(v)) for v in cands] == list(S.ternary_row(logn, K.SEED, stream))


def test_candidate_extraction():
    out = np.arange(1, 17, dtype=np.uint32)[None] * np.uint32(0x01010101)
    c = S.candidates(out)
    assert c.shape == (1, 8)
    for i in range(8):
        assert int(c[0, i]) == int(out[0, 2 * i]) | int(out[0, 2 * i + 1]) << 32
    assert out.astype("<u4").tobytes()[8 * 3:8 * 4] == int(c[0, 3]).to_bytes(8, "little")


@pytest.mark.parametrize("q", K.PLANT_MODULI, ids=lambda q: f"{q.bit_length()}b")
def test_uniform_rule_on_planted_sequences(q):
    for cands, word, used in K.planted_sequences(q):
        seen = []

        def feed():
            for v in cands + [0]:   # (a 65th candidate that must never be looked at)
                seen.append(v)
                yield v

        assert S.uniform_word(q, feed()) == word
        assert len(seen) == used


def test_ternary_rule_on_planted_words():
    assert [S.ternary_word(v) for v in (0, 1, 2)] == [-1, 0, 1]
    assert S.ternary_word(0b0111) == 0 and S.ternary_word(0b1011) == 1 and S.ternary_word(0b0011) == -1   # first field 3: the second
    assert S.ternary_word(S.M64) == 0                                            # all fields 3
    assert S.ternary_word(S.M64 >> 2) == -1 and S.ternary_word((2 << 62) | (S.M64 >> 2)) == 1   # only the last field is not 3
    assert S.ternary_word((1 << 62) | (S.M64 >> 2)) == 0


def test_binomial_extremes():
    m = (1 << 21) - 1
    assert S.cbd_word(m) == 21 and S.cbd_word(m << 21) == -21 and S.cbd_word(0) == 0 and S.cbd_word(m | m << 21) == 0
    assert S.cbd_word(S.M64) == 0 and S.cbd_word(~(m | m << 21) & S.M64) == 0       # bits 42 .. 63 are not read
    assert S.cbd_word(0b101 | 1 << 21) == 1


def test_rows_are_the_word_rules():
    """the vectorised rows against the single-word rules"""
    logn, stream = 6, 77
    cands = S.candidates(S.chacha20_blocks(S.states(K.SEED, np.arange(8), S.word13(0, S.TERNARY, 0), stream))).reshape(-1)
    assert [S.ternary_word(int(v)) for v in cands] == list(S.ternary_row(logn, K.SEED, stream))
    q = 65537
    row, redraws = S.uniform_row(1 << logn, q, K.SEED, stream, 3)
    assert redraws.max() >= 2
    for i in range(1 << logn):
        seq = (int(S.candidates(S.chacha20_blocks(S.states(K.SEED, [i // 8], S.word13(a, S.UNIFORM, 3), stream)))[0, i % 8]) for a in range(64))
        assert S.uniform_word(q, seq) == int(row[i])
    assert np.array_equal(S.sample_uniform(logn, [q], K.SEED, stream, [3], batch=2)[1, 0], S.uniform_row(1 << logn, q, K.SEED, stream + 1, 3)[0])


# ---- the distributions under the fixed seeds, N = 2^15 ------------------------------------------------------------------------------------
def test_ternary_frequencies():
    t = S.ternary_row(N15, K.SEED, 3)
    for v in (-1, 0, 1):
        assert abs(float((t == v).mean()) - 1 / 3) <= 0.01
    assert set(np.unique(t)) == {-1, 0, 1}


def test_binomial_variance():
    c = S.cbd_row(N15, K.SEED, 3)
    assert abs(float(c.var()) - 10.5) <= 0.5 and abs(float(c.mean())) < 0.1 and int(np.abs(c).max()) <= 21


@pytest.mark.parametrize("q", [M.PACK40EDGE[1], 65537])
def test_modulus_just_above_a_power_of_two_redraws_every_other_word(q):
    assert q - (1 << (q.bit_length() - 1)) < q >> 10
    row, redraws = S.uniform_row(1 << N15, q, K.SEED, 3, 1)
    assert 0.4 <= float((redraws > 0).mean()) <= 0.6
    assert int((redraws >= 3).sum()) >= 1
    assert int(row.max()) < q


def test_table_primes_need_essentially_no_redraw():
    for q in P.P40[:3] + P.P50[:2] + [M.Q59]:
        row, redraws = S.uniform_row(1 << N15, q, K.SEED, 3, 0)
        assert int((redraws > 0).sum()) <= 2 and int(row.max()) < q   # (a P40 prime rejects about 1.5e-6 of its candidates, a P50 prime fewer)


def test_kinds_seeds_streams_and_labels_separate_the_keystream():
    n, q = 1 << 8, P.P40[0]
    base = S.uniform_row(n, q, K.SEED, 4, 0)[0]
    assert not np.array_equal(base, S.uniform_row(n, q, K.SEED, 4, 1)[0])
    assert not np.array_equal(base, S.uniform_row(n, q, K.SEED, 5, 0)[0])
    assert not np.array_equal(base, S.uniform_row(n, q, K.SEED2, 4, 0)[0])
    assert not np.array_equal(S.ternary_row(8, K.SEED, 4), np.clip(S.cbd_row(8, K.SEED, 4), -1, 1))
