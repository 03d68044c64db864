"""hp_dev_poly_from_signed, hp_dev_hks_keygen, hp_dev_hks_keygen_rot: hybrid key-switch keys generated on the device.

Sampling stays with the caller, so the calls are deterministic and every output word is pinned: the keys are CANONICAL residues, equal
word for word -- at both parity levels -- to keygen() of tests/hks_model.py handed the same uniform rows a and error polynomials e.
The model draws them from its random source (for key r, digit d: rng.poly((E, n), mext), then rng.words(n, 17)); `Draws` stands in
for that source, forwards to a SplitMix (planting edge words where a test asks for them) and records what it returned.  The
recorded rows are what the device gets.  A model key is computed once per shape and shared by the tests that need it."""
import ctypes as C

import numpy as np
import pytest

import moduli as M
import params as P
from gpu_words import dev_i64
from hks_model import centred, chain, decryption_errors, decryption_setup, keygen, rotations_of
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


class Draws:
    """keygen()'s random source: a SplitMix whose draws are recorded (a: the uniform rows, e: the error polynomials, secrets: the
    ternary draws of decryption_setup); `plant` edits a uniform row set before it is handed out"""

    def __init__(self, seed, plant=None):
        self.rng, self.plant, self.a, self.e, self.secrets = SplitMix(seed), plant, [], [], []

    def poly(self, shape, moduli):
        x = self.rng.poly(shape, moduli)
        if self.plant:
            x = self.plant(self.rng, x, moduli)
        self.a.append(x)
        return x

    def words(self, n, bound=0):
        w = self.rng.words(n, bound)
        if bound == 17:
            self.e.append(w.astype(np.int64) - 8)
        if bound == 3:
            self.secrets.append(w.astype(np.int64) - 1)
        return w

    def device_rows(self, eng, keys):
        a, e = np.stack(self.a), np.stack(self.e)
        nd = len(self.a) // keys
        return eng.to_device(a.reshape((keys, nd) + a.shape[1:])), dev_i64(eng, e.reshape(keys, nd, -1))


def ternary(rng, n):
    return rng.words(n, 3).astype(np.int64) - 1


def secret_rows(orc, mext, s):
    """a signed polynomial in NTT form over the chain, strict words [E][n]"""
    return orc.poly_reduce_strict(mext, orc.poly_ntt(mext, np.stack([(s % q).astype(U) for q in mext])))


def canonical(key, mext):
    return bool((key < np.array(mext, dtype=U)[:, None]).all())


_CASES = {}


def model_case(orc, logn, L, k, alpha, keys, mext=None, tag="table"):
    """ternary s_to and independent ternary s_from[r]; the model's keys [keys][nd][2][E][n] and the draws behind them"""
    at = (logn, L, k, alpha, keys, tag)
    if at not in _CASES:
        mext = mext or chain(L, k)
        n = 1 << logn
        rng = SplitMix(8100 + 16 * logn + L)
        s_to, s_from = ternary(rng, n), [ternary(rng, n) for _ in range(keys)]
        draws = Draws(8200 + logn + keys)
        exp = np.stack([keygen(orc, draws, logn, mext, L, k, alpha, s_to, sf) for sf in s_from])
        exp.setflags(write=False)
        _CASES[at] = (mext, secret_rows(orc, mext, s_to), np.stack([secret_rows(orc, mext, sf) for sf in s_from]), draws, exp)
    return _CASES[at]


def device_keys(eng, case, k, alpha, in_place=False):
    mext, s_to, s_from, draws, exp = case
    keys = exp.shape[0]
    d_a, d_e = draws.device_rows(eng, keys)
    if not in_place:
        return eng.to_host(eng.hks_keygen(mext, k, alpha, eng.to_device(s_to), eng.to_device(s_from), d_a, d_e))
    out = eng.empty(exp.shape).fill_(0x5A5A5A5A5A5A5A5A)
    out[:, :, 1] = d_a
    return eng.to_host(eng.hks_keygen(mext, k, alpha, eng.to_device(s_to), eng.to_device(s_from), None, d_e, out=out))


# ---- 1. bit-exact to the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha,keys", [
    (5, 4, 2, 2, 1),     # generic transforms, a row shorter than one chunk
    (6, 5, 2, 3, 3),     # last digit shorter than alpha, several keys
    (5, 3, 1, 1, 2),     # hehub's shape: one limb per digit, one special prime
    (11, 3, 2, 2, 2),    # tiled transforms, one full chunk
    (12, 5, 1, 3, 1),    # two chunks per row
])
def test_keygen_matches_the_model(eng, orc, logn, L, k, alpha, keys):
    case = model_case(orc, logn, L, k, alpha, keys)
    exp = case[4]
    assert canonical(exp, case[0])
    got = device_keys(eng, case, k, alpha)
    assert got.shape == exp.shape == (keys, (L + alpha - 1) // alpha, 2, L + k, 1 << logn)
    assert np.array_equal(got, exp)


# ---- 2. a rows preloaded into the key -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha,keys", [(6, 5, 2, 3, 3), (11, 3, 2, 2, 2)])
def test_keygen_converts_preloaded_rows_in_place(eng, orc, logn, L, k, alpha, keys):
    case = model_case(orc, logn, L, k, alpha, keys)
    assert np.array_equal(device_keys(eng, case, k, alpha, in_place=True), case[4])


# ---- 3. planted inputs --------------------------------------------------------------------------------------------------------------
def edge_positions(n):
    """the first and the last two words of a row and the two either side of every boundary between a thread's rounds (512 words), the
    chunk boundaries (2048) among them"""
    bounds = set(range(0, n, 512)) | {n}
    return sorted({i for b in bounds for i in (b - 2, b - 1, b, b + 1) if 0 <= i < n})


def plant_edges(rng, a, moduli):
    """uniform words below 2q, with 0, q - 1, q and 2q - 1 at the edge positions"""
    E, n = a.shape
    a = a + rng.words(E * n, 2).reshape(E, n).astype(U) * np.array(moduli, dtype=U)[:, None]
    for m, q in enumerate(moduli):
        for j, i in enumerate(edge_positions(n)):
            a[m, i] = (0, q - 1, q, 2 * q - 1)[(j + m) % 4]
    return a


@pytest.mark.parametrize("logn,L,k,alpha", [(5, 4, 2, 2), (11, 3, 2, 2)])
def test_keygen_on_planted_rows(eng, orc, logn, L, k, alpha):
    """lazy secrets (the rows a chained call hands in) and edge words in a.  The model takes its secrets as integer polynomials: the
    centred integers behind the lazy rows, whose strict transform is the residue of every planted word."""
    mext, n = chain(L, k), 1 << logn
    rng = SplitMix(8300 + logn)
    s_to, s_from = M.lazy_rows(rng, (L + k, n), mext), M.lazy_rows(rng, (L + k, n), mext)
    draws = Draws(8400 + logn, plant=plant_edges)
    exp = keygen(orc, draws, logn, mext, L, k, alpha, centred(orc, mext, s_to), centred(orc, mext, s_from))
    assert canonical(exp, mext)
    a = draws.a[0]
    for m, q in enumerate(mext):
        assert {0, q - 1, q, 2 * q - 1} <= set(int(w) for w in a[m, edge_positions(n)]) and int(a[m].max()) < 2 * q
    d_a, d_e = draws.device_rows(eng, 1)
    got = eng.to_host(eng.hks_keygen(mext, k, alpha, eng.to_device(s_to), eng.to_device(s_from[None]), d_a, d_e))
    assert np.array_equal(got[0], exp)


# ---- 4. off-table and wide moduli ---------------------------------------------------------------------------------------------------
def offtable_chain(name, L, k):
    if name == "HIGHMID+W59":
        return M.HIGHMID[:3] + M.W59[-2:]
    return M.CHAINS[name][:L] + M.CHAINS[name][-k:]


@pytest.mark.parametrize("name", ["W59", "ABOVE", "HIGHMID+W59"])
def test_keygen_on_offtable_moduli(eng, orc, name):
    logn, L, k, alpha, keys = 11, 3, 2, 2, 2
    mext = offtable_chain(name, L, k)
    case = model_case(orc, logn, L, k, alpha, keys, mext=mext, tag=name)
    if name == "HIGHMID+W59":
        # the premise of this chain: the transformed error rows the fused kernel reads are NOT lazy words below 2q
        e = case[3].e[0]
        e_ntt = orc.poly_ntt(mext, np.stack([(e % q).astype(U) for q in mext]))
        assert (e_ntt >= 2 * np.array(mext, dtype=U)[:, None]).any()
    assert canonical(case[4], mext)
    assert np.array_equal(device_keys(eng, case, k, alpha), case[4])


# ---- 5. parity level A ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha,keys", [(11, 4, 2, 2, 2), (12, 5, 1, 3, 1)])
def test_keygen_at_parity_level_a(eng, orc, logn, L, k, alpha, keys):
    """canonical output: level A gives the words of level B exactly, whatever the transform of the error rows leaves in between"""
    case = model_case(orc, logn, L, k, alpha, keys)
    b_words = device_keys(eng, case, k, alpha)
    eng.set_parity_level("A")
    try:
        a_words = device_keys(eng, case, k, alpha)
        eng.sync()
    finally:
        eng.set_parity_level("B")
    assert np.array_equal(b_words, case[4])
    assert np.array_equal(a_words, b_words)


# ---- 6. rotation keys -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,L,k,alpha", [(5, 4, 2, 2), (11, 4, 2, 2)])
def test_rotation_keys_match_the_model_and_rotate(eng, orc, logn, L, k, alpha):
    """decryption_setup's direction: key r switches move_r(s) back to s.  Steps 0, a duplicate, N/2 + 1 and two conjugations."""
    mext = P.P40[:L] + P.P50[:k]
    n, q = 1 << logn, mext[:L]
    steps, conj = rotations_of(logn, 6)
    rots = list(zip(steps, conj))
    draws = Draws(8600 + logn)
    s_ntt, keys = decryption_setup(orc, draws, logn, mext, L, k, alpha, rots)
    exp = np.stack(keys)
    d_s = eng.poly_from_signed(mext, dev_i64(eng, draws.secrets[0][None]))[0]
    d_a, d_e = draws.device_rows(eng, len(rots))
    d_keys = eng.hks_keygen_rot(mext, k, alpha, d_s, steps, d_a, d_e, conj)
    assert np.array_equal(eng.to_host(d_keys), exp)
    # the generated keys at work: the same words in, so the same words out, and they decrypt to the rotated plaintext
    ct = SplitMix(8700 + logn).poly((2, L, n), q)
    d_ct = eng.to_device(ct[None])
    got = eng.to_host(eng.ckks_rotate_hoisted_hks(mext, k, alpha, d_ct, [d_keys[r] for r in range(len(rots))], steps, conj))[0]
    ref = eng.to_host(eng.ckks_rotate_hoisted_hks(mext, k, alpha, d_ct, [eng.to_device(key) for key in keys], steps, conj))[0]
    assert np.array_equal(got, ref)
    err_got, err_ref = (decryption_errors(orc, logn, q, ct, s_ntt, rots, outs) for outs in (got, ref))
    Q = 1
    for m in q:
        Q *= m
    for worst, worst_ref in zip(err_got, err_ref):
        assert worst <= worst_ref and worst < (1 << 24) and worst * (1 << 60) < Q, (worst, worst_ref)


def test_rotation_key_list_longer_than_one_argument_table(eng, orc):
    """34 entries: the fused kernel takes its maps as arguments, 32 to a launch -- the second launch starts at key 32"""
    logn, L, k, alpha = 5, 2, 1, 1
    mext = P.P40[:L] + P.P50[:k]
    steps, conj = rotations_of(logn, 34)
    draws = Draws(8650)
    _, keys = decryption_setup(orc, draws, logn, mext, L, k, alpha, list(zip(steps, conj)))
    d_s = eng.poly_from_signed(mext, dev_i64(eng, draws.secrets[0][None]))[0]
    d_a, d_e = draws.device_rows(eng, len(steps))
    assert np.array_equal(eng.to_host(eng.hks_keygen_rot(mext, k, alpha, d_s, steps, d_a, d_e, conj)), np.stack(keys))


# ---- 7. relinearisation, end to end ---------------------------------------------------------------------------------------------------
def test_relinearisation_key_end_to_end(eng, orc):
    logn, L, k, alpha = 11, 4, 2, 2
    mext, n = chain(L, k), 1 << 11
    rng = SplitMix(8800)
    s = ternary(rng, n)
    s_rows = secret_rows(orc, mext, s)
    draws = Draws(8801)
    exp = keygen(orc, draws, logn, mext, L, k, alpha, s, centred(orc, mext, orc.poly_mul(mext, s_rows, s_rows)))
    d_s = eng.poly_from_signed(mext, dev_i64(eng, s[None]))            # [1][E][n]
    d_a, d_e = draws.device_rows(eng, 1)
    d_key = eng.hks_keygen(mext, k, alpha, d_s[0], eng.poly_mul(mext, d_s, d_s), d_a, d_e)
    assert np.array_equal(eng.to_host(d_key)[0], exp)
    ct1, ct2 = (eng.to_device(rng.poly((1, 2, L, n), mext[:L])) for _ in range(2))
    got = eng.to_host(eng.ckks_mult_hks(mext, k, alpha, ct1, ct2, d_key[0]))
    ref = eng.to_host(eng.ckks_mult_hks(mext, k, alpha, ct1, ct2, eng.to_device(exp)))
    assert np.array_equal(got, ref)


# ---- 8. poly_from_signed --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [5, 11])
def test_poly_from_signed(eng, orc, logn):
    """every int64: residues by Python integers (a negative c is q - (|c| mod q), and 0 where that is q), then the oracle's transform"""
    moduli = P.P40[:3] + [M.HIGHMID[0]]
    n, B = 1 << logn, 2
    rng = SplitMix(8900 + logn)
    coeffs = (rng.words(B * n, 17).astype(np.int64) - 8).reshape(B, n)
    planted = [0, 1, -1, 8, -8, 2**63 - 1, -2**63, -2**63 + 1]
    for q in moduli:
        planted += [q, -q, q - 1, -(q - 1)]
    assert len(planted) <= n
    coeffs[0, :len(planted)] = planted
    coeffs[1, n - len(planted):] = planted[::-1]
    got = eng.to_host(eng.poly_from_signed(moduli, dev_i64(eng, coeffs)))
    assert got.shape == (B, len(moduli), n)
    for b in range(B):
        residues = np.array([[int(c) % q for c in coeffs[b]] for q in moduli], dtype=U)
        assert np.array_equal(got[b], orc.poly_ntt(moduli, residues)), b


# ---- 9. refusals before anything is enqueued -------------------------------------------------------------------------------------------
FILL = 0x5A5A5A5A5A5A5A5A


def test_refusals_leave_the_output_untouched(eng):
    from hehub_amd import capi

    logn, L, k, alpha, keys = 5, 4, 2, 2, 2
    n, E, nd = 1 << logn, L + k, 2
    mext = P.P40[:L] + P.P50[:k]
    marr = (capi.u64 * E)(*mext)
    s_to, s_from, a = eng.empty((E, n)).zero_(), eng.empty((keys, E, n)).zero_(), eng.empty((keys, nd, E, n)).zero_()
    e = eng.torch.zeros((keys, nd, n), dtype=eng.torch.int64, device=a.device)
    kwords = keys * nd * 2 * E * n
    # the key buffer in the middle of a larger one: room for the overlap cases on either side
    big = eng.empty((3 * kwords,)).fill_(FILL)
    out = big.data_ptr() + 8 * kwords
    steps = (C.c_size_t * keys)(1, 2)
    ptr = lambda t: t.data_ptr()

    def untouched():
        eng.sync()
        return bool((big == FILL).all())

    def gen(**kw):
        v = dict(logn=logn, L=L, k=k, alpha=alpha, m=marr, keys=keys, s_to=ptr(s_to), s_from=ptr(s_from), a=ptr(a), e=ptr(e), out=out)
        v.update(kw)
        return eng.lib.hp_dev_hks_keygen(eng.h, v["logn"], v["L"], v["k"], v["alpha"], v["m"], v["keys"], C.c_void_p(v["s_to"]),
                                         C.c_void_p(v["s_from"]), C.c_void_p(v["a"]), C.c_void_p(v["e"]), C.c_void_p(v["out"]))

    def rot(**kw):
        v = dict(logn=logn, L=L, k=k, alpha=alpha, m=marr, keys=keys, steps=steps, conj=None, s=ptr(s_to), a=ptr(a), e=ptr(e), out=out)
        v.update(kw)
        return eng.lib.hp_dev_hks_keygen_rot(eng.h, v["logn"], v["L"], v["k"], v["alpha"], v["m"], v["keys"], v["steps"], v["conj"],
                                             C.c_void_p(v["s"]), C.c_void_p(v["a"]), C.c_void_p(v["e"]), C.c_void_p(v["out"]))

    coeffs = eng.torch.zeros((2, n), dtype=eng.torch.int64, device=a.device)
    qarr = (capi.u64 * L)(*mext[:L])

    def signed(**kw):
        v = dict(logn=logn, L=L, m=qarr, batch=2, coeffs=ptr(coeffs), out=out)
        v.update(kw)
        return eng.lib.hp_dev_poly_from_signed(eng.h, v["logn"], v["L"], v["m"], v["batch"], C.c_void_p(v["coeffs"]), C.c_void_p(v["out"]))

    refused = []
    # NULL pointers (d_a and conj excepted)
    refused += [gen(m=None), gen(s_to=None), gen(s_from=None), gen(e=None), gen(out=None)]
    refused += [rot(m=None), rot(steps=None), rot(s=None), rot(e=None), rot(out=None)]
    refused += [signed(m=None), signed(coeffs=None), signed(out=None)]
    # the shape limits of hp_dev_hks_switch
    for bad in (dict(alpha=0), dict(alpha=9), dict(k=0), dict(k=17), dict(L=31), dict(L=0)):
        refused += [gen(**bad), rot(**bad)]
    refused += [signed(L=0), signed(L=33)]
    # nothing to do
    refused += [gen(keys=0), rot(keys=0), signed(batch=0)]
    # a step out of range on an entry that is not a conjugation
    far = (C.c_size_t * keys)(1, 1 << 17)
    refused += [rot(steps=far), rot(steps=far, conj=(C.c_ubyte * keys)(1, 0))]
    # misaligned pointers
    refused += [gen(s_to=ptr(s_to) + 8), gen(s_from=ptr(s_from) + 8), gen(a=ptr(a) + 8), gen(e=ptr(e) + 8), gen(out=out + 8)]
    refused += [rot(s=ptr(s_to) + 8), rot(a=ptr(a) + 8), rot(e=ptr(e) + 8), rot(out=out + 8)]
    refused += [signed(coeffs=ptr(coeffs) + 8), signed(out=out + 8)]
    # the output overlapping an input: the input's last 16 bytes on the output's first, and the input starting inside the output
    last = out + 8 * kwords - 16
    for name, words in (("s_to", E * n), ("s_from", keys * E * n), ("a", keys * nd * E * n), ("e", keys * nd * n)):
        refused += [gen(**{name: out - 8 * words + 16}), gen(**{name: last})]
    for name, words in (("s", E * n), ("a", keys * nd * E * n), ("e", keys * nd * n)):
        refused += [rot(**{name: out - 8 * words + 16}), rot(**{name: last})]
    refused += [signed(coeffs=out - 8 * 2 * n + 16), signed(coeffs=out + 8 * 2 * L * n - 16)]
    assert all(rc == capi.HP_EINVAL for rc in refused), refused
    assert untouched()
    # a chain hp_dev_hks_switch refuses is refused with its code (a repeated modulus: not pairwise coprime), before anything is written
    twice = (capi.u64 * E)(*([mext[0]] + mext[:1] + mext[2:]))   # (inside one digit)
    z = eng.empty((1, L, n)).zero_()
    code = eng.lib.hp_dev_hks_switch(eng.h, logn, L, k, alpha, twice, 1, C.c_void_p(ptr(z)), C.c_void_p(ptr(a)), C.c_void_p(out))
    assert code != capi.HP_OK and gen(m=twice) == code and rot(m=twice) == code
    assert untouched()
    # what is allowed: a step out of range under a conjugation, no a rows (they are in the key), adjacent buffers
    assert rot(steps=far, conj=(C.c_ubyte * keys)(0, 1)) == capi.HP_OK
    assert gen(a=None) == capi.HP_OK
    assert gen(s_to=out - 8 * E * n) == capi.HP_OK and signed(coeffs=out + 8 * 2 * L * n) == capi.HP_OK
    eng.sync()
    assert bool((big[:kwords] == FILL).all()) and bool((big[2 * kwords:] == FILL).all())


# ---- 10. workspace ----------------------------------------------------------------------------------------------------------------------
def test_workspace_does_not_grow_with_the_number_of_keys(orc):
    """the error rows are spread and transformed inside the key buffer: no scratch copy of them.  A context of its own, so that no
    earlier call has grown the workspace."""
    from hehub_amd.engine import Engine

    logn, L, k, alpha = 11, 3, 2, 2
    e = Engine(0)
    try:
        sizes = []
        for keys in (1, 3):
            case = model_case(orc, logn, L, k, alpha, keys)
            assert np.array_equal(device_keys(e, case, k, alpha), case[4])
            sizes.append(e.workspace_bytes())
        assert sizes[0] == sizes[1]
    finally:
        e.close()
