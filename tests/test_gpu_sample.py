"""hp_dev_sample_uniform / _ternary / _cbd, hp_dev_hks_keygen_seeded / _rot_seeded, hp_dev_hks_key_expand: sampling on the device.

Everything is a function of (seed, stream), so every word is pinned: the samplers by tests/sample_model.py, the seeded keys twice --
by hp_dev_hks_keygen run on the device-sampled rows, and by keygen() of tests/hks_model.py fed from the sample model through
`SampleDraws`, which stands in for its random source.  Shapes and references are those of tests/sample_cases.py, which
tests/test_sample_host.py holds the host implementation to as well; a model reference is computed once and shared."""
import ctypes as C

import numpy as np
import pytest

import sample_cases as K
import sample_model as S
from gpu_words import dev_i64
from hks_model import centred_error, chain, decryption_errors, keygen, rotations_of
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64
FILL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def signed_host(t):
    return t.detach().cpu().numpy()


# ---- 1. the uniform sampler ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.UNIFORM_CASES))
def test_uniform_equals_the_model(eng, name):
    logn, moduli, batch, stream, ids = K.UNIFORM_CASES[name]
    got = eng.to_host(eng.sample_uniform(logn, moduli, K.SEED, stream, batch, ids))
    assert got.shape == (batch, len(moduli), 1 << logn)
    assert np.array_equal(got, K.model_uniform(logn, moduli, stream, ids, batch))
    assert bool((got < np.array(moduli, dtype=U)[None, :, None]).all())


def test_uniform_with_a_stride_leaves_the_gaps_and_the_guard(eng):
    logn, moduli, batch, stream = K.STRIDE_CASE
    L, n = len(moduli), 1 << logn
    stride = L * n + 64
    buf = eng.empty((batch * stride + 64,)).fill_(FILL)
    eng.sample_uniform(logn, moduli, K.SEED, stream, batch, out=buf, stride_words=stride)
    got = eng.to_host(buf)
    exp = K.model_uniform(logn, moduli, stream, None, batch)
    for b in range(batch):
        assert np.array_equal(got[b * stride:b * stride + L * n].reshape(L, n), exp[b]), b
        assert bool((got[b * stride + L * n:(b + 1) * stride] == FILL).all()), b
    assert bool((got[batch * stride:] == FILL).all())


def test_batch_b_of_a_stream_is_batch_0_of_the_stream_plus_b(eng):
    logn, moduli, s = 5, K.FIVE[:3], 40
    three = eng.to_host(eng.sample_uniform(logn, moduli, K.SEED, s, 3))
    for b in range(3):
        assert np.array_equal(three[b], eng.to_host(eng.sample_uniform(logn, moduli, K.SEED, s + b, 1))[0])
    assert not np.array_equal(three[0], three[1])
    assert not np.array_equal(three[0], eng.to_host(eng.sample_uniform(logn, moduli, K.SEED2, s, 1))[0])


def test_limb_ids_name_the_rows_of_the_longer_chain(eng):
    logn, sub, _, stream, ids = K.UNIFORM_CASES["limb_ids"]
    five = eng.to_host(eng.sample_uniform(logn, K.FIVE, K.SEED, stream))[0]
    got = eng.to_host(eng.sample_uniform(logn, sub, K.SEED, stream, 1, ids))[0]
    assert np.array_equal(got, five[ids])
    assert not np.array_equal(eng.to_host(eng.sample_uniform(logn, sub, K.SEED, stream))[0][2], five[4])   # (default label 2, not 4)


# ---- 2. ternary and centred binomial --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", K.SIGNED_LOGN)
def test_ternary_and_binomial_equal_the_model(eng, logn):
    t = signed_host(eng.sample_ternary(logn, K.SEED, K.SIGNED_STREAM, K.SIGNED_BATCH))
    c = signed_host(eng.sample_cbd(logn, K.SEED, K.SIGNED_STREAM, K.SIGNED_BATCH))
    assert t.dtype == np.int64 and t.shape == c.shape == (K.SIGNED_BATCH, 1 << logn)
    assert np.array_equal(t, K.model_signed(S.TERNARY, logn))
    assert np.array_equal(c, K.model_signed(S.CBD, logn))


def test_the_three_kinds_share_no_keystream(eng):
    """one (seed, stream) under the three kinds: were the keystream shared, the ternary row would be a function of the other two.
    Reduced to signs the rows agree about as often as independent ones (1/3), and no two rows are equal."""
    logn, stream = 11, 33
    u = eng.to_host(eng.sample_uniform(logn, [3], K.SEED, stream, 2)).astype(np.int64)[:, 0] - 1
    t = signed_host(eng.sample_ternary(logn, K.SEED, stream, 2))
    c = signed_host(eng.sample_cbd(logn, K.SEED, stream, 2))
    w = signed_host(eng.sample_cbd(logn, K.SEED, stream + 1, 1))
    rows = [u[0], u[1], t[0], t[1], np.sign(c[0]), np.sign(c[1]), np.sign(w[0])]
    assert np.array_equal(c[1], w[0])   # (batch 1 of a stream is the next stream)
    for i in range(len(rows) - 1):
        for j in range(i + 1, len(rows) - 1):
            assert not np.array_equal(rows[i], rows[j]) and float((rows[i] == rows[j]).mean()) < 0.45, (i, j)


# ---- 3. seeded key generation -----------------------------------------------------------------------------------------------------------------
class SampleDraws:
    """keygen()'s random source, fed from the sample model: for the digits in order, poly() is the uniform sample and words(n, 17) the
    scaled centred-binomial sample (shifted by the 8 keygen() subtracts again) of the next polynomial id"""

    def __init__(self, logn, seed, stream, scale):
        self.logn, self.seed, self.stream, self.scale = logn, seed, stream, scale

    def poly(self, shape, moduli):
        assert shape == (len(moduli), 1 << self.logn)
        return np.array(K.model_uniform(self.logn, moduli, self.stream, None, 1, self.seed)[0])

    def words(self, n, bound=0):
        assert bound == 17 and n == 1 << self.logn
        e = self.scale * S.cbd_row(self.logn, self.seed, self.stream) + 8
        self.stream += 1
        return e


_KEYS = {}


def secrets(logn, keys):
    """ternary s_to and s_from[r], from the sample model"""
    rows = S.sample_ternary(logn, K.SEED2, 500, keys + 1)
    return rows[0], rows[1:]


def model_keys(orc, logn, L, k, alpha, keys, scale):
    at = (logn, L, k, alpha, keys, scale)
    if at not in _KEYS:
        mext, nd = chain(L, k), (L + alpha - 1) // alpha
        s_to, s_from = secrets(logn, keys)
        exp = np.stack([keygen(orc, SampleDraws(logn, K.SEED, K.KEYGEN_STREAM + r * nd, scale), logn, mext, L, k, alpha, s_to, s_from[r])
                        for r in range(keys)])
        exp.setflags(write=False)
        _KEYS[at] = exp
    return _KEYS[at]


def device_secrets(eng, mext, logn, keys):
    s_to, s_from = secrets(logn, keys)
    return eng.poly_from_signed(mext, dev_i64(eng, s_to[None]))[0], eng.poly_from_signed(mext, dev_i64(eng, s_from))


def sampled_rows(eng, mext, logn, count, stream, scale):
    """the rows a seeded call draws, by the samplers themselves: a [count][E][n], e [count][n]"""
    return eng.sample_uniform(logn, mext, K.SEED, stream, count), eng.sample_cbd(logn, K.SEED, stream, count) * scale


@pytest.mark.parametrize("scale", [1, 65537])
@pytest.mark.parametrize("logn,L,k,alpha,keys", K.KEYGEN_CASES)
def test_seeded_keys(eng, orc, logn, L, k, alpha, keys, scale):
    mext, nd, E, n = chain(L, k), (L + alpha - 1) // alpha, L + k, 1 << logn
    d_to, d_from = device_secrets(eng, mext, logn, keys)
    got = eng.to_host(eng.hks_keygen_seeded(mext, k, alpha, d_to, d_from, K.SEED, K.KEYGEN_STREAM, scale))
    assert got.shape == (keys, nd, 2, E, n)
    # the plain generator on the device-sampled rows
    a, e = sampled_rows(eng, mext, logn, keys * nd, K.KEYGEN_STREAM, scale)
    ref = eng.to_host(eng.hks_keygen(mext, k, alpha, d_to, d_from, a.reshape(keys, nd, E, n), e.reshape(keys, nd, n)))
    assert np.array_equal(got, ref)
    # the exact model fed from the sample model
    assert np.array_equal(got, model_keys(orc, logn, L, k, alpha, keys, scale))
    assert bool((got < np.array(mext, dtype=U)[:, None]).all())
    # parity level A: the same words
    eng.set_parity_level("A")
    try:
        at_a = eng.to_host(eng.hks_keygen_seeded(mext, k, alpha, d_to, d_from, K.SEED, K.KEYGEN_STREAM, scale))
        eng.sync()
    finally:
        eng.set_parity_level("B")
    assert np.array_equal(at_a, got)


@pytest.mark.parametrize("logn,L,k,alpha", [(5, 4, 2, 2), (11, 4, 2, 2)])
def test_seeded_rotation_keys(eng, logn, L, k, alpha):
    mext, nd, E, n = chain(L, k), (L + alpha - 1) // alpha, L + k, 1 << logn
    steps, conj = rotations_of(logn, 6)
    d_s, _ = device_secrets(eng, mext, logn, 1)
    got = eng.to_host(eng.hks_keygen_rot_seeded(mext, k, alpha, d_s, steps, K.SEED, 77, 1, conj))
    a, e = sampled_rows(eng, mext, logn, 6 * nd, 77, 1)
    ref = eng.to_host(eng.hks_keygen_rot(mext, k, alpha, d_s, steps, a.reshape(6, nd, E, n), e.reshape(6, nd, n), conj))
    assert got.shape == (6, nd, 2, E, n) and np.array_equal(got, ref)
    assert not np.array_equal(got[1], got[2])   # (the duplicate step: another polynomial id, another key)


def test_key_expand_restores_the_a_halves_and_leaves_the_b_halves(eng):
    logn, L, k, alpha, keys = 11, 3, 2, 2, 2
    mext = chain(L, k)
    d_to, d_from = device_secrets(eng, mext, logn, keys)
    d_keys = eng.hks_keygen_seeded(mext, k, alpha, d_to, d_from, K.SEED, 90, 1)
    original = eng.to_host(d_keys).copy()
    d_keys[:, :, 1] = 0x1234567
    assert not np.array_equal(eng.to_host(d_keys), original)
    eng.hks_key_expand(mext, k, alpha, d_keys, K.SEED, 90)
    after = eng.to_host(d_keys)
    assert np.array_equal(after[:, :, 0], original[:, :, 0])
    assert np.array_equal(after, original)
    # the [0] halves are not read either: other words there, the same [1] halves
    d_keys[:, :, 0] = 7
    eng.hks_key_expand(mext, k, alpha, d_keys, K.SEED, 90)
    again = eng.to_host(d_keys)
    assert np.array_equal(again[:, :, 1], original[:, :, 1]) and bool((again[:, :, 0] == 7).all())
    # expanded from the sample model: a * 2^64 mod q
    a = K.model_uniform(logn, mext, 90 + 1, None, 1)[0]
    exp = np.array([[int(w) * (1 << 64) % q for w in row[:16]] for row, q in zip(a, mext)], dtype=U)
    assert np.array_equal(original[0, 1, 1][:, :16], exp)


def test_workspace_is_a_function_of_n_dnum_and_keys(eng):
    from hehub_amd.engine import Engine

    logn, keys = 11, 2
    sizes = []
    for L, k in ((3, 2), (4, 1)):   # dnum = 2 either way
        e = Engine(0)
        try:
            mext = chain(L, k)
            d_to, d_from = device_secrets(e, mext, logn, keys)
            assert e.workspace_bytes() == 0
            e.hks_keygen_seeded(mext, k, 2, d_to, d_from, K.SEED, 1, 1)
            e.sync()
            sizes.append(e.workspace_bytes())
        finally:
            e.close()
    assert sizes[0] == sizes[1] and sizes[0] >= keys * 2 * (1 << logn) * 8


# ---- 4. end to end: the noise of a seeded key -----------------------------------------------------------------------------------------------------
def test_seeded_keys_decrypt_within_the_worst_case(eng, orc):
    """secret from sample_ternary, relinearisation key (s_from = s * s) and a rotation key by the seeded calls.  Worst case of
    |out0 + out1 s - pt s_from|: a digit is below its modulus product <= P, |e| <= 21, N terms per digit, plus ModDown's rounding with a
    ternary secret: dnum * 21 * N + N."""
    logn, L, k, alpha = 11, 3, 2, 2
    mext, n, nd = chain(L, k), 1 << logn, 2
    q = mext[:L]
    bound = nd * 21 * n + n
    d_s = eng.poly_from_signed(mext, eng.sample_ternary(logn, K.SEED2, 600, 1))           # [1][E][n]
    s_ntt = orc.poly_reduce_strict(q, np.ascontiguousarray(eng.to_host(d_s)[0, :L]))
    assert np.array_equal(signed_host(eng.sample_ternary(logn, K.SEED2, 600, 1)), S.sample_ternary(logn, K.SEED2, 600, 1))
    d_s2 = eng.poly_mul(mext, d_s, d_s)
    d_key = eng.hks_keygen_seeded(mext, k, alpha, d_s[0], d_s2, K.SEED, 700, 1)
    pt = SplitMix(9100).poly((1, L, n), q)
    out = eng.to_host(eng.hks_switch(mext, k, alpha, eng.to_device(pt), d_key[0]))[0]
    s2 = orc.poly_mul(q, s_ntt, s_ntt)
    lhs = orc.poly_add(q, np.ascontiguousarray(out[0]), orc.poly_mul(q, np.ascontiguousarray(out[1]), s_ntt))
    err = centred_error(orc, logn, q, orc.poly_sub(q, lhs, orc.poly_mul(q, pt[0], s2)))
    print("relinearisation key: error", err, "bound", bound)
    assert err <= bound
    # a rotation key through the hoisted rotation
    steps, conj = [3, 0], [False, True]
    d_rot = eng.hks_keygen_rot_seeded(mext, k, alpha, d_s[0], steps, K.SEED, 800, 1, conj)
    ct = SplitMix(9101).poly((2, L, n), q)
    outs = eng.to_host(eng.ckks_rotate_hoisted_hks(mext, k, alpha, eng.to_device(ct[None]), [d_rot[0], d_rot[1]], steps, conj))[0]
    errs = decryption_errors(orc, logn, q, ct, s_ntt, list(zip(steps, conj)), outs)
    print("rotation keys: errors", errs, "bound", bound)
    assert all(e <= bound for e in errs)


# ---- 5. refusals before anything is enqueued ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(eng):
    from hehub_amd import capi

    logn, L, k, alpha, keys = 5, 4, 2, 2, 2
    n, E, nd = 1 << logn, L + k, 2
    mext = chain(L, k)
    marr = (capi.u64 * E)(*mext)
    seed = (C.c_ubyte * 32)(*K.SEED)
    s_to, s_from = eng.empty((E, n)).zero_(), eng.empty((keys, E, n)).zero_()
    kwords = keys * nd * 2 * E * n
    big = eng.empty((3 * kwords,)).fill_(FILL)
    out = big.data_ptr() + 8 * kwords
    steps = (C.c_size_t * keys)(1, 2)
    ptr = lambda t: t.data_ptr()
    lib, h, vp = eng.lib, eng.h, C.c_void_p

    def untouched():
        eng.sync()
        return bool((big == FILL).all())

    def uni(**kw):
        v = dict(logn=logn, L=E, m=marr, ids=None, batch=2, seed=seed, stream=1, stride=0, out=out)
        v.update(kw)
        return lib.hp_dev_sample_uniform(h, v["logn"], v["L"], v["m"], v["ids"], v["batch"], v["seed"], v["stream"], v["stride"], vp(v["out"]))

    def sgn(fn, **kw):
        v = dict(logn=logn, batch=2, seed=seed, stream=1, out=out)
        v.update(kw)
        return fn(h, v["logn"], v["batch"], v["seed"], v["stream"], vp(v["out"]))

    def gen(**kw):
        v = dict(logn=logn, L=L, k=k, alpha=alpha, m=marr, keys=keys, s_to=ptr(s_to), s_from=ptr(s_from), seed=seed, stream=1, scale=1, out=out)
        v.update(kw)
        return lib.hp_dev_hks_keygen_seeded(h, v["logn"], v["L"], v["k"], v["alpha"], v["m"], v["keys"], vp(v["s_to"]), vp(v["s_from"]),
                                            v["seed"], v["stream"], v["scale"], vp(v["out"]))

    def rot(**kw):
        v = dict(logn=logn, L=L, k=k, alpha=alpha, m=marr, keys=keys, steps=steps, conj=None, s=ptr(s_to), seed=seed, stream=1, scale=1, out=out)
        v.update(kw)
        return lib.hp_dev_hks_keygen_rot_seeded(h, v["logn"], v["L"], v["k"], v["alpha"], v["m"], v["keys"], v["steps"], v["conj"],
                                                vp(v["s"]), v["seed"], v["stream"], v["scale"], vp(v["out"]))

    def exp(**kw):
        v = dict(logn=logn, L=L, k=k, alpha=alpha, m=marr, keys=keys, seed=seed, stream=1, out=out)
        v.update(kw)
        return lib.hp_dev_hks_key_expand(h, v["logn"], v["L"], v["k"], v["alpha"], v["m"], v["keys"], v["seed"], v["stream"], vp(v["out"]))

    tern, cbd = lib.hp_dev_sample_ternary, lib.hp_dev_sample_cbd
    refused = []
    # the ring degree: below one block, above the engine's limit
    for bad in (0, 2, 17):
        refused += [uni(logn=bad), sgn(tern, logn=bad), sgn(cbd, logn=bad), gen(logn=bad), rot(logn=bad), exp(logn=bad)]
    # the number of moduli; nothing to do
    refused += [uni(L=0), uni(L=33, m=(capi.u64 * 33)(*([mext[0]] * 33))), gen(L=0), rot(L=0), exp(L=0), gen(L=31), rot(L=31), exp(L=31)]
    refused += [uni(batch=0), sgn(tern, batch=0), sgn(cbd, batch=0), gen(keys=0), rot(keys=0), exp(keys=0)]
    # moduli a word cannot be drawn for
    for q in (0, 1, 1 << 63, (1 << 64) - 1):
        refused += [uni(m=(capi.u64 * E)(*(mext[:2] + [q] + mext[3:])))]
    # limb ids, strides
    refused += [uni(ids=(C.c_uint32 * E)(0, 1, 256, 3, 4, 5)), uni(ids=(C.c_uint32 * E)(0, 1, 2, 3, 4, 1 << 31))]
    refused += [uni(stride=E * n - 2), uni(stride=E * n + 1), uni(stride=1), uni(stride=2)]
    # pointers: NULL, misaligned; a NULL seed
    refused += [uni(m=None), uni(out=None), uni(out=out + 8), uni(seed=None)]
    refused += [sgn(f, out=None) for f in (tern, cbd)] + [sgn(f, out=out + 8) for f in (tern, cbd)] + [sgn(f, seed=None) for f in (tern, cbd)]
    refused += [gen(m=None), gen(s_to=None), gen(s_from=None), gen(out=None), gen(seed=None)]
    refused += [gen(s_to=ptr(s_to) + 8), gen(s_from=ptr(s_from) + 8), gen(out=out + 8)]
    refused += [rot(m=None), rot(steps=None), rot(s=None), rot(out=None), rot(seed=None), rot(s=ptr(s_to) + 8), rot(out=out + 8)]
    refused += [exp(m=None), exp(out=None), exp(seed=None), exp(out=out + 8)]
    # the error scale: 21 * scale must fit an int64
    for bad in (0, 1 << 58, (1 << 64) - 1):
        refused += [gen(scale=bad), rot(scale=bad)]
    # what the plain generators refuse: digit sizes, special primes, a far step, the output overlapping an input
    for bad in (dict(alpha=0), dict(alpha=9), dict(k=0), dict(k=17)):
        refused += [gen(**bad), rot(**bad), exp(**bad)]
    far = (C.c_size_t * keys)(1, 1 << 17)
    refused += [rot(steps=far), rot(steps=far, conj=(C.c_ubyte * keys)(1, 0))]
    last = out + 8 * kwords - 16
    refused += [gen(s_to=out - 8 * E * n + 16), gen(s_to=last), gen(s_from=out - 8 * keys * E * n + 16), gen(s_from=last),
                rot(s=out - 8 * E * n + 16), rot(s=last)]
    assert all(rc == capi.HP_EINVAL for rc in refused), refused
    assert untouched()
    # a chain hp_dev_hks_keygen refuses is refused with its code (a repeated modulus), before anything is written
    twice = (capi.u64 * E)(*([mext[0]] + mext[:1] + mext[2:]))
    zeros_e = eng.torch.zeros((keys, nd, n), dtype=eng.torch.int64, device=s_to.device)
    code = lib.hp_dev_hks_keygen(h, logn, L, k, alpha, twice, keys, vp(ptr(s_to)), vp(ptr(s_from)), None, vp(ptr(zeros_e)), vp(out))
    assert code != capi.HP_OK and gen(m=twice) == code and rot(m=twice) == code and exp(m=twice) == code
    assert untouched()
    # what is allowed: the largest scale, the largest limb id, an exact stride, a far step under a conjugation, adjacent buffers
    assert gen(scale=(1 << 58) - 1) == capi.HP_OK and rot(steps=far, conj=(C.c_ubyte * keys)(0, 1)) == capi.HP_OK
    assert exp() == capi.HP_OK and gen(s_to=out - 8 * E * n) == capi.HP_OK
    assert uni(ids=(C.c_uint32 * E)(255, 0, 1, 2, 3, 4), stride=E * n) == capi.HP_OK
    assert sgn(tern) == capi.HP_OK and sgn(cbd, logn=3) == capi.HP_OK
    eng.sync()
    assert bool((big[:kwords] == FILL).all()) and bool((big[2 * kwords:] == FILL).all())
