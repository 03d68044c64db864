"""hp_dev_sample_gauss and the four seeded calls under hp_ctx_set_error_sampler(4): discrete Gaussian
errors drawn on the device.

Everything is a function of (seed, stream) and the inputs, so every word is pinned: the sampler by tests/gauss_model.py (itself held to
the header's table and rule on the CPU, tests/test_gauss_host.py), the seeded calls by the composition of the sampler calls with the
plain calls that were there before, and by exact decryption against the model's rows.  Shapes and shared references:
tests/gauss_cases.py, tests/rlwe_seeded_cases.py."""
import ctypes as C

import numpy as np
import pytest

import gauss_cases as GC
import gauss_model as G
import rlwe_seeded_cases as RC
import rlwe_seeded_model as R
import sample_model as S
from hks_model import chain

pytestmark = pytest.mark.gpu
U = np.uint64
FILL = 0x5A5A5A5A5A5A5A5A
CBD, GAUSS = S.CBD, G.GAUSS


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture
def gauss(eng):
    """the module's engine with the Gaussian error sampler, put back to the default afterwards"""
    eng.set_error_sampler(GAUSS)
    yield eng
    eng.set_error_sampler(CBD)


def signed_host(t):
    return t.detach().cpu().numpy()


def below(got, moduli):
    return bool((got < np.array(moduli, dtype=U)[:, None]).all())


def strict(orc, moduli, rows):
    """poly_reduce_strict over the leading axes of [..][L][n]"""
    L, n = rows.shape[-2:]
    flat = np.ascontiguousarray(rows).reshape(-1, L, n)
    return np.stack([orc.poly_reduce_strict(moduli, np.ascontiguousarray(r)) for r in flat]).reshape(rows.shape)


def at_level_a(eng, call):
    eng.set_parity_level("A")
    try:
        out = eng.to_host(call())
        eng.sync()
    finally:
        eng.set_parity_level("B")
    return out


def mod_rows(rows, moduli):
    """object rows [L][n] -> u64, plain %"""
    return np.array([[int(v) % q for v in row] for row, q in zip(rows, moduli)], dtype=U)


def obj(a):
    return np.asarray(a).astype(object)


def model_error_ntt(orc, logn, moduli, stream, scale):
    """NTT(scale * the model's Gaussian row of the id `stream`), canonical"""
    return R.forward(orc, moduli, G.residues(moduli, G.gauss_row(logn, GC.SEED, stream), scale))


# ---- 1. signed rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,batch", GC.SIGNED_SHAPES)
def test_signed_rows_equal_the_model(eng, logn, batch):
    got = signed_host(eng.sample_gauss(logn, GC.SEED, GC.SIGNED_STREAM, batch))
    assert got.dtype == np.int64 and got.shape == (batch, 1 << logn)
    assert np.array_equal(got, GC.model_signed(logn, batch))
    assert -30 <= int(got.min()) and int(got.max()) <= 30


def test_polynomial_b_of_a_stream_is_polynomial_0_of_the_stream_plus_b(eng):
    logn, batch = GC.SIGNED_SHAPES[-1]
    rows = signed_host(eng.sample_gauss(logn, GC.SEED, GC.SIGNED_STREAM, batch))
    for b in range(batch):
        assert np.array_equal(rows[b], signed_host(eng.sample_gauss(logn, GC.SEED, GC.SIGNED_STREAM + b, 1))[0]), b
    assert not np.array_equal(rows[0], rows[1])
    assert not np.array_equal(rows[0], signed_host(eng.sample_gauss(logn, GC.SEED2, GC.SIGNED_STREAM, 1))[0])
    assert not np.array_equal(rows[0], signed_host(eng.sample_cbd(logn, GC.SEED, GC.SIGNED_STREAM, 1))[0])
    # the ids are 64-bit: the carry into word 15 and the wrap
    for stream in ((1 << 32) - 1, (1 << 64) - 1):
        assert np.array_equal(signed_host(eng.sample_gauss(3, GC.SEED, stream, 2)), G.sample_gauss(3, GC.SEED, stream, 2))


# ---- 2. the residue rows of the ciphertext calls (k_gauss_spread), through the zero-plaintext encryption ------------------------------------
def zero_encryption_carries_the_model_rows(eng, orc, logn, moduli, stream, scale, batch):
    """c0 + a * s = NTT(scale * the model's row) in every modulus, for the zero plaintext; the same words at parity level A"""
    sk = eng.sample_small_ntt(logn, moduli, S.TERNARY, GC.SEED2, RC.SECRET_STREAM)[0]
    s_ntt = eng.to_host(sk)
    call = lambda: eng.rlwe_encrypt_seeded(moduli, sk, None, GC.SEED, stream, scale, batch=batch)
    got = eng.to_host(call())
    assert got.shape == (batch, 2, len(moduli), 1 << logn) and below(got, moduli)
    assert np.array_equal(got[:, 1], eng.to_host(eng.sample_uniform(logn, moduli, GC.SEED, stream, batch)))
    for b in range(batch):
        lhs = mod_rows(obj(got[b, 0]) + obj(got[b, 1]) * obj(s_ntt), moduli)
        assert np.array_equal(lhs, model_error_ntt(orc, logn, moduli, stream + b, scale)), (scale, b)
    assert np.array_equal(got, at_level_a(eng, call)), scale


@pytest.mark.parametrize("logn,batch", [(3, 3), (11, 2)])
def test_error_rows_on_a_59_bit_modulus_off_the_table(gauss, orc, logn, batch):
    moduli = GC.WIDE
    assert len(moduli) == 3 and max(moduli).bit_length() == 59 and R.chain_supports(orc, logn, moduli)
    for scale in GC.SCALES:
        zero_encryption_carries_the_model_rows(gauss, orc, logn, moduli, 70 + logn, scale, batch)


def test_error_rows_take_the_division_path_and_the_largest_scale(gauss, orc):
    """65537 is below 30 * 65537: hp_sample_residue divides (65537 = 2^16 + 1 admits the ring degrees up to 2^15); at 2^58 - 1 it divides
    in every modulus and 30 * scale still fits an int64"""
    zero_encryption_carries_the_model_rows(gauss, orc, 5, [RC.TABLE[0], 65537, RC.TABLE[2]], 91, 65537, 2)
    zero_encryption_carries_the_model_rows(gauss, orc, 3, RC.TABLE, 1, (1 << 58) - 1, 1)


# ---- 3. seeded secret-key encryption ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n8_L3_B3", "n32_L3_B1_t", "n2048_L3_B3_t"])
def test_encrypt_seeded_carries_exactly_the_gaussian_error(gauss, orc, name):
    eng = gauss
    logn, moduli, batch, scale, stream = RC.CASES[name]
    L, n = len(moduli), 1 << logn
    sk = eng.sample_small_ntt(logn, moduli, S.TERNARY, GC.SEED2, RC.SECRET_STREAM)[0]
    s_ntt = RC.secret_ntt(orc, logn, moduli)
    assert np.array_equal(eng.to_host(sk), s_ntt)
    pt = RC.plaintext(name)
    d_pt = eng.to_device(np.array(pt))
    a = eng.to_host(eng.sample_uniform(logn, moduli, GC.SEED, stream, batch))
    outs = {}
    for with_pt in (True, False):
        full = eng.to_host(eng.rlwe_encrypt_seeded(moduli, sk, d_pt if with_pt else None, GC.SEED, stream, scale, batch=batch))
        c0 = eng.to_host(eng.rlwe_encrypt_seeded(moduli, sk, d_pt if with_pt else None, GC.SEED, stream, scale, with_c1=False, batch=batch))
        assert full.shape == (batch, 2, L, n) and below(full, moduli) and c0.shape == (batch, L, n)
        assert np.array_equal(full[:, 1], a)                      # the c1 rows are still hp_dev_sample_uniform's
        assert np.array_equal(c0, full[:, 0])
        for b in range(batch):
            lhs = obj(full[b, 0]) + obj(a[b]) * obj(s_ntt)
            if with_pt:
                lhs = lhs - obj(R.forward(orc, moduli, pt[b]))
            assert np.array_equal(mod_rows(lhs, moduli), model_error_ntt(orc, logn, moduli, stream + b, scale)), (with_pt, b)
        outs[with_pt] = (full, c0)
        # the same words at parity level A
        assert np.array_equal(full, at_level_a(eng, lambda: eng.rlwe_encrypt_seeded(moduli, sk, d_pt if with_pt else None, GC.SEED, stream,
                                                                                     scale, batch=batch)))
        assert np.array_equal(c0, at_level_a(eng, lambda: eng.rlwe_encrypt_seeded(moduli, sk, d_pt if with_pt else None, GC.SEED, stream,
                                                                                   scale, with_c1=False, batch=batch)))
    assert not np.array_equal(outs[True][0][:, 0], outs[False][0][:, 0])
    # and it is another ciphertext than the binomial one
    eng.set_error_sampler(CBD)
    assert not np.array_equal(outs[True][0][:, 0], eng.to_host(eng.rlwe_encrypt_seeded(moduli, sk, d_pt, GC.SEED, stream, scale))[:, 0])


# ---- 4. public-key encryption -------------------------------------------------------------------------------------------------------------
def expand(t, batch):
    return t.unsqueeze(0).expand(batch, *t.shape).contiguous()


@pytest.mark.parametrize("name", ["n32_L3_B1_t", "n2048_L3_B3_t"])
def test_encrypt_pk_seeded_is_the_composition_of_the_sampler_and_the_plain_calls(gauss, orc, name):
    eng = gauss
    logn, moduli, batch, scale, stream = RC.CASES[name]
    stream += RC.PK_ENC_OFFSET
    sk = eng.sample_small_ntt(logn, moduli, S.TERNARY, GC.SEED2, RC.SECRET_STREAM)[0]
    pk = eng.rlwe_encrypt_seeded(moduli, sk, None, GC.SEED2, RC.PK_STREAM, scale, batch=1)[0]
    d_pt = eng.to_device(np.array(RC.plaintext(name)))
    got = eng.to_host(eng.rlwe_encrypt_pk_seeded(moduli, pk, d_pt, GC.SEED, stream, scale))
    assert got.shape == (batch, 2, len(moduli), 1 << logn) and below(got, moduli)
    # e0_b, e1_b: the Gaussian samples of the ids stream + 2b, stream + 2b + 1; u_b: the ternary sample of stream + 2b
    e = eng.poly_from_signed(moduli, eng.sample_gauss(logn, GC.SEED, stream, 2 * batch) * scale).view(batch, 2, len(moduli), 1 << logn)
    u = eng.sample_small_ntt(logn, moduli, S.TERNARY, GC.SEED, stream, 2 * batch)[0::2].contiguous()
    ptn = eng.ntt_(moduli, d_pt.clone())
    ct0 = eng.poly_add(moduli, eng.poly_add(moduli, eng.poly_mul(moduli, expand(pk[0], batch), u), e[:, 0].contiguous()), ptn)
    ct1 = eng.poly_add(moduli, eng.poly_mul(moduli, expand(pk[1], batch), u), e[:, 1].contiguous())
    assert np.array_equal(got[:, 0], strict(orc, moduli, eng.to_host(ct0)))
    assert np.array_equal(got[:, 1], strict(orc, moduli, eng.to_host(ct1)))
    assert np.array_equal(got, at_level_a(eng, lambda: eng.rlwe_encrypt_pk_seeded(moduli, pk, d_pt, GC.SEED, stream, scale)))
    # no plaintext: the same call on zeros
    none = eng.to_host(eng.rlwe_encrypt_pk_seeded(moduli, pk, None, GC.SEED, stream, scale, batch=batch))
    assert np.array_equal(none, eng.to_host(eng.rlwe_encrypt_pk_seeded(moduli, pk, eng.empty(tuple(d_pt.shape)).zero_(), GC.SEED, stream, scale)))


def test_public_key_ciphertext_decrypts_to_the_models_error(gauss):
    """dec - pt = error_scale * (u * e_pk + e0 + e1 * s) of the model's rows, exactly (N = 32: the schoolbook products are cheap)"""
    eng = gauss
    name = "n32_L3_B1_t"
    logn, moduli, batch, scale, stream = RC.CASES[name]
    stream += RC.PK_ENC_OFFSET
    pt = RC.plaintext(name)
    sk = eng.sample_small_ntt(logn, moduli, S.TERNARY, GC.SEED2, RC.SECRET_STREAM)[0]
    pk = eng.rlwe_encrypt_seeded(moduli, sk, None, GC.SEED2, RC.PK_STREAM, scale, batch=1)[0]
    ct = eng.rlwe_encrypt_pk_seeded(moduli, pk, eng.to_device(np.array(pt)), GC.SEED, stream, scale)
    dec = eng.to_host(eng.rlwe_decrypt_core(moduli, ct, sk))
    s = RC.secret(logn)
    e_pk = G.gauss_row(logn, GC.SEED2, RC.PK_STREAM)
    for b in range(batch):
        u = S.ternary_row(logn, GC.SEED, stream + 2 * b)
        e0, e1 = G.gauss_row(logn, GC.SEED, stream + 2 * b), G.gauss_row(logn, GC.SEED, stream + 2 * b + 1)
        err = [scale * (x + int(y) + z) for x, y, z in zip(R.negacyclic(u, e_pk), e0, R.negacyclic(e1, s))]
        assert max(abs(v) for v in err) > 0 and all(2 * max(abs(v) for v in err) < q for q in moduli)
        for m, q in enumerate(moduli):
            assert [R.centred(int(d) - int(p), q) for d, p in zip(dec[b, m], pt[b, m])] == err, (b, m)


# ---- 5. seeded keys -----------------------------------------------------------------------------------------------------------------------
KEY_SHAPE = (5, 4, 2, 2)   # logn, L, k, alpha: two digits, the smallest of sample_cases.KEYGEN_CASES


def key_inputs(eng, keys):
    logn, L, k, _ = KEY_SHAPE
    mext = chain(L, k)
    rows = S.sample_ternary(logn, GC.SEED2, 500, keys + 1)
    to_dev = lambda x: eng.torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to(f"cuda:{eng.device}")
    return mext, eng.poly_from_signed(mext, to_dev(rows[:1]))[0], eng.poly_from_signed(mext, to_dev(rows[1:]))


@pytest.mark.parametrize("scale", GC.SCALES)
def test_seeded_keys_are_the_plain_generators_on_the_sampled_rows(gauss, scale):
    eng = gauss
    logn, L, k, alpha = KEY_SHAPE
    nd, E, n, keys, stream = (L + alpha - 1) // alpha, L + k, 1 << logn, 2, 1000
    mext, d_to, d_from = key_inputs(eng, keys)
    got = eng.to_host(eng.hks_keygen_seeded(mext, k, alpha, d_to, d_from, GC.SEED, stream, scale))
    a = eng.sample_uniform(logn, mext, GC.SEED, stream, keys * nd).reshape(keys, nd, E, n)
    e = (eng.sample_gauss(logn, GC.SEED, stream, keys * nd) * scale).reshape(keys, nd, n)
    assert np.array_equal(signed_host(e).reshape(keys * nd, n), scale * G.sample_gauss(logn, GC.SEED, stream, keys * nd))
    ref = eng.to_host(eng.hks_keygen(mext, k, alpha, d_to, d_from, a, e))
    assert got.shape == (keys, nd, 2, E, n) and np.array_equal(got, ref)
    assert bool((got < np.array(mext, dtype=U)[:, None]).all())
    assert np.array_equal(got, at_level_a(eng, lambda: eng.hks_keygen_seeded(mext, k, alpha, d_to, d_from, GC.SEED, stream, scale)))
    # rotation keys: a duplicate step and a conjugation
    steps, conj = [1, 1, 0], [False, False, True]
    rot = eng.to_host(eng.hks_keygen_rot_seeded(mext, k, alpha, d_to, steps, GC.SEED, stream + 77, scale, conj))
    a = eng.sample_uniform(logn, mext, GC.SEED, stream + 77, 3 * nd).reshape(3, nd, E, n)
    e = (eng.sample_gauss(logn, GC.SEED, stream + 77, 3 * nd) * scale).reshape(3, nd, n)
    assert np.array_equal(rot, eng.to_host(eng.hks_keygen_rot(mext, k, alpha, d_to, steps, a, e, conj)))
    assert not np.array_equal(rot[0], rot[1])
    # the binomial keys are other keys, their a-halves the same
    eng.set_error_sampler(CBD)
    cbd = eng.to_host(eng.hks_keygen_seeded(mext, k, alpha, d_to, d_from, GC.SEED, stream, scale))
    assert np.array_equal(cbd[:, :, 1], got[:, :, 1]) and not np.array_equal(cbd[:, :, 0], got[:, :, 0])


# ---- 6. the setting: default, fork, refusals; unchanged behaviour -------------------------------------------------------------------------
def four_calls(e, logn=5):
    """the words of the four seeded calls on one small shape, as host arrays.  e may be a lane, whose stream is not torch's: torch's
    copies are waited for before the lane reads them, and the lane before torch reads what it wrote"""
    moduli, L, k, alpha = RC.TABLE, *KEY_SHAPE[1:]
    mext = chain(L, k)
    rows = S.sample_ternary(logn, GC.SEED2, 500, 2)
    coeffs = e.torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(f"cuda:{e.device}")
    e.torch.cuda.synchronize()
    secrets = e.poly_from_signed(mext, coeffs)
    sk = e.sample_small_ntt(logn, moduli, S.TERNARY, GC.SEED2, RC.SECRET_STREAM)[0]
    pk = e.rlwe_encrypt_seeded(moduli, sk, None, GC.SEED2, RC.PK_STREAM, 1, batch=1)[0]
    outs = [e.hks_keygen_seeded(mext, k, alpha, secrets[0], secrets[1:], GC.SEED, 11, 3),
            e.hks_keygen_rot_seeded(mext, k, alpha, secrets[0], [1, 2], GC.SEED, 12, 3),
            e.rlwe_encrypt_seeded(moduli, sk, None, GC.SEED, 13, 3, batch=2),
            e.rlwe_encrypt_pk_seeded(moduli, pk, None, GC.SEED, 14, 3, batch=2)]
    e.sync()
    return [e.to_host(t) for t in outs]


def same(xs, ys):
    return all(np.array_equal(x, y) for x, y in zip(xs, ys))


def test_default_sampler_fork_and_refused_settings():
    from hehub_amd import capi
    from hehub_amd.engine import Engine, InvalidArgument

    e = Engine(0)
    lane = child = None
    try:
        assert e.get_error_sampler() == CBD == 3
        never_set = four_calls(e)
        e.set_error_sampler(CBD)
        assert same(never_set, four_calls(e))
        # the default draws the binomial rows: what the call wrote before the setting existed
        sk = e.sample_small_ntt(5, RC.TABLE, S.TERNARY, GC.SEED2, RC.SECRET_STREAM)[0]
        a, err = e.sample_uniform(5, RC.TABLE, GC.SEED, 13, 2), e.sample_cbd(5, GC.SEED, 13, 2) * 3
        lazy = e.to_host(e.rlwe_encrypt_core(RC.TABLE, err, a, e.empty((2, 3, 32)).zero_(), sk))
        assert np.array_equal(never_set[2], np.stack([np.stack([mod_rows(half, RC.TABLE) for half in ct]) for ct in lazy]))
        lane = e.fork()
        assert lane.get_error_sampler() == CBD
        e.set_error_sampler(GAUSS)
        assert e.get_error_sampler() == GAUSS and lane.get_error_sampler() == CBD      # (a lane keeps what it had at the fork)
        child = e.fork()
        assert child.get_error_sampler() == GAUSS
        under_gauss = four_calls(e)
        assert not any(np.array_equal(x, y) for x, y in zip(under_gauss, never_set))
        assert same(under_gauss, four_calls(child))
        assert same(never_set, four_calls(lane))
        # refused kinds leave the setting and the next output as they were
        for bad in (0, 1, 2, 5, 1 << 16 | 4, (1 << 32) - 1):
            with pytest.raises(InvalidArgument):
                e.set_error_sampler(bad)
            assert e.lib.hp_ctx_set_error_sampler(e.h, bad) == capi.HP_EINVAL and b"error sampler" in e.lib.hp_last_error(e.h)
            assert e.get_error_sampler() == GAUSS
        assert same(under_gauss, four_calls(e))
        e.set_error_sampler(CBD)
        assert same(never_set, four_calls(e))
    finally:
        for x in (child, lane, e):
            if x is not None:
                x.close()


def test_refusals_leave_the_output_untouched(eng):
    from hehub_amd import capi

    logn, moduli, batch = 5, RC.TABLE, 2
    L, n = len(moduli), 1 << logn
    marr = (capi.u64 * L)(*moduli)
    seed = (C.c_ubyte * 32)(*GC.SEED)
    words = batch * L * n
    big = eng.empty((3 * words,)).fill_(FILL)
    out = big.data_ptr() + 8 * words
    lib, h, vp = eng.lib, eng.h, C.c_void_p

    def untouched():
        eng.sync()
        return bool((big == FILL).all())

    def gau(**kw):
        v = dict(logn=logn, batch=batch, seed=seed, stream=1, out=out)
        v.update(kw)
        return lib.hp_dev_sample_gauss(h, v["logn"], v["batch"], v["seed"], v["stream"], vp(v["out"]))

    def small(**kw):
        v = dict(logn=logn, L=L, m=marr, batch=batch, kind=GAUSS, seed=seed, stream=1, scale=1, out=out)
        v.update(kw)
        return lib.hp_dev_sample_small_ntt(h, v["logn"], v["L"], v["m"], v["batch"], v["kind"], v["seed"], v["stream"], v["scale"], vp(v["out"]))

    refused = []

    def refuse(rcs):
        for rc in rcs:
            assert rc == capi.HP_EINVAL and lib.hp_last_error(h), rcs
            refused.append(rc)

    # hp_dev_sample_gauss: what hp_dev_sample_cbd refuses -- the ring degree, nothing to do, pointers, the seed
    refuse([gau(logn=bad) for bad in (0, 2, 17)] + [gau(batch=0), gau(out=None), gau(out=out + 8), gau(seed=None)])
    assert gau(batch=(1 << 30) * 256 * 8 // n + 1) == capi.HP_EUNSUPPORTED     # (more blocks than one launch takes)
    # hp_dev_sample_small_ntt takes the ternary and the binomial kind as before: kind 4 is refused like 0, 1 and 5
    for kind in (0, 1, 4, 5, 1 << 16 | 4):
        refuse([small(kind=kind)])
        assert b"2 (ternary) or 3 (centred binomial)" in lib.hp_last_error(h)
    assert len(refused) >= 12 and untouched()
    # what is allowed: one block per row
    assert gau() == capi.HP_OK and gau(logn=3, batch=1) == capi.HP_OK
    assert small(kind=CBD) == capi.HP_OK
    eng.sync()
    assert bool((big[:words] == FILL).all()) and bool((big[2 * words:] == FILL).all())
