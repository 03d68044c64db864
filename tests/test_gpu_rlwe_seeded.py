"""hp_dev_sample_small_ntt, hp_dev_rlwe_encrypt_seeded, hp_dev_rlwe_encrypt_pk_seeded: fresh ciphertexts drawn on the device.

Everything is a function of (seed, stream) and the inputs, so every word is pinned: by the exact model tests/rlwe_seeded_model.py (itself
held to exact decryption on the CPU, tests/test_rlwe_seeded_model.py), by the composition of the calls that were there before
(hp_dev_sample_* + hp_dev_poly_from_signed / hp_dev_rlwe_encrypt_core -- those return hehub's lazy words, so the composition is compared
after poly_reduce_strict), and by the call itself at parity level A.  Shapes, chains and the shared references: tests/rlwe_seeded_cases.py."""
import ctypes as C

import numpy as np
import pytest

import rlwe_seeded_cases as RC
import rlwe_seeded_model as R
import sample_cases as K
import sample_model as S

pytestmark = pytest.mark.gpu
U = np.uint64
FILL = 0x5A5A5A5A5A5A5A5A
NAMES = sorted(RC.CASES)


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def below(got, moduli):
    return bool((got < np.array(moduli, dtype=U)[:, None]).all())


def strict(orc, moduli, rows):
    """poly_reduce_strict over the leading axes of [..][L][n]"""
    L, n = rows.shape[-2:]
    flat = np.ascontiguousarray(rows).reshape(-1, L, n)
    return np.stack([orc.poly_reduce_strict(moduli, np.ascontiguousarray(r)) for r in flat]).reshape(rows.shape)


def device_secret(eng, logn, moduli):
    return eng.sample_small_ntt(logn, moduli, S.TERNARY, K.SEED2, RC.SECRET_STREAM)[0]


def device_plaintext(eng, name):
    return eng.to_device(np.array(RC.plaintext(name)))   # (a copy: the shared reference is read-only)


def at_level_a(eng, call):
    eng.set_parity_level("A")
    try:
        out = eng.to_host(call())
        eng.sync()
    finally:
        eng.set_parity_level("B")
    return out


# ---- 1. small polynomials straight into NTT form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [S.TERNARY, S.CBD])
@pytest.mark.parametrize("logn,moduli,batch", [(3, RC.TABLE, 3), (5, RC.HEAVY, 3), (5, RC.TABLE[:1], 1), (11, RC.TABLE, 1), (11, RC.HEAVY[1:2], 3)])
def test_sample_small_ntt(eng, orc, kind, logn, moduli, batch):
    stream = 60 + logn
    sampler = eng.sample_ternary if kind == S.TERNARY else eng.sample_cbd
    for scale in RC.SMALL_SCALES:   # (the largest: 21 * scale >= q for every modulus, the rule's division path)
        got = eng.to_host(eng.sample_small_ntt(logn, moduli, kind, K.SEED, stream, batch, scale))
        assert got.shape == (batch, len(moduli), 1 << logn) and below(got, moduli)
        composed = eng.to_host(eng.poly_from_signed(moduli, sampler(logn, K.SEED, stream, batch) * scale))
        assert np.array_equal(got, strict(orc, moduli, composed)), scale
        assert np.array_equal(got, R.small_ntt(orc, logn, moduli, kind, K.SEED, stream, scale, batch)), scale
        assert np.array_equal(got, at_level_a(eng, lambda: eng.sample_small_ntt(logn, moduli, kind, K.SEED, stream, batch, scale))), scale


# ---- 2. secret-key encryption, the full form --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_encrypt_seeded_against_model_composition_and_level_a(eng, orc, name):
    logn, moduli, batch, scale, stream = RC.CASES[name]
    L, n = len(moduli), 1 << logn
    sk, pt = device_secret(eng, logn, moduli), device_plaintext(eng, name)
    got = eng.to_host(eng.rlwe_encrypt_seeded(moduli, sk, pt, K.SEED, stream, scale))
    assert got.shape == (batch, 2, L, n) and below(got, moduli)
    assert np.array_equal(eng.to_host(sk), RC.secret_ntt(orc, logn, moduli))
    assert np.array_equal(got, RC.model_ct(orc, name))
    # the calls that were there before: sample, sample, hehub's encrypt core (lazy words)
    a, e = eng.sample_uniform(logn, moduli, K.SEED, stream, batch), eng.sample_cbd(logn, K.SEED, stream, batch) * scale
    composed = eng.to_host(eng.rlwe_encrypt_core(moduli, e, a, pt, sk))
    assert np.array_equal(got, strict(orc, moduli, composed))
    assert np.array_equal(got, at_level_a(eng, lambda: eng.rlwe_encrypt_seeded(moduli, sk, pt, K.SEED, stream, scale)))


# ---- 3. the compressed form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_compressed_form_is_c0_and_the_uniform_sampler_restores_c1(eng, orc, name):
    logn, moduli, batch, scale, stream = RC.CASES[name]
    L, n = len(moduli), 1 << logn
    words = batch * L * n
    sk, pt = device_secret(eng, logn, moduli), device_plaintext(eng, name)
    full = RC.model_ct(orc, name)
    buf = eng.empty((words + 64,)).fill_(FILL)
    eng.rlwe_encrypt_seeded(moduli, sk, pt, K.SEED, stream, scale, with_c1=False, out=buf)
    got = eng.to_host(buf)
    assert np.array_equal(got[:words].reshape(batch, L, n), full[:, 0])
    assert bool((got[words:] == FILL).all())
    assert np.array_equal(got[:words], at_level_a(eng, lambda: eng.rlwe_encrypt_seeded(moduli, sk, pt, K.SEED, stream, scale, with_c1=False)).reshape(-1))
    # c0 plus (seed, stream) is the ciphertext: the existing uniform sampler writes the c1 rows
    ct = eng.empty((batch, 2, L, n)).fill_(FILL)
    ct[:, 0] = buf[:words].view(batch, L, n)
    eng.sample_uniform(logn, moduli, K.SEED, stream, batch, out=ct.view(-1)[L * n:], stride_words=2 * L * n)
    assert np.array_equal(eng.to_host(ct), full)


# ---- 4. the zero plaintext; workspace -----------------------------------------------------------------------------------------------------
def test_null_plaintext_is_the_zero_plaintext_and_needs_no_workspace():
    from hehub_amd.engine import Engine

    logn, moduli, batch, scale, stream = 11, RC.TABLE, 3, 65537, 3300
    L, n = len(moduli), 1 << logn
    e = Engine(0)
    try:
        sk = device_secret(e, logn, moduli)
        e.sync()
        assert e.workspace_bytes() == 0
        outs = {}
        for c1 in (True, False):
            outs[c1] = e.to_host(e.rlwe_encrypt_seeded(moduli, sk, None, K.SEED, stream, scale, with_c1=c1, batch=batch))
        pk_like = e.rlwe_encrypt_seeded(moduli, sk, None, K.SEED, stream, scale, batch=1)
        e.sync()
        assert e.workspace_bytes() == 0
        zero = e.empty((batch, L, n)).zero_()
        assert np.array_equal(outs[True], e.to_host(e.rlwe_encrypt_seeded(moduli, sk, zero, K.SEED, stream, scale)))
        e.sync()
        assert e.workspace_bytes() == 0                       # (NTT(pt) passes through the c1 rows)
        assert np.array_equal(outs[False], e.to_host(e.rlwe_encrypt_seeded(moduli, sk, zero, K.SEED, stream, scale, with_c1=False)))
        e.sync()
        assert 0 < e.workspace_bytes() <= batch * L * n * 8 + 256
        assert np.array_equal(outs[False], outs[True][:, 0]) and np.array_equal(e.to_host(pk_like)[0], outs[True][0])
        # the public-key call: u, and pt where there is one
        e.release_workspace()
        e.rlwe_encrypt_pk_seeded(moduli, pk_like[0], None, K.SEED, stream, scale, batch=batch)
        e.sync()
        assert 0 < e.workspace_bytes() <= batch * L * n * 8 + 256
        e.rlwe_encrypt_pk_seeded(moduli, pk_like[0], zero, K.SEED, stream, scale)
        e.sync()
        assert e.workspace_bytes() <= 2 * (batch * L * n * 8 + 256)
    finally:
        e.close()


# ---- 5. exact decryption --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_decryption_returns_exactly_the_drawn_error(eng, name):
    logn, moduli, batch, scale, stream = RC.CASES[name]
    sk, pt = device_secret(eng, logn, moduli), RC.plaintext(name)
    ct = eng.rlwe_encrypt_seeded(moduli, sk, device_plaintext(eng, name), K.SEED, stream, scale)
    dec = eng.to_host(eng.rlwe_decrypt_core(moduli, ct, sk))
    assert below(dec, moduli)
    for b in range(batch):
        e = S.cbd_row(logn, K.SEED, stream + b)
        for m, q in enumerate(moduli):
            diff = [(int(d) - int(p)) % q for d, p in zip(dec[b, m], pt[b, m])]
            assert diff == [scale * int(v) % q for v in e], (b, m)
            if 2 * 21 * scale < q:
                assert [R.centred(x, q) for x in diff] == [scale * int(v) for v in e], (b, m)


# ---- 6. public-key encryption -----------------------------------------------------------------------------------------------------------------
def device_pk(eng, name):
    logn, moduli, _, scale, _ = RC.CASES[name]
    return eng.rlwe_encrypt_seeded(moduli, device_secret(eng, logn, moduli), None, K.SEED2, RC.PK_STREAM, scale, batch=1)[0]


@pytest.mark.parametrize("name", NAMES)
def test_encrypt_pk_seeded_against_model_and_level_a(eng, orc, name):
    logn, moduli, batch, scale, stream = RC.CASES[name]
    pk, pt = device_pk(eng, name), device_plaintext(eng, name)
    assert np.array_equal(eng.to_host(pk), RC.model_pk(orc, name))
    got = eng.to_host(eng.rlwe_encrypt_pk_seeded(moduli, pk, pt, K.SEED, stream + RC.PK_ENC_OFFSET, scale))
    assert got.shape == (batch, 2, len(moduli), 1 << logn) and below(got, moduli)
    assert np.array_equal(got, RC.model_pk_ct(orc, name))
    assert np.array_equal(got, at_level_a(eng, lambda: eng.rlwe_encrypt_pk_seeded(moduli, pk, pt, K.SEED, stream + RC.PK_ENC_OFFSET, scale)))
    # no plaintext: the same call on zeros
    none = eng.to_host(eng.rlwe_encrypt_pk_seeded(moduli, pk, None, K.SEED, stream, scale, batch=batch))
    assert np.array_equal(none, eng.to_host(eng.rlwe_encrypt_pk_seeded(moduli, pk, eng.empty(tuple(pt.shape)).zero_(), K.SEED, stream, scale)))


@pytest.mark.parametrize("name", ["n2048_L3_B3_t", "n2048_L1_B1"])
def test_public_key_ciphertext_decrypts_within_the_worst_case(eng, name):
    """|u|, |s| <= 1 and |e| <= 21: N terms in each of the two products u e_pk and e1 s, plus e0 -- error_scale * 21 * (2 N + 1)"""
    logn, moduli, batch, scale, stream = RC.CASES[name]
    bound = scale * 21 * (2 * (1 << logn) + 1)
    assert all(2 * bound < q for q in moduli)
    sk, pt = device_secret(eng, logn, moduli), RC.plaintext(name)
    ct = eng.rlwe_encrypt_pk_seeded(moduli, device_pk(eng, name), device_plaintext(eng, name), K.SEED, stream + RC.PK_ENC_OFFSET, scale)
    dec = eng.to_host(eng.rlwe_decrypt_core(moduli, ct, sk))
    errs = []
    for b in range(batch):
        rows = [[R.centred(int(d) - int(p), q) for d, p in zip(dec[b, m], pt[b, m])] for m, q in enumerate(moduli)]
        assert all(r == rows[0] for r in rows)   # (one integer polynomial behind every limb)
        errs.append(max(abs(v) for v in rows[0]))
    print(name, "public-key decryption error", errs, "bound", bound)
    assert max(errs) <= bound and min(errs) > 0


# ---- 7. batch element b is element 0 of the call at its id -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n8_L3_B3", "n32_L1_B3", "n2048_L3_B3_t"])
def test_batch_element_b_is_the_call_at_its_own_id(eng, name):
    logn, moduli, batch, scale, stream = RC.CASES[name]
    sk, pt = device_secret(eng, logn, moduli), device_plaintext(eng, name)
    pk = device_pk(eng, name)
    ct = eng.to_host(eng.rlwe_encrypt_seeded(moduli, sk, pt, K.SEED, stream, scale))
    c0 = eng.to_host(eng.rlwe_encrypt_seeded(moduli, sk, pt, K.SEED, stream, scale, with_c1=False))
    pct = eng.to_host(eng.rlwe_encrypt_pk_seeded(moduli, pk, pt, K.SEED, stream, scale))
    small = eng.to_host(eng.sample_small_ntt(logn, moduli, S.CBD, K.SEED, stream, batch, scale))
    for b in range(batch):
        one = pt[b:b + 1].contiguous()
        assert np.array_equal(ct[b], eng.to_host(eng.rlwe_encrypt_seeded(moduli, sk, one, K.SEED, (stream + b) & S.M64, scale))[0]), b
        assert np.array_equal(c0[b], eng.to_host(eng.rlwe_encrypt_seeded(moduli, sk, one, K.SEED, (stream + b) & S.M64, scale, with_c1=False))[0]), b
        assert np.array_equal(pct[b], eng.to_host(eng.rlwe_encrypt_pk_seeded(moduli, pk, one, K.SEED, (stream + 2 * b) & S.M64, scale))[0]), b
        assert np.array_equal(small[b], eng.to_host(eng.sample_small_ntt(logn, moduli, S.CBD, K.SEED, (stream + b) & S.M64, 1, scale))[0]), b
    assert not np.array_equal(ct[0], ct[1]) and not np.array_equal(pct[0], pct[1])


# ---- 8. refusals before anything is enqueued -------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(eng):
    from hehub_amd import capi

    logn, moduli, batch = 5, RC.TABLE, 2
    L, n = len(moduli), 1 << logn
    marr = (capi.u64 * L)(*moduli)
    seed = (C.c_ubyte * 32)(*K.SEED)
    sk, pk, pt = eng.empty((L, n)).zero_(), eng.empty((2, L, n)).zero_(), eng.empty((batch, L, n)).zero_()
    cwords = batch * 2 * L * n
    big = eng.empty((3 * cwords,)).fill_(FILL)
    out = big.data_ptr() + 8 * cwords
    ptr = lambda t: t.data_ptr()
    lib, h, vp = eng.lib, eng.h, C.c_void_p

    def untouched():
        eng.sync()
        return bool((big == FILL).all())

    def small(**kw):
        v = dict(logn=logn, L=L, m=marr, batch=batch, kind=S.CBD, seed=seed, stream=1, scale=1, out=out)
        v.update(kw)
        return lib.hp_dev_sample_small_ntt(h, v["logn"], v["L"], v["m"], v["batch"], v["kind"], v["seed"], v["stream"], v["scale"], vp(v["out"]))

    def enc(**kw):
        v = dict(logn=logn, L=L, m=marr, batch=batch, sk=ptr(sk), pt=ptr(pt), seed=seed, stream=1, scale=1, c1=1, out=out)
        v.update(kw)
        return lib.hp_dev_rlwe_encrypt_seeded(h, v["logn"], v["L"], v["m"], v["batch"], vp(v["sk"]), vp(v["pt"]), v["seed"], v["stream"],
                                              v["scale"], v["c1"], vp(v["out"]))

    def pke(**kw):
        v = dict(logn=logn, L=L, m=marr, batch=batch, pk=ptr(pk), pt=ptr(pt), seed=seed, stream=1, scale=1, out=out)
        v.update(kw)
        return lib.hp_dev_rlwe_encrypt_pk_seeded(h, v["logn"], v["L"], v["m"], v["batch"], vp(v["pk"]), vp(v["pt"]), v["seed"], v["stream"],
                                                 v["scale"], vp(v["out"]))

    calls = (small, enc, pke)
    refused = []

    def refuse(rcs):
        for rc in rcs:
            assert rc == capi.HP_EINVAL and eng.lib.hp_last_error(h), rcs
            refused.append(rc)

    # the ring degree: below one block, above the engine's limit; the number of moduli; nothing to do
    for bad in (0, 2, 17):
        refuse([f(logn=bad) for f in calls])
    m33 = (capi.u64 * 33)(*([moduli[0]] * 33))
    refuse([f(L=0) for f in calls] + [f(L=33, m=m33) for f in calls] + [f(batch=0) for f in calls])
    # moduli no word can be drawn for
    for q in (0, 1, 1 << 63, (1 << 64) - 1):
        refuse([f(m=(capi.u64 * L)(moduli[0], q, moduli[2])) for f in calls])
    # pointers: NULL, misaligned; a NULL seed
    refuse([f(m=None) for f in calls] + [f(seed=None) for f in calls] + [f(out=None) for f in calls] + [f(out=out + 8) for f in calls])
    refuse([enc(sk=None), enc(sk=ptr(sk) + 8), enc(pt=ptr(pt) + 8), pke(pk=None), pke(pk=ptr(pk) + 8), pke(pt=ptr(pt) + 8)])
    # the scale: 21 * scale must fit an int64; the kind; with_c1
    for bad in (0, 1 << 58, (1 << 64) - 1):
        refuse([small(scale=bad), enc(scale=bad), pke(scale=bad)])
    refuse([small(kind=k) for k in (0, 1, 4, 1 << 16 | 2)] + [enc(c1=2), enc(c1=-1)])
    # the output overlapping an input: from either side, by one pair of words
    last_full, last_c0 = out + 8 * cwords - 16, out + 8 * (cwords // 2) - 16
    refuse([enc(sk=out - 8 * L * n + 16), enc(sk=last_full), enc(c1=0, sk=last_c0), enc(pt=out - 8 * batch * L * n + 16), enc(pt=last_full),
            pke(pk=out - 8 * 2 * L * n + 16), pke(pk=last_full), pke(pt=out - 8 * batch * L * n + 16), pke(pt=last_full)])
    assert len(refused) > 60 and untouched()
    # a chain the transform plan refuses is refused with its code (a prime without a 2N-th root of unity: 96 = 3 * 32), before anything is written
    rootless = (capi.u64 * L)(moduli[0], moduli[1], 97)
    x = eng.empty((L, n)).zero_()
    code = lib.hp_dev_ntt(h, logn, L, rootless, 1, vp(ptr(x)))
    assert code != capi.HP_OK and [f(m=rootless) for f in calls] == [code] * 3
    assert untouched()
    # what is allowed: the largest scale, adjacent buffers, no plaintext, the compressed form inside its half
    assert small(scale=(1 << 58) - 1) == capi.HP_OK and small(kind=S.TERNARY, logn=3) == capi.HP_OK
    assert enc(scale=(1 << 58) - 1, sk=out - 8 * L * n) == capi.HP_OK and enc(pt=None) == capi.HP_OK and pke(pt=None) == capi.HP_OK
    assert enc(c1=0, sk=out + 8 * (cwords // 2)) == capi.HP_OK
    eng.sync()
    assert bool((big[:cwords] == FILL).all()) and bool((big[2 * cwords:] == FILL).all())
