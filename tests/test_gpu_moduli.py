"""The engine on moduli off the prime table (tests/moduli.py): the families of every width and the named chains, word for word
with the oracle at level B -- transforms (tiled, generic, split), the scheme pipelines with lazy input words, the knobs that change
the digit-row format, the hybrid key switch -- and parity level A on the chains it serves and the chains it must leave at level B.
The oracle's words on these moduli are pinned to the reference by tests/test_moduli_edges.py."""
import numpy as np
import pytest

import moduli as M
import params as P
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64
LOGNS = (1, 4, 10, 11, 12, 13, 14, 15, 16)
SCHEME_LOGNS = (3, 11, 13, 15)


def _engine(monkeypatch=None, **env):
    from hehub_amd.engine import Engine

    for k in ("HP_NO_PACK48", "HP_NO_FUSED_DROP", "HP_PACK48_MIN_LOGN", "HP_SPLIT_MAX_ITEMS"):
        if monkeypatch:
            monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return Engine(0)     # (the knobs are read here)


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.release_workspace()
    e.close()


def qcol(moduli):
    return np.array(moduli, dtype=U)[:, None]


# ---- transforms --------------------------------------------------------------------------------------------------------------

def _rows(logn, primes, B, seed):
    """[B, L, n]: every (polynomial, limb) row one of the edge input kinds"""
    n, rng = 1 << logn, SplitMix(seed)
    x = np.empty((B, len(primes), n), dtype=U)
    for b in range(B):
        for j, q in enumerate(primes):
            x[b, j] = M.edge_words(rng, M.INPUT_KINDS[(b + j) % len(M.INPUT_KINDS)], q, n)
    return x


def _check_device_transforms(e, orc, logn, primes, B, seed):
    x = _rows(logn, primes, B, seed)
    y = np.stack([[orc.ntt(logn, q, x[b, j]) for j, q in enumerate(primes)] for b in range(B)])
    d = e.to_device(x)
    e.ntt_(primes, d)
    assert np.array_equal(e.to_host(d), y), ("ntt", logn, primes)
    z = np.stack([[orc.intt(logn, q, y[b, j]) for j, q in enumerate(primes)] for b in range(B)])
    e.intt_(primes, d)
    assert np.array_equal(e.to_host(d), z), ("intt", logn, primes)
    zx = np.stack([[orc.intt(logn, q, x[b, j]) for j, q in enumerate(primes)] for b in range(B)])
    d = e.to_device(x)
    e.intt_(primes, d, strict=True)
    assert np.array_equal(e.to_host(d), zx % qcol(primes)), ("intt strict", logn, primes)


@pytest.mark.parametrize("logn", LOGNS)
def test_transforms_on_every_family(eng, orc, logn):
    primes = [q for q in M.ALL if M.max_logn(q) >= logn]
    n = 1 << logn
    for q in primes[:: max(1, len(primes) // 12)]:                    # the host entry points on a spread of them
        for kind in M.INPUT_KINDS:
            x = M.edge_words(SplitMix(q % 997 + logn), kind, q, n)
            y = eng.host_ntt(logn, q, x)
            assert np.array_equal(y, orc.ntt(logn, q, x)), (q, logn, kind)
            assert np.array_equal(eng.host_intt(logn, q, y), orc.intt(logn, q, y)), (q, logn, kind)
    for i in range(0, len(primes), 24):                                # many limbs per launch
        _check_device_transforms(eng, orc, logn, primes[i:i + 24], 1 if logn >= 15 else 2, 10 + i + logn)
    for q in primes[:: max(1, len(primes) // 6)]:                     # one limb (the split kernels' few-limb launches)
        _check_device_transforms(eng, orc, logn, [q], 2, q % 1009)


@pytest.mark.parametrize("logn", [11, 13, 15, 16])
def test_transforms_generic_and_split(monkeypatch, orc, logn):
    primes = [q for q in M.ALL if M.max_logn(q) >= logn][::3]
    eng = _engine()
    try:
        eng.force_generic(True)
        _check_device_transforms(eng, orc, logn, primes[:8], 1, 50 + logn)
    finally:
        eng.close()
    eng = _engine(monkeypatch, HP_SPLIT_MAX_ITEMS="4096")
    try:
        for sel in (primes[:2], primes[2:3], primes[3:10]):
            _check_device_transforms(eng, orc, logn, sel, 1, 60 + logn)
    finally:
        eng.close()


# ---- scheme pipelines at level B ------------------------------------------------------------------------------------------------

def _scheme_inputs(name, logn, B):
    mext = M.CHAINS[name]
    n, L = 1 << logn, len(mext) - 1
    rng = SplitMix(300 * sorted(M.CHAINS).index(name) + logn)
    ct1 = M.lazy_rows(rng, (B, 2, L, n), mext[:L])          # what a chained hehub call hands in: lazy words
    ct2 = rng.poly((B, 2, L, n), mext[:L])
    key = rng.poly((L, 2, L + 1, n), mext)
    return mext, ct1, ct2, key


_EXPECTED = {}


def _expected(orc, name, logn, B):
    """the oracle's words for every pipeline of _run_pipelines (cached: the knob test reuses them)"""
    k = (name, logn, B)
    if k not in _EXPECTED:
        mext, ct1, ct2, key = _scheme_inputs(name, logn, B)
        L, q = len(mext) - 1, mext[:-1]
        ex = lambda f: np.stack([f(i) for i in range(B)])
        quad = ex(lambda i: orc.mult_low_level(q, ct1[i], ct2[i]))
        ext = ex(lambda i: orc.ext_prod(mext, quad[i, 2], key))
        out = {"quad": quad, "ext": ext,
               "rescale_ext": ex(lambda i: orc.ckks_rescale(mext, ext[i])),
               "relin": ex(lambda i: orc.ckks_relinearize(mext, quad[i], key)),
               "bgv_relin": ex(lambda i: orc.bgv_relinearize(mext, quad[i], key)),
               "rot": ex(lambda i: orc.ckks_rotate(mext, ct1[i], key, 3 + i)),
               "conj": ex(lambda i: orc.ckks_conjugate(mext, ct2[i], key))}
        if L >= 2:
            out["rescale"] = ex(lambda i: orc.ckks_rescale(q, ct1[i]))
            for t in (65537, 2, 1):
                out[f"switch{t}"] = ex(lambda i: orc.bgv_mod_drop(q, t, ct1[i]))
            out["mult"] = ex(lambda i: orc.ckks_mult(mext, ct1[i], ct2[i], key))
            out["bgv_mult"] = ex(lambda i: orc.bgv_mult(mext, 65537, ct1[i], ct2[i], key))
        _EXPECTED[k] = out
    return _EXPECTED[k]


def _run_pipelines(e, name, logn, B):
    mext, ct1, ct2, key = _scheme_inputs(name, logn, B)
    L, q = len(mext) - 1, mext[:-1]
    d1, d2, dk = e.to_device(ct1), e.to_device(ct2), e.to_device(key)
    h = e.to_host
    quad = e.mult_low_level(q, d1, d2)
    got = {"quad": h(quad)}
    ext = e.ext_prod(mext, quad[:, 2].contiguous(), dk)
    got["ext"] = h(ext)
    got["rescale_ext"] = h(e.ckks_rescale(mext, ext))
    got["relin"] = h(e.ckks_relinearize(mext, quad, dk))
    got["bgv_relin"] = h(e.bgv_relinearize(mext, quad, dk))
    got["rot"] = h(e.ckks_rotate_many(mext, L, d1, [dk] * B, [3 + i for i in range(B)]))
    got["rot1"] = h(e.ckks_rotate(mext, d1[:1].contiguous(), dk, 3))
    got["conj"] = h(e.ckks_conjugate(mext, d2, dk))
    if L >= 2:
        got["rescale"] = h(e.ckks_rescale(q, d1))
        for t in (65537, 2, 1):
            got[f"switch{t}"] = h(e.bgv_mod_switch(q, t, d1))
        got["mult"] = h(e.ckks_mult(mext, d1, d2, dk))
        got["bgv_mult"] = h(e.bgv_mult(mext, 65537, d1, d2, dk))
        pairs = [(d1[b, 0], d1[b, 1], d2[b, 0], d2[b, 1]) for b in range(B)]
        got["mult_rows"] = h(e.ckks_mult_rows(mext, L, pairs, dk))
        got["bgv_mult_rows"] = h(e.bgv_mult_rows(mext, 65537, pairs, dk))
    return got


def _compare(got, exp, what):
    for k, v in got.items():
        want = {"rot1": lambda: exp["rot"][:1], "mult_rows": lambda: exp["mult"], "bgv_mult_rows": lambda: exp["bgv_mult"]}.get(k, lambda: exp[k])()
        assert np.array_equal(v, want), (what, k, np.argwhere(v != want)[:3].tolist())


SCHEME_CASES = [(name, logn) for name in sorted(M.CHAINS) for logn in SCHEME_LOGNS]


@pytest.mark.parametrize("name,logn", SCHEME_CASES)
def test_scheme_pipelines_at_level_b(eng, orc, name, logn):
    B = 2
    _compare(_run_pipelines(eng, name, logn, B), _expected(orc, name, logn, B), (name, logn))


@pytest.mark.parametrize("env", [{"HP_NO_PACK48": "1"}, {"HP_NO_FUSED_DROP": "1"}, {"HP_PACK48_MIN_LOGN": "11"}],
                         ids=lambda e: ",".join(f"{k[3:]}={v}" for k, v in e.items()))
@pytest.mark.parametrize("name", ["W59", "PACKEDGE", "LOWMID"])
def test_knobs_leave_the_words_alone(monkeypatch, orc, name, env):
    e = _engine(monkeypatch, **env)
    try:
        for logn in (11, 13):
            _compare(_run_pipelines(e, name, logn, 2), _expected(orc, name, logn, 2), (name, logn, env))
    finally:
        e.close()


# ---- hybrid key switch -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["W59", "ABOVE"])
def test_hybrid_key_switch(eng, orc, name):
    from hks_model import model_switch

    logn, L, k, alpha = 11, 3, 2, 2
    mext = M.CHAINS[name][:L] + M.CHAINS[name][-k:]
    n, q = 1 << logn, mext[:L]
    rng = SplitMix(1900 + L)
    nd = (L + alpha - 1) // alpha
    pt = np.stack([M.lazy_rows(rng, (L, n), q) % qcol(q) for _ in range(2)])
    key = rng.poly((nd, 2, L + k, n), mext)
    models = [model_switch(orc, logn, mext, L, k, alpha, pt[i], key) for i in range(2)]
    got = eng.to_host(eng.hks_switch(mext, k, alpha, eng.to_device(pt), eng.to_device(key)))
    for i in range(2):
        assert np.array_equal(got[i], models[i]), (name, i)
    if M.level_a_chain(mext, logn):
        eng.set_parity_level("A")
        try:
            got = eng.to_host(eng.hks_switch(mext, k, alpha, eng.to_device(pt), eng.to_device(key)))
            eng.sync()
        finally:
            eng.set_parity_level("B")
        qa = qcol(q)[None]
        for i in range(2):
            assert (got[i] < 2 * qa).all() and np.array_equal(got[i] % qa, models[i] % qa), (name, i)


# ---- parity level A ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def enga():
    e = _engine()
    e.set_parity_level("A")
    yield e
    e.release_workspace()
    e.close()


WIDE_EDGE = [M.FAMILIES[k]["below"] for k in (44, 46, 48)] + [M.FAMILIES[k]["above"] for k in (45, 47, 49)]
LEVEL_A_CHAINS = {"ABOVE": M.ABOVE, "PACK40EDGE": M.PACK40EDGE, "WIDE_EDGE": WIDE_EDGE}


@pytest.mark.parametrize("logn", [11, 13])
@pytest.mark.parametrize("name", sorted(LEVEL_A_CHAINS))
def test_level_a_residues_on_eligible_chains(enga, orc, name, logn):
    """as test_gpu_level_a.test_scheme_level_residues: canonical residues of the oracle's words"""
    mext = LEVEL_A_CHAINS[name]
    assert M.level_a_chain(mext, logn)
    e, B = enga, 2
    n, L = 1 << logn, len(mext) - 1
    q = mext[:L]
    rng = SplitMix(2100 + logn)
    ct1, ct2 = M.lazy_rows(rng, (B, 2, L, n), q), rng.poly((B, 2, L, n), q)
    key = rng.poly((L, 2, L + 1, n), mext)
    d1, d2, dk = e.to_device(ct1), e.to_device(ct2), e.to_device(key)
    ex = lambda f: np.stack([f(i) for i in range(B)])
    canon = lambda mods, a: a % np.array(mods[:a.shape[-2]], dtype=U)[:, None]
    quad = e.mult_low_level(q, d1, d2)
    quad_h = e.to_host(quad)
    assert np.array_equal(quad_h, ex(lambda i: orc.mult_low_level(q, ct1[i], ct2[i])))
    ext = e.to_host(e.ext_prod(mext, quad[:, 2].contiguous(), dk))
    assert np.array_equal(canon(mext, ext), canon(mext, ex(lambda i: orc.ext_prod(mext, quad_h[i, 2], key))))
    assert (ext < 2 * qcol(mext)).all()
    checks = [
        (e.ckks_rescale(q, d1), ex(lambda i: orc.ckks_rescale(q, ct1[i]))),
        (e.bgv_mod_switch(q, 65537, d1), ex(lambda i: orc.bgv_mod_drop(q, 65537, ct1[i]))),
        (e.ckks_relinearize(mext, quad, dk), ex(lambda i: orc.ckks_relinearize(mext, quad_h[i], key))),
        (e.ckks_rotate(mext, d1, dk, 3), ex(lambda i: orc.ckks_rotate(mext, ct1[i], key, 3))),
        (e.ckks_mult(mext, d1, d2, dk), ex(lambda i: orc.ckks_mult(mext, ct1[i], ct2[i], key))),
        (e.bgv_mult(mext, 65537, d1, d2, dk), ex(lambda i: orc.bgv_mult(mext, 65537, ct1[i], ct2[i], key))),
    ]
    for got, want in checks:
        got = e.to_host(got)
        assert (want < 2 * qcol(q[:want.shape[-2]])).all()          # hehub's own words are lazy: residues are reduce_strict of them
        assert np.array_equal(got, canon(q, want))
    e.sync()                                                          # the range guard stays quiet


@pytest.mark.parametrize("logn", [12, 13])
@pytest.mark.parametrize("name", ["LOWMID", "OVER50", "HIGHMID"])
def test_ineligible_chains_run_at_level_b(enga, orc, name, logn):
    """a chain with a limb hehub's fold is not exact on (or one >= 2^50) keeps level B: the oracle's raw words, wrapped ones included"""
    mext = M.CHAINS[name]
    assert not M.level_a_chain(mext, logn)
    _compare(_run_pipelines(enga, name, logn, 2), _expected(orc, name, logn, 2), (name, logn, "A"))
    enga.sync()


def test_residue_transforms_refuse_moduli_hehub_folds_inexactly(enga, orc):
    from hehub_amd.engine import HpError

    logn, n = 12, 1 << 12
    for q in (M.LOWMID_Q, M.HIGHMID[0], M.OVER50[-1]):
        assert not M.level_a_chain([q], logn)
        x = enga.to_device(M.edge_words(SplitMix(5), "lazy", q, n).reshape(1, 1, n))
        for f in (enga.ntt_residues_, enga.intt_residues_):
            with pytest.raises(HpError):
                f([q], x)
    for q in M.ABOVE:
        x = M.edge_words(SplitMix(6), "max", q, n)
        d = enga.to_device(x.reshape(1, 1, n))
        enga.ntt_residues_([q], d)
        assert np.array_equal(enga.to_host(d)[0, 0], orc.ntt(logn, q, x) % U(q))
    enga.sync()


def test_high_mid_words_from_hehub_are_accepted(enga, orc):
    """Decision pinned: level A does not serve moduli whose hehub words reach 2q (high_mid).  Such a chain keeps level B, so the words
    hehub's own transform produced -- some at or above 2q -- go into a level-A context without tripping the range guard."""
    mext, logn = M.HIGHMID, 12
    n, L = 1 << logn, len(mext) - 1
    q = mext[:L]
    rng = SplitMix(77)
    coef = rng.poly((2, 2, L, n), q)
    ct = np.stack([[[orc.ntt(logn, q[j], coef[b, h, j]) for j in range(L)] for h in range(2)] for b in range(2)])
    assert (ct >= 2 * qcol(q)).any()
    key = rng.poly((L, 2, L + 1, n), mext)
    got = enga.to_host(enga.ckks_mult(mext, enga.to_device(ct), enga.to_device(ct[::-1].copy()), enga.to_device(key)))
    for b in range(2):
        assert np.array_equal(got[b], orc.ckks_mult(mext, ct[b], ct[1 - b], key))
    enga.sync()


# ---- the exact reference on the GPU ------------------------------------------------------------------------------------------

EXACT_GPU = [q for q in [65537] + [M.FAMILIES[k][p] for k in (30, 40, 45, 50, 55) for p in ("below", "above")]]


@pytest.mark.parametrize("logn", [11, 12, 13, 14, 15])
def test_exact_product_on_the_gpu(eng, enga, logn):
    n = 1 << logn
    for q in EXACT_GPU:
        if logn > M.max_logn(q) or not M.hehub_fold_exact(q, q, logn):
            continue
        rng = SplitMix(q % 4099 + logn)
        a, b = M.edge_words(rng, "lazy", q, n), M.edge_words(rng, "strict", q, n)
        want = M.negacyclic_product(a, b, q)
        da, db = eng.to_device(a.reshape(1, 1, n)), eng.to_device(b.reshape(1, 1, n))
        eng.ntt_([q], da); eng.ntt_([q], db)
        c = eng.poly_mul([q], da, db)
        eng.intt_([q], c, strict=True)
        assert np.array_equal(eng.to_host(c)[0, 0], want), (q, logn)
        if M.level_a_chain([q], logn):
            da, db = enga.to_device(a.reshape(1, 1, n)), enga.to_device(b.reshape(1, 1, n))
            enga.ntt_residues_([q], da); enga.ntt_residues_([q], db)
            c = enga.poly_mul([q], da, db)
            enga.intt_residues_([q], c)
            assert np.array_equal(enga.to_host(c)[0, 0], want), (q, logn, "residues")
    enga.sync()
