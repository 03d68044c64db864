"""hehub_amd/bootstrap.py on the device.

N = 32 (bootstrap_model.SMALL, the first seed of the CPU model test): BootstrapPlan.run on model-made keys and a model-made one-limb
ciphertext, EVERY call's output compared residue for residue with model_bootstrap's (tests/bootstrap_model.py) and held below 2q, then
the decoded result; once more at parity level A.  Where words are compared the device equals the model exactly.

N = 2048: three factors per side, ONE top-level key set made on the device by hp_dev_hks_keygen_rot_seeded (rotations and the
conjugation) and hp_dev_hks_keygen_seeded (s^2) and used through the _at calls at every level, two ciphertexts encrypted on the device
at one limb, bootstrap, decrypt, decode: every slot within 4 x bootstrap_model.MODEL_SLOT_ERROR (the margin covers other keys and
errors than the model drew), at both parity levels.  The secret has Hamming weight 8, so |I| <= 4.5 < K = 5 in the worst case."""
import numpy as np
import pytest

import bootstrap_model as bm
import params as P
from hehub_amd.bootstrap import BootstrapPlan, decode, encode
from hks_model import crt
from oracle.pyoracle import SplitMix

pytestmark = pytest.mark.gpu
U = np.uint64
THRESHOLD = 4 * bm.MODEL_SLOT_ERROR
SEED = bytes(range(32))
# 50-bit moduli and Delta = 2^40 (q_0 / Delta = 2^10 as in the small case): a diagonal is one rounding per coefficient at a scale of
# about one modulus, and at N = 2048 a slot of the first factor sums about sqrt(N) of those roundings times a dozen diagonals times
# inputs of magnitude sqrt(N) / 3 -- at 40-bit moduli that alone is 2^-28 on x = t / (K q_0), which EvalMod and SlotToCoeff
# multiply by K q_0 / Delta sqrt(N) = 2^18 (measured with 40-bit moduli: 1.4e-04).  The small case keeps 40 bits: N = 32 sums 8 times less.
BIG = dict(logn=11, L=19, k=5, alpha=4, H=8, K=5, factors=3, precision_bits=34, delta=1 << 40, bits=50, batch=2)


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def small(orc):
    """the plan, keys, ciphertext, slots and the model's trace of the N = 32 case: computed once, left unchanged"""
    c = bm.SMALL
    N, n = 1 << c["logn"], 1 << (c["logn"] - 1)
    bp = BootstrapPlan(c["logn"], bm.small_chain(), c["k"], c["delta"], c["K"], factors=c["factors"], precision_bits=c["precision_bits"])
    rng = SplitMix(bm.SEEDS[0])
    s = bm.sparse_secret(rng, N, c["H"])
    keys, s_ntt = bm.model_keys(orc, rng, bp, c["alpha"], s)
    v = rng.words(2 * n, 2001).astype(np.float64) / 1000 - 1
    z = (v[:n] + 1j * v[n:]) / np.sqrt(2)
    ct = bm.encrypt_at_q0(orc, rng, bp.q[0], np.ascontiguousarray(s_ntt[:1]), encode(z, c["delta"], N), N)
    trace = {}
    out = bm.model_bootstrap(orc, bp, c["alpha"], keys, ct, trace)
    return dict(bp=bp, keys=keys, s_ntt=s_ntt, z=z, ct=ct, trace=trace, out=out)


def device_keys(e, keys, alpha):
    return {"alpha": alpha, "rot": {s: e.to_device(k) for s, k in keys["rot"].items()}, "conj": e.to_device(keys["conj"]),
            "relin": e.to_device(keys["relin"])}


def test_every_call_equals_the_model(eng, orc, small):
    bp, c = small["bp"], bm.SMALL
    steps = []
    out = eng.to_host(bp.run(eng, eng.to_device(small["ct"][None].copy()), device_keys(eng, small["keys"], c["alpha"]), trace=steps))
    names = [name for name, _ in steps]
    assert names == list(small["trace"]) and names[0] == "raise" and "evalmod" in names and names[-1].startswith("stc")
    for name, t in steps:
        got, exp = eng.to_host(t), small["trace"][name]
        assert got.shape == exp.shape, name
        qv = np.array(bp.q[:got.shape[2]], dtype=U)[:, None]
        assert (got < U(2) * qv).all(), name
        assert np.array_equal(got % qv, exp % qv), name
    qv = np.array(bp.q[:bp.out_limbs], dtype=U)[:, None]
    assert out.shape == (1, 2, bp.out_limbs, bp.N) and np.array_equal(out[0] % qv, small["out"] % qv)
    got = decode([int(v) for v in bm.decrypt(orc, bp.q[:bp.out_limbs], small["s_ntt"], out[0])], bp.out_scale, bp.N)
    err = float(np.abs(got - small["z"]).max())
    print(f"N = 32 on the device: max slot error {err:.3e}, threshold {THRESHOLD:.3e}")
    assert err <= THRESHOLD


def test_the_whole_run_at_parity_level_a(orc, small):
    """(N = 32 has no level-A transforms: the calls that follow the context's level run level B's kernels, residues unchanged)"""
    from hehub_amd.engine import Engine

    bp = small["bp"]
    e = Engine(0)
    try:
        e.set_parity_level("A")
        out = e.to_host(bp.run(e, e.to_device(small["ct"][None].copy()), device_keys(e, small["keys"], bm.SMALL["alpha"])))
    finally:
        e.close()
    qv = np.array(bp.q[:bp.out_limbs], dtype=U)[:, None]
    assert (out < U(2) * qv).all() and np.array_equal(out[0] % qv, small["out"] % qv)


def test_end_to_end_with_device_keys_and_device_ciphertexts(eng):
    c = BIG
    logn, N, n, B, k, alpha = c["logn"], 1 << c["logn"], 1 << (c["logn"] - 1), c["batch"], c["k"], c["alpha"]
    chain = P.ntt_primes(c["L"] + k, logn, c["bits"])
    q, mext = chain[k:], chain[k:] + chain[:k]
    assert round(q[0] / c["delta"]) == 1 << 10
    bp = BootstrapPlan(logn, mext, k, c["delta"], c["K"], factors=c["factors"], precision_bits=c["precision_bits"])
    assert (c["H"] + 1) / 2 < c["K"] and all(len(st.calls[0].split.babies) + len(st.calls[0].split.giants) >= 4 for st in bp.all_stages)
    rng = SplitMix(9911)
    s = bm.sparse_secret(rng, N, c["H"])
    i64 = lambda a: eng.torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(f"cuda:{eng.device}")
    d_s = eng.poly_reduce_strict_(mext, eng.poly_from_signed(mext, i64(s[None])))                       # [1][E][N]
    rots = bp.rotations_needed
    d_rot = eng.hks_keygen_rot_seeded(mext, k, alpha, d_s[0], [st for st, _ in rots], SEED, 1000, 1, [cj for _, cj in rots])
    d_relin = eng.hks_keygen_seeded(mext, k, alpha, d_s[0], eng.poly_mul(mext, d_s, d_s), SEED, 5000, 1)
    keys = {"alpha": alpha, "rot": {st: d_rot[i] for i, (st, cj) in enumerate(rots) if not cj},
            "conj": d_rot[[cj for _, cj in rots].index(True)], "relin": d_relin[0]}
    v = rng.words(B * 2 * n, 2001).astype(np.float64).reshape(B, 2, n) / 1000 - 1
    z = (v[:, 0] + 1j * v[:, 1]) / np.sqrt(2)
    q0 = q[0]
    pt = np.array([[[m % q0 for m in encode(z[b], c["delta"], N)]] for b in range(B)], dtype=U)          # [B][1][N], coefficient form
    d_ct = eng.rlwe_encrypt_seeded([q0], d_s[0][:1].contiguous(), eng.to_device(pt), SEED, 7000, 1)
    assert tuple(d_ct.shape) == (B, 2, 1, N)
    diags = bp.upload(eng)
    sk = d_s[0][:bp.out_limbs].contiguous()
    qo = q[:bp.out_limbs]

    def slot_error(e):
        out = bp.run(e, d_ct, keys, diags)
        assert tuple(out.shape) == (B, 2, bp.out_limbs, N)
        coef = e.to_host(e.rlwe_decrypt_core(qo, out, sk))                                                 # [B][out][N], strict
        worst = 0.0
        for b in range(B):
            vals = []
            for i in range(N):
                x, Q = crt([coef[b, a, i] for a in range(len(qo))], qo)
                vals.append(x if x < Q // 2 else x - Q)
            worst = max(worst, float(np.abs(decode(vals, bp.out_scale, N) - z[b]).max()))
        return worst

    err = slot_error(eng)
    print(f"N = 2048, {bp.levels} levels ({c['factors']} factors per side, degree {bp.degree}, r = {bp.r}), {len(rots)} keys: "
          f"max slot error {err:.3e} = 2^{np.log2(err):.2f}, threshold {THRESHOLD:.3e}")
    assert err <= THRESHOLD
    eng.set_parity_level("A")
    try:
        err_a = slot_error(eng)
        eng.sync()
    finally:
        eng.set_parity_level("B")
    print(f"at parity level A: {err_a:.3e}")
    assert err_a <= THRESHOLD
