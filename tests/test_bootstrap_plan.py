"""hehub_amd/bootstrap.py without a GPU and without ciphertexts: the encoder, the slot rotation the engine's cycle(step) performs (pinned
against the checker's cycle through hks_model.move, not assumed), the special FFT's factors against the dense matrices, the baby-step
giant-step split, the float simulation of a whole plan, and the exact level and scale accounting."""
from fractions import Fraction

import numpy as np
import pytest

import params as P
from bootstrap_model import SMALL, small_chain
from hehub_amd import bootstrap as bs
from hks_model import move

U = np.uint64


def random_slots(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)) / np.sqrt(2)


@pytest.mark.parametrize("logn", [2, 5, 8])
def test_encoder_round_trip(logn):
    """one rounding per coefficient: the decoded slots are within N / 2 roundings of 1/2 each, over the scale"""
    N = 1 << logn
    z = random_slots(logn, N // 2)
    t = bs.encode(z, 1 << 30, N)
    assert len(t) == N and all(isinstance(v, int) for v in t)
    assert np.abs(bs.decode(t, 1 << 30, N) - z).max() <= N * 0.5 / (1 << 30)
    assert np.abs(bs.decode(bs.encode(z, Fraction(1 << 31, 2), N), 1 << 30, N) - z).max() <= N * 0.5 / (1 << 30)


@pytest.mark.parametrize("logn", [3, 5])
def test_rotation_convention_of_the_engine_cycle(orc, logn):
    """with slot j = t(zeta^(3^j)), cycle(step) on the NTT form is out[j] = in[j - step] for EVERY step and the involution is the
    conjugation; step_of(r) is the step of y[j] = x[j + r].  (With 5^j slots an odd step is a rotation composed with the conjugation.)"""
    N, n, q = 1 << logn, 1 << (logn - 1), P.ntt_primes(1, logn, 40)[0]
    z = random_slots(40 + logn, n)
    t = bs.encode(z, 1 << 24, N)
    rows = orc.poly_ntt([q], np.array([[v % q for v in t]], dtype=U))

    def slots_of(words):
        c = orc.poly_intt([q], np.ascontiguousarray(words))[0] % U(q)
        return bs.decode([int(v) if int(v) < q // 2 else int(v) - q for v in c], 1 << 24, N)

    base = slots_of(rows)
    for step in range(n):
        assert np.allclose(slots_of(move(orc, rows, step, False)), np.roll(base, step), atol=1e-9), step
    assert np.allclose(slots_of(move(orc, rows, 0, True)), np.conj(base), atol=1e-9)
    for r in (1, 2, n - 1):
        assert np.allclose(slots_of(move(orc, rows, bs.step_of(r, n), False)), np.roll(base, -r), atol=1e-9)
    assert bs.GEN == 3


@pytest.mark.parametrize("n,factors", [(n, f) for n in (4, 8, 16, 32, 64) for f in (1, 2, 3) if f <= n.bit_length() - 1])
def test_factored_products_against_the_dense_matrices(n, factors):
    """(n = 4 has two stages: no third factor)"""
    N = 2 * n
    E0 = bs._roots(N)[:, :n]
    R = np.eye(n)[bs.bit_reverse(n)]
    stages = n.bit_length() - 1
    per = [stages // factors + (1 if f < stages % factors else 0) for f in range(factors)]
    S = np.eye(n, dtype=np.complex128)
    for G, cnt in zip(bs.stc_factors(n, factors), per):
        assert 0 < len(G) <= 2 * (1 << cnt) - 1                       # at most 2 radix - 1 non-zero diagonals
        S = bs.dense(G, n) @ S
    assert np.abs(S @ R - E0).max() <= 1e-9
    C = np.eye(n, dtype=np.complex128)
    for G, cnt in zip(bs.cts_factors(n, factors), reversed(per)):
        assert 0 < len(G) <= 2 * (1 << cnt) - 1
        C = bs.dense(G, n) @ C
    assert np.abs(R @ C - E0.conj().T).max() <= 1e-9


@pytest.mark.parametrize("n", [4, 16, 64])
def test_coefficients_from_slots_and_back(n):
    """t_lo = Re(E0^H w) / n, t_hi = Re(E0^H (-i Sigma) w) / n, and w = E0 t_lo + i Sigma E0 t_hi: what CoeffToSlot and SlotToCoeff compute"""
    N = 2 * n
    F = bs._roots(N)
    E0, sg = F[:, :n], bs.sigma(n)
    t = np.random.default_rng(n).standard_normal(N)
    w = F @ t
    assert np.allclose(t[:n], (E0.conj().T @ w).real / n) and np.allclose(t[n:], (E0.conj().T @ (-1j * sg * w)).real / n)
    assert np.allclose(w, E0 @ t[:n] + 1j * sg * (E0 @ t[n:]))
    # Sigma commutes with every stage but S_2
    for s in range(1, n.bit_length() - 1):
        D = bs.dense(bs.stage(n, 2 << s), n)
        assert np.allclose(D * sg[None, :], sg[:, None] * D)


@pytest.mark.parametrize("n,factors", [(8, 1), (8, 2), (8, 3), (64, 1), (64, 2), (64, 3), (1024, 2), (1024, 3)])
def test_bsgs_split_recomposes_each_matrix(n, factors):
    """every split fits one call: at most 32 babies, 32 giants, 256 diagonals (hp_dev_ckks_lintrans_bsgs_hks's tables)"""
    x = random_slots(n + factors, n)
    for G in bs.stc_factors(n, factors) + bs.cts_factors(n, factors):
        sp = bs.bsgs_split(G, n)
        assert len(sp.babies) <= 32 and len(sp.giants) <= 32 and len(sp.babies) * len(sp.giants) <= 256
        assert 0 in sp.babies
        assert np.allclose(bs.bsgs_apply(sp, x), bs.mat_apply(G, x), atol=1e-9)
        seen = {}
        for g, row in zip(sp.giants, sp.diags):
            for i, d in zip(sp.babies, row):
                if d is not None:
                    seen[(g + i) % n] = np.roll(d, -g)                 # diag_{g,i} = rot_g^-1(diag_{g+i})
        assert set(seen) == set(G) and all(np.allclose(seen[r], G[r]) for r in G)


@pytest.fixture(scope="module")
def small_plan():
    c = SMALL
    return bs.BootstrapPlan(c["logn"], small_chain(), c["k"], c["delta"], c["K"], factors=c["factors"], precision_bits=c["precision_bits"])


def test_level_and_scale_accounting_is_exact(small_plan):
    bp, c = small_plan, SMALL
    assert bp.r >= 1                                                   # the double-angle steps are part of this plan
    assert bp.levels == 2 * c["factors"] + bs.chebyshev_levels(bp.degree) + bp.r
    assert bp.in_limbs == c["L"] and bp.out_limbs == c["L"] - bp.levels >= 1
    assert isinstance(bp.out_scale, Fraction) and bp.out_scale == c["delta"]
    assert bp.in_scale == c["K"] * bp.q[0]
    level, scale = bp.in_limbs, bp.in_scale
    for st in bp.stages:
        assert (st.level, st.in_scale) == (level, scale)
        assert st.out_scale == st.in_scale * st.diag_scale / bp.q[level - 1]         # exactly
        level, scale = level - 1, st.out_scale
    assert len(bp.stages[-1].calls) == 2 and all(len(st.calls) == 1 for st in bp.stages[:-1])
    assert (bp.evalmod.in_limbs, bp.evalmod.scales[0]) == (level, scale) and bp.evalmod_level == level
    assert len(bp.evalmod.steps) >= bp.r and bp.evalmod.final_drops == 0
    level, scale = bp.evalmod.out_limbs, bp.evalmod.out_scale
    for st in bp.stages_out:
        assert (st.level, st.in_scale) == (level, scale)
        assert st.out_scale == st.in_scale * st.diag_scale / bp.q[level - 1]
        level, scale = level - 1, st.out_scale
    assert [call.half for call in bp.stages_out[0].calls] == [0, 1]
    assert (level, scale) == (bp.out_limbs, bp.out_scale)
    rots = bp.rotations_needed
    assert rots[-1] == (0, True) and all(0 < s < bp.n and not cj for s, cj in rots[:-1]) and len(set(rots)) == len(rots)
    for st in bp.all_stages:
        for call in st.calls:
            for r in call.split.babies + call.split.giants:
                assert r % bp.n == 0 or (bs.step_of(r, bp.n), False) in rots
            bsteps, gsteps, b_id, g_id, polys = call.marshal(bp.n)
            assert bsteps == [bs.step_of(r, bp.n) for r in call.split.babies] and gsteps == [bs.step_of(r, bp.n) for r in call.split.giants]
            assert b_id == [s == 0 for s in bsteps] and g_id == [s == 0 for s in gsteps] and polys is call.polys
            assert len(polys) == len(gsteps) and all(len(row) == len(bsteps) for row in polys)
            for row in call.polys:
                assert all(p is None or (len(p) == bp.N and all(isinstance(v, int) for v in p)) for p in row)
    with pytest.raises(ValueError):
        bs.BootstrapPlan(c["logn"], small_chain()[:8] + small_chain()[-c["k"]:], c["k"], c["delta"], c["K"], factors=c["factors"])


def test_evaluate_plain_reproduces_the_slots(small_plan):
    """EvalMod's polynomial is within 2^-precision_bits of the sine; SlotToCoeff multiplies by q_0 / (2 pi Delta) and sums at most 2n
    coefficients per slot; the sine's cube is (2 pi max|m| / q_0)^2 / 6 of the result, |m| <= Delta sqrt(2) per coefficient at the most"""
    bp, c = small_plan, SMALL
    ratio = bp.q[0] / (2 * np.pi * c["delta"])
    bound = 2.0 ** -c["precision_bits"] * ratio * 2 * bp.n + (2 * np.pi * np.sqrt(2) * c["delta"] / bp.q[0]) ** 2 / 6 * 2 * bp.n
    z = random_slots(77, bp.n)
    rng = np.random.default_rng(78)
    for I in (None, rng.integers(-(c["K"] - 1), c["K"], bp.N)):
        err = np.abs(bp.evaluate_plain(z, I) - z).max()
        print(f"evaluate_plain: max slot error {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    assert bound < 2.0 ** -10


def test_evalmod_parameters_reach_the_precision():
    for K, bits in ((5, 20), (5, 27), (12, 24)):
        degree, r = bs.evalmod_parameters(K, bits)
        f = lambda x: np.cos(2 * np.pi * (K * x - 0.25) / (1 << r))
        xs = np.linspace(-1, 1, 3001)
        e = bs.cheb_eval(bs.cheb_coefficients(f, degree), xs)
        for _ in range(r):
            e = 2 * e * e - 1
        assert np.abs(e - np.sin(2 * np.pi * K * xs)).max() < 2.0 ** -bits
