"""The whole bootstrap in the exact model (tests/bootstrap_model.py: model_mod_raise, hks_model.model_bsgs, polyeval_model.model_plan, the
checker's rescale) at N = 32, without a GPU: three seeds, each with a fresh secret of Hamming weight 8, fresh keys and a fresh one-limb
ciphertext of random slots.

  * the raised ciphertext decrypts to m + e + q_0 I with |I| <= (H + 1) / 2 < K -- the worst case for centred c_0, c_1 and H non-zero
    ternary coefficients, not a probability;
  * the bootstrapped ciphertext decrypts and decodes to the slots; the largest slot error over the seeds is the constant
    bootstrap_model.MODEL_SLOT_ERROR, and the device's end-to-end threshold is 4 x that (different keys and errors are drawn there);
  * 4 x the constant has to lie below 2^-10: the sine's linearisation alone costs a relative (2 pi Delta / q_0)^2 / 6, about 2^-17 at
    q_0 / Delta = 2^10; anything worse than 2^-10 means the degree, r, K or the diagonals' scale are wrong."""
import numpy as np

import bootstrap_model as bm
from hehub_amd.bootstrap import BootstrapPlan, decode, encode
from oracle.pyoracle import SplitMix


def slots(rng, n):
    v = rng.words(2 * n, 2001).astype(np.float64) / 1000 - 1
    return (v[:n] + 1j * v[n:]) / np.sqrt(2)


def test_model_bootstrap_refreshes_a_one_limb_ciphertext(orc):
    c = bm.SMALL
    N, n = 1 << c["logn"], 1 << (c["logn"] - 1)
    bp = BootstrapPlan(c["logn"], bm.small_chain(), c["k"], c["delta"], c["K"], factors=c["factors"], precision_bits=c["precision_bits"])
    assert (c["H"] + 1) / 2 < c["K"] and round(bp.q[0] / c["delta"]) == 1 << 10
    q0, worst = bp.q[0], 0.0
    for seed in bm.SEEDS:
        rng = SplitMix(seed)
        s = bm.sparse_secret(rng, N, c["H"])
        assert np.count_nonzero(s) == c["H"]
        keys, s_ntt = bm.model_keys(orc, rng, bp, c["alpha"], s)
        z = slots(rng, n)
        m = encode(z, c["delta"], N)
        ct = bm.encrypt_at_q0(orc, rng, q0, np.ascontiguousarray(s_ntt[:1]), m, N)
        raised = np.stack([bm.model_mod_raise(orc, c["logn"], bp.q, ct[h][0])[0] for h in range(2)])
        t = bm.decrypt(orc, bp.q, s_ntt, raised)
        I = [(int(tv) - int(mv) + q0 // 2) // q0 for tv, mv in zip(t, m)]
        assert all(abs(int(tv) - int(mv) - q0 * i) <= 8 for tv, mv, i in zip(t, m, I))        # m + e + q_0 I, |e| <= 8
        assert max(abs(i) for i in I) <= (c["H"] + 1) / 2 < c["K"]
        out = bm.model_bootstrap(orc, bp, c["alpha"], keys, ct)
        assert out.shape == (2, bp.out_limbs, N)
        got = decode([int(v) for v in bm.decrypt(orc, bp.q[:bp.out_limbs], s_ntt, out)], bp.out_scale, N)
        err = float(np.abs(got - z).max())
        print(f"seed {seed}: |I| <= {max(abs(i) for i in I)}, max slot error {err:.3e} = 2^{np.log2(err):.2f}")
        worst = max(worst, err)
    print(f"largest slot error {worst:.3e}; recorded {bm.MODEL_SLOT_ERROR:.3e}; device threshold {4 * bm.MODEL_SLOT_ERROR:.3e}")
    assert worst <= bm.MODEL_SLOT_ERROR
    assert 4 * bm.MODEL_SLOT_ERROR < bm.ERROR_CEILING
