"""The exact model of hp_dev_ckks_lincomb and hp_dev_ckks_eval_plan_hks: a linear form in Python integers, and a step as the pieces
every hybrid multiplication is already held to -- dot_model.model_tensor_sum + Z, hks_model.model_switch on the level's sub-key
(hks_levels.sub_key), the oracle's poly_add and ckks_rescale: dot_model.model_dot with Z added to (d0, d1).  The device and the model
hand each stage different representatives, so every comparison built on this is on strict residues plus "every word below 2q".
No test, no fixture; needs no GPU."""
import numpy as np

from dot_model import model_tensor_sum
from hks_levels import level_chain, sub_key
from hks_model import model_switch

U = np.uint64

# ---- the cases tests/test_polyeval_model.py measures in the model and tests/test_gpu_polyeval.py holds the device to ----------------
DELTA = 1 << 40
CHEB15 = [0.5, 0.61, -0.22, -0.17, 0.11, 0.05, -0.07, 0.02, 0.031, -0.012, 0.009, 0.004, -0.0051, 0.0022, -0.0013, 0.0007]
POWER7 = [0.02, 0.18, -0.06, 0.05, 0.04, -0.03, 0.01, -0.08]   # |p| < 1/2 on [-1, 1]: one 40-bit limb is left for Delta p(x)
E2E = dict(logn=11, L=7, key_L0=8, k=2, alpha=2, n1=4, xs=(0.73, -0.9, 0.001, -0.25))   # the end-to-end case, model and device
# max |dec - Delta p(x)| measured in the model (test_polyeval_model.py has the cases); every threshold is 8 x its measurement
POWER_MEASURED, POWER_THRESHOLD = 2, 16            # power (4, 2), N = 16
CHEB16_MEASURED, CHEB16_THRESHOLD = 5, 40          # Chebyshev degree 15 (4, 4), N = 16
E2E_MEASURED, E2E_THRESHOLD = 115, 920             # the same plan at the end-to-end case's own ring degree, N = 2048


def model_lincomb(q, cts, coefs=None, cst=None, start=None):
    """cts[j]: one ciphertext [2][L_j][n] (u64 words, L_j >= len(q)); coefs[j]: an integer or a list of len(q) residues (None: 1);
    cst: the same, added to polynomial 0 -> the canonical residues of start + sum_j coefs[j] cts[j] + cst, [2][L][n] (dtype object)"""
    L, n = len(q), cts[0].shape[-1] if cts else start.shape[-1]
    res = lambda c, m: 1 if c is None else int(c[m]) if hasattr(c, "__len__") else int(c)
    out = np.zeros((2, L, n), dtype=object) if start is None else start[:2, :L].astype(object)
    for j, ct in enumerate(cts):
        c = None if coefs is None else coefs[j]
        for m in range(L):
            out[:, m] += ct[:, m].astype(object) * res(c, m)
    for m in range(L):
        if cst is not None:
            out[0, m] += res(cst, m)
        out[:, m] %= q[m]
    return out


def model_form(q, form, elems):
    """a polyeval.Form over the elements computed so far -> [2][len(q)][n] canonical residues (dtype object), or None for an empty form"""
    if not form.terms and form.cst is None:
        return None
    n = elems[0].shape[-1]
    return model_lincomb(q, [elems[e] for e, _ in form.terms], [c for _, c in form.terms], form.cst,
                         start=np.zeros((2, len(q), n), dtype=object))


def model_step(orc, logn, mext_top, key_L0, k, alpha, key_top, level, xs, ys, z):
    """xs[t], ys[t]: [2][level][n] u64; z: [2][level][n] residues (dtype object) or None; key_top: the key of the top chain
    -> rescale(relin(sum_t xs[t] (x) ys[t]) + z), [2][level-1][n] words (compare on strict residues)"""
    mext = level_chain(mext_top, key_L0, level, k)
    q = mext[:level]
    if not xs:
        return orc.ckks_rescale(q, np.ascontiguousarray(z.astype(U)))
    quad = model_tensor_sum(q, xs, ys)
    if z is not None:
        quad[:2] += z
        for i, m in enumerate(q):
            quad[:2, i] %= m
    quad = quad.astype(U)
    sw = model_switch(orc, logn, mext, level, k, alpha, np.ascontiguousarray(quad[2]), sub_key(key_top, key_L0, level, k, alpha))
    lin = np.stack([orc.poly_add(q, sw[0], np.ascontiguousarray(quad[0])), orc.poly_add(q, sw[1], np.ascontiguousarray(quad[1]))])
    return orc.ckks_rescale(q, lin)


def model_plan(orc, logn, mext_top, key_L0, k, alpha, key_top, plan, ct):
    """a polyeval.Plan on one ciphertext ct [2][L][n] (L = plan.in_limbs <= key_L0) -> [2][plan.out_limbs][n] words"""
    elems = [ct]
    for s in plan.steps:
        q = mext_top[:s.level]
        forms = [[model_form(q, f, elems).astype(U) for f in xy] for xy in s.products]
        elems.append(model_step(orc, logn, mext_top, key_L0, k, alpha, key_top, s.level, [f[0] for f in forms], [f[1] for f in forms],
                                model_form(q, s.z, elems)))
    out = elems[-1]
    for d in range(plan.final_drops):
        out = orc.ckks_rescale(mext_top[:out.shape[1]], np.ascontiguousarray(out))
    return out


# ---- what the CPU model test and the device's end-to-end test share: constants as plaintexts, exact decryption ---------------------
def encrypt_constant(orc, rng, q, s_ntt, value, n):
    """a fresh ciphertext [2][L][n] of the constant polynomial `value` (its NTT form is the constant in every position): c1 uniform,
    c0 = e - c1 s + value, e with coefficients in [-8, 8]"""
    a = rng.poly((len(q), n), q)
    e = rng.words(n, 17).astype(np.int64) - 8
    e_ntt = orc.poly_reduce_strict(q, orc.poly_ntt(q, np.stack([(e % m).astype(U) for m in q])))
    m_rows = np.stack([np.full(n, value % m, dtype=U) for m in q])
    c0 = orc.poly_add(q, orc.poly_sub(q, e_ntt, orc.poly_mul(q, a, s_ntt)), m_rows)
    return np.stack([orc.poly_reduce_strict(q, c0), a])


def decrypt_error(orc, q, s_ntt, ct, expected):
    """max over the coefficients of |centred(c0 + c1 s) - (expected at coefficient 0, 0 elsewhere)|, exact integers"""
    from hks_model import centred

    L = len(q)
    s = np.ascontiguousarray(s_ntt[:L])
    dec = centred(orc, q, orc.poly_add(q, np.ascontiguousarray(ct[0]), orc.poly_mul(q, np.ascontiguousarray(ct[1]), s)))
    dec[0] -= expected
    return max(abs(int(v)) for v in dec)
