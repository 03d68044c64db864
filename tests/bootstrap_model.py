"""Exact models of the bootstrapping calls (tests only): ModRaise as integers, and the whole bootstrap composed of the models of its calls.

model_mod_raise is the contract of hp_dev_ckks_mod_raise (include/hehub_amd.h) written out: the strict inverse transform of limb
row 0 modulo q_0, the centring rule of k_base_from_single and of the drop prologue -- half = q_0 // 2 in integers, a coefficient
c >= half is the negative c - q_0 -- and the forward transform of the centred integers modulo every q_m.  The transforms are the
checker's (exact words of hehub's, reduced here), everything between them is Python integers."""
import numpy as np

U = np.uint64


def centre(c, q0):
    """strict coefficients modulo q0 -> the signed integers of the centring rule (Python integers)"""
    half = q0 // 2
    return [int(x) if int(x) < half else int(x) - q0 for x in c]


def model_mod_raise(orc, logn, moduli, row0):
    """row0: u64[N] NTT-form words modulo q_0 = moduli[0] (any representative) -> (u64[L][N] canonical residues of the raised
    polynomial, the centred coefficients as Python integers)"""
    q0 = int(moduli[0])
    words = (np.asarray(row0, dtype=U) % U(q0)).astype(U)
    c = orc.intt(logn, q0, words) % U(q0)
    v = centre(c, q0)
    rows = [words]
    for q in moduli[1:]:
        q = int(q)
        rows.append(orc.ntt(logn, q, np.array([x % q for x in v], dtype=U)) % U(q))
    return np.stack(rows), v


def planted_coefficients(rng, n, q0):
    """strict coefficients modulo q0: uniform ones with the values at which the centring changes sides planted among them --
    0, 1, half - 1, half, half + 1, q0 - 1 -- from the first position on and again, in reverse, at the end of the row"""
    half = q0 // 2
    vals = [0, 1, half - 1, half, half + 1, q0 - 1]
    c = rng.words(n, q0)
    assert n >= 8
    c[:6] = np.array(vals, dtype=U)
    if n >= 16:
        c[n - 6:] = np.array(vals[::-1], dtype=U)
    return c


# ---- the whole bootstrap, composed of the models every call is already held to -------------------------------------------------------
def model_conjugate(orc, logn, mext, L, k, alpha, ct, key):
    """hp_dev_ckks_conjugate_hks on one ciphertext (tests/test_hks.py holds the device to exactly this)"""
    from hks_model import model_switch

    moved = np.stack([orc.poly_involution(np.ascontiguousarray(ct[h])) for h in range(2)])
    sw = model_switch(orc, logn, mext, L, k, alpha, moved[1], key)
    return np.stack([orc.poly_add(mext[:L], sw[0], moved[0]), sw[1]])


def encode_diagonal(orc, mext, poly):
    """integer coefficients -> [E][N] canonical NTT words over the chain"""
    rows = np.stack([np.array([int(c) % q for c in poly], dtype=U) for q in mext])
    return orc.poly_reduce_strict(mext, orc.poly_ntt(mext, rows))


def model_bootstrap(orc, bp, alpha, keys, ct, trace=None):
    """bp: a hehub_amd.bootstrap.BootstrapPlan; keys: {"rot": {step: key [nd][2][E][n]}, "conj": key, "relin": key} for the top chain;
    ct [2][in][N] (row 0 is read) -> [2][bp.out_limbs][N].  hks_model.model_bsgs, polyeval_model.model_plan, the oracle's rescale.
    trace: a dict that receives every intermediate ciphertext (batch) under the names of BootstrapPlan.run's trace"""
    from hks_levels import sub_diag, sub_key
    from hks_model import model_bsgs
    from polyeval_model import model_lincomb, model_plan

    logn, k, L0, n = bp.logn, bp.k, bp.key_L0, bp.n
    note = (lambda name, cts: trace.__setitem__(name, np.stack(cts))) if trace is not None else (lambda name, cts: None)
    diags = {}

    def diag_rows(call):
        if id(call) not in diags:
            diags[id(call)] = [[None if p is None else encode_diagonal(orc, bp.mext, p) for p in row] for row in call.polys]
        return diags[id(call)]

    def bsgs(level, call, x):
        mext = bp.level_chain(level)
        sub = lambda r: None if r % n == 0 else sub_key(keys["rot"][(-r) % n], L0, level, k, alpha)
        sp = call.split
        out = model_bsgs(orc, logn, mext, level, k, alpha, x, [sub(r) for r in sp.babies], [(-r) % n for r in sp.babies],
                         [False] * len(sp.babies), [sub(r) for r in sp.giants], [(-r) % n for r in sp.giants], [False] * len(sp.giants),
                         [[sub_diag(d, L0, level, k) for d in row] for row in diag_rows(call)])
        return np.ascontiguousarray(out.astype(U))

    rescale = lambda level, x: orc.ckks_rescale(bp.q[:level], np.ascontiguousarray(x))
    raised = np.stack([model_mod_raise(orc, logn, bp.q, ct[h][0])[0] for h in range(2)])
    xs = [raised]
    note("raise", xs)
    for j, st in enumerate(bp.stages):
        xs = [bsgs(st.level, call, x) for call in st.calls for x in xs]
        note(f"cts{j}", xs)
        xs = [rescale(st.level, x) for x in xs]
        note(f"cts{j}_rescaled", xs)
    lvl = bp.evalmod_level
    mext = bp.level_chain(lvl)
    conj = [model_conjugate(orc, logn, mext, lvl, k, alpha, x, sub_key(keys["conj"], L0, lvl, k, alpha)) for x in xs]
    note("conj", conj)
    xs = [model_lincomb(bp.q[:lvl], [x, xb]).astype(U) for x, xb in zip(xs, conj)]
    note("real", xs)
    xs = [model_plan(orc, logn, bp.mext, L0, k, alpha, keys["relin"], bp.evalmod, np.ascontiguousarray(x)) for x in xs]
    note("evalmod", xs)
    for j, st in enumerate(bp.stages_out):
        if j == 0:
            outs = [bsgs(st.level, call, np.ascontiguousarray(xs[call.half])) for call in st.calls]
            xs = [model_lincomb(bp.q[:st.level], outs).astype(U)]
        else:
            xs = [bsgs(st.level, st.calls[0], np.ascontiguousarray(xs[0]))]
        note(f"stc{j}", xs)
        xs = [rescale(st.level, x) for x in xs]
        note(f"stc{j}_rescaled", xs)
    return xs[0]


# ---- the case the CPU model test measures and the device tests repeat ----------------------------------------------------------------
# N = 32, 16 slots; a secret of Hamming weight H: the raised ciphertext decrypts to m + q_0 I with |I| <= (H + 1) / 2 < K in the WORST
# case (|c_0 + c_1 s| <= (q_0 / 2)(1 + H) for centred c_0, c_1 and H non-zero ternary coefficients), not with some probability.
SMALL = dict(logn=5, L=15, k=3, alpha=3, H=8, K=5, factors=2, precision_bits=27, delta=1 << 30, bits=40, special_bits=50)
SEEDS = (9901, 9902, 9903)
# the largest slot error |decode(decrypt(bootstrap(ct))) - z| over SEEDS, measured in the model (tests/test_bootstrap_model.py prints
# it); the device's end-to-end threshold is 4 x this
MODEL_SLOT_ERROR = 6.4e-6          # measured 6.364e-06 = 2^-17.26 (seeds 9901 / 9902 / 9903: 4.66e-06, 4.24e-06, 6.36e-06)
# where 4 x that has to lie: the sine's linearisation alone costs a relative (2 pi Delta / q_0)^2 / 6, about 2^-17 at q_0 / Delta = 2^10
ERROR_CEILING = 2.0 ** -10


def small_chain(c=SMALL):
    import params as P

    q = P.ntt_primes(c["L"], c["logn"], c["bits"])
    return q + P.ntt_primes(c["k"], c["logn"], c["special_bits"])


def sparse_secret(rng, N, H):
    """a ternary secret with exactly H non-zero coefficients"""
    s = np.zeros(N, dtype=np.int64)
    pos = []
    while len(pos) < H:
        p = int(rng.words(1, N)[0])
        if p not in pos:
            pos.append(p)
    for p in pos:
        s[p] = 1 if int(rng.words(1, 2)[0]) else -1
    return s


def model_keys(orc, rng, bp, alpha, s):
    """hybrid keys of the top chain for everything bp needs: rotations, the conjugation, s^2"""
    from hks_model import centred, keygen, move

    mext, L0, k, logn = bp.mext, bp.key_L0, bp.k, bp.logn
    s_ntt = orc.poly_reduce_strict(mext, orc.poly_ntt(mext, np.stack([(s % m).astype(U) for m in mext])))
    q_rows = np.ascontiguousarray(s_ntt[:L0])
    make = lambda s_from: keygen(orc, rng, logn, mext, L0, k, alpha, s, s_from)
    keys = {"rot": {}, "conj": None, "relin": make(centred(orc, bp.q, orc.poly_mul(bp.q, q_rows, q_rows)))}
    for step, cj in bp.rotations_needed:
        key = make(centred(orc, bp.q, move(orc, q_rows, step, cj)))
        if cj:
            keys["conj"] = key
        else:
            keys["rot"][step] = key
    return keys, s_ntt


def encrypt_at_q0(orc, rng, q0, s_ntt0, m, N):
    """a fresh one-limb ciphertext [2][1][N] of the integer polynomial m: c1 uniform, c0 = e - c1 s + m, e in [-8, 8]"""
    a = rng.poly((1, N), [q0])
    e = rng.words(N, 17).astype(np.int64) - 8
    pt = np.array([[(int(mi) + int(ei)) % q0 for mi, ei in zip(m, e)]], dtype=U)
    c0 = orc.poly_sub([q0], orc.poly_reduce_strict([q0], orc.poly_ntt([q0], pt)), orc.poly_mul([q0], a, s_ntt0))
    return np.stack([orc.poly_reduce_strict([q0], c0), a])


def decrypt(orc, q, s_ntt, ct):
    """the centred integer coefficients of c0 + c1 s over the moduli q"""
    from hks_model import centred

    s = np.ascontiguousarray(s_ntt[:len(q)])
    return centred(orc, q, orc.poly_add(q, np.ascontiguousarray(ct[0]), orc.poly_mul(q, np.ascontiguousarray(ct[1]), s)))
