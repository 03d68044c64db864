"""The exact integer model of the hybrid key switch and of the calls built on it -- the plain switch, hoisted rotations, the diagonal
transform and its baby-step giant-step form -- with what the tests around it share: key generation, decryption errors, rotation
lists, random diagonals and the three cases in which two entry points must agree.

Python integers for the ModUp / ModDown compositions and the sums, the oracle's own transform / Montgomery primitives for everything
hehub also does (so lazy representations agree).  No test, no fixture: tests/test_hks.py, tests/test_gpu_hks_*.py and
tests/hks_edges.py import from here, and the model itself needs no GPU (tests/test_hks_edges.py holds it to plain arithmetic)."""
import numpy as np

import params as P
from oracle.pyoracle import SplitMix

U = np.uint64
M64 = (1 << 64) - 1


# ---- one switch (hp_dev_hks_switch) ------------------------------------------------------------------------------------------------
def crt(residues, moduli):
    Q = 1
    for q in moduli:
        Q *= q
    x = 0
    for r, q in zip(residues, moduli):
        M = Q // q
        x += int(r) * M * pow(M, -1, q)
    return x % Q, Q


def below_2q(rows, moduli):
    """lazy transform words [L][n] brought below 2q the way the ModDown kernels do it (hp_lazy_below_2q, hp_device.h): minus 8q, 4q, 2q
    where that fits -- nothing where the word already is below 2q, which is everywhere but at moduli far below their power of two,
    where hehub's fold leaves words of up to 16q and hehub's lazy subtraction would wrap"""
    rows = rows.copy()
    for j, q in enumerate(moduli):
        for s in (8, 4, 2):
            rows[j] -= np.where(rows[j] >= U(s * q), U(s * q), U(0))
    return rows


def digits_of(L, alpha):
    return [list(range(d * alpha, min((d + 1) * alpha, L))) for d in range((L + alpha - 1) // alpha)]


def model_switch(orc, logn, mext, L, k, alpha, pt, key):
    """exact model of hp_dev_hks_switch for one polynomial: pt [L][n], key [nd][2][E][n] -> [2][L][n]"""
    n, E = 1 << logn, L + k
    digs = digits_of(L, alpha)
    coef = orc.poly_reduce_strict(mext[:L], orc.poly_intt(mext[:L], pt))
    D = np.zeros((len(digs), E, n), dtype=U)
    for d, limbs in enumerate(digs):
        ints = [crt([coef[a][i] for a in limbs], [mext[a] for a in limbs])[0] for i in range(n)]
        for m in range(E):
            if m in limbs:
                D[d, m] = pt[m]
            else:
                lifted = np.array([x % mext[m] for x in ints], dtype=U)
                D[d, m] = orc.ntt(logn, mext[m], lifted)
    ks = np.zeros((2, E, n), dtype=U)
    for h in range(2):
        for m in range(E):
            acc = [sum(int(D[d, m, i]) * int(key[d, h, m, i]) for d in range(len(digs))) for i in range(n)]
            pairs = np.array([[a & (2**64 - 1), a >> 64] for a in acc], dtype=U)
            ks[h, m] = orc.montgomery_128_lazy(mext[m], pairs)
    pm = mext[L:]
    out = np.zeros((2, L, n), dtype=U)
    for h in range(2):
        yp = orc.poly_reduce_strict(pm, orc.poly_intt(pm, np.ascontiguousarray(ks[h, L:])))
        Ys = [crt([yp[j][i] for j in range(k)], pm) for i in range(n)]
        rem = np.zeros((L, n), dtype=U)
        for i_q in range(L):
            q = mext[i_q]
            vals = [(y % q) if y < Pm // 2 else q - ((Pm - y) % q) for (y, Pm) in Ys]
            rem[i_q] = orc.ntt(logn, q, np.array(vals, dtype=U))
        diff = orc.poly_sub(mext[:L], np.ascontiguousarray(ks[h, :L]), below_2q(rem, mext[:L]))
        Pprod = 1
        for p in pm:
            Pprod *= p
        out[h] = orc.poly_rns_scalar_mul(mext[:L], diff, [pow(Pprod % q, -1, q) for q in mext[:L]])
    return out


def keygen(orc, rng, logn, mext, L, k, alpha, s_to, s_from, sigma_bound=8):
    """hybrid key u64[nd][2][E][n]: row d = RLWE encryption under s_to of (P mod q_i) * s_from on the limbs of digit d."""
    n, E = 1 << logn, L + k
    digs = digits_of(L, alpha)
    Pprod = 1
    for p in mext[L:]:
        Pprod *= p
    key = np.zeros((len(digs), 2, E, n), dtype=U)
    to_ntt = orc.poly_reduce_strict(mext, orc.poly_ntt(mext, np.stack([(s_to % q).astype(U) for q in mext])))
    from_ntt = orc.poly_reduce_strict(mext, orc.poly_ntt(mext, np.stack([(s_from % q).astype(U) for q in mext])))
    for d, limbs in enumerate(digs):
        a = rng.poly((E, n), mext)                                  # uniform, NTT form
        e = (rng.words(n, 2 * sigma_bound + 1).astype(np.int64) - sigma_bound)
        e_ntt = orc.poly_reduce_strict(mext, orc.poly_ntt(mext, np.stack([(e % q).astype(U) for q in mext])))
        b = orc.poly_sub(mext, e_ntt, orc.poly_mul(mext, a, to_ntt))          # e - a*s
        msg = np.zeros((E, n), dtype=U)
        for m in limbs:
            msg[m] = orc.poly_rns_scalar_mul([mext[m]], from_ntt[m][None], [Pprod % mext[m]])[0]
        b = orc.poly_reduce_strict(mext, orc.poly_add(mext, b, msg))
        mont = [(1 << 64) % q for q in mext]                        # Montgomery form, as hehub stores its keys
        key[d, 0] = orc.poly_reduce_strict(mext, orc.poly_rns_scalar_mul(mext, b, mont))
        key[d, 1] = orc.poly_reduce_strict(mext, orc.poly_rns_scalar_mul(mext, a, mont))
    return key


def centred_error(orc, logn, moduli, poly_ntt):
    """max |coefficient| of an NTT-form RNS polynomial, read as a centred integer"""
    c = orc.poly_reduce_strict(moduli, orc.poly_intt(moduli, poly_ntt))
    worst = 0
    for i in range(c.shape[1]):
        x, Q = crt([c[a][i] for a in range(len(moduli))], moduli)
        worst = max(worst, min(x, Q - x))
    return worst


# ---- model_switch in two halves, and the hoisted rotations (hp_dev_ckks_rotate_hoisted_hks) --------------------------------------------
def model_digits(orc, logn, mext, L, k, alpha, pt):
    """D [nd][E][n]: the digit rows the digit stage (HksCall::digits) builds from pt [L][n] -- pt's own words inside the digit, NTT of
    the exact ModUp value (the non-negative integer behind the digit's strict residues) elsewhere"""
    n, E = 1 << logn, L + k
    digs = digits_of(L, alpha)
    coef = orc.poly_reduce_strict(mext[:L], orc.poly_intt(mext[:L], pt))
    D = np.zeros((len(digs), E, n), dtype=U)
    for d, limbs in enumerate(digs):
        ints = [crt([coef[a][i] for a in limbs], [mext[a] for a in limbs])[0] for i in range(n)]
        for m in range(E):
            if m in limbs:
                D[d, m] = pt[m]
            else:
                D[d, m] = orc.ntt(logn, mext[m], np.array([x % mext[m] for x in ints], dtype=U))
    return D


def model_rest(orc, logn, mext, L, k, D, key):
    """inner product (summed in digit order, one Montgomery reduction), ModDown, * P^-1: D [nd][E][n], key [nd][2][E][n] -> [2][L][n]"""
    n, E = 1 << logn, L + k
    Do, Ko = D.astype(object), key.astype(object)
    ks = np.zeros((2, E, n), dtype=U)
    for h in range(2):
        for m in range(E):
            acc = sum(Do[d, m] * Ko[d, h, m] for d in range(D.shape[0]))
            pairs = np.array([[a & M64, (a >> 64) & M64] for a in acc], dtype=U)
            ks[h, m] = orc.montgomery_128_lazy(mext[m], pairs)
    pm = mext[L:]
    Pprod = 1
    for p in pm:
        Pprod *= p
    out = np.zeros((2, L, n), dtype=U)
    for h in range(2):
        yp = orc.poly_reduce_strict(pm, orc.poly_intt(pm, np.ascontiguousarray(ks[h, L:])))
        ys = [crt([yp[j][i] for j in range(k)], pm)[0] for i in range(n)]
        rem = np.zeros((L, n), dtype=U)
        for i_q in range(L):
            q = mext[i_q]
            rem[i_q] = orc.ntt(logn, q, np.array([(y % q) if y < Pprod // 2 else q - ((Pprod - y) % q) for y in ys], dtype=U))
        diff = orc.poly_sub(mext[:L], np.ascontiguousarray(ks[h, :L]), below_2q(rem, mext[:L]))
        out[h] = orc.poly_rns_scalar_mul(mext[:L], diff, [pow(Pprod % q, -1, q) for q in mext[:L]])
    return out


def move(orc, a, step, conj):
    a = np.ascontiguousarray(a)
    return orc.poly_involution(a) if conj else orc.poly_cycle(a, step)


def model_hoisted(orc, logn, mext, L, k, alpha, ct, keys, steps, conj):
    """ct [2][L][n] -> [R][2][L][n]"""
    q = mext[:L]
    D = model_digits(orc, logn, mext, L, k, alpha, ct[1])
    out = []
    for key, step, cj in zip(keys, steps, conj):
        sw = model_rest(orc, logn, mext, L, k, np.stack([move(orc, D[d], step, cj) for d in range(D.shape[0])]), key)
        out.append(np.stack([orc.poly_add(q, sw[0], move(orc, ct[0], step, cj)), sw[1]]))
    return np.stack(out)


def chain(L, k):
    return P.P40[:L] + (P.P50 + P.P40[L:])[:k]


def rotations_of(logn, R):
    """R (step, conj) pairs.  The long list: step 0, a duplicate, N/2 + 1 (the same map as step 1), conjugations at two places"""
    n = 1 << logn
    steps = ([0, 1, 1, n // 2 + 1, 3, 2] + list(range(4, 4 + R)))[:R]
    if R == 2:
        steps = [3, 1]
    if R == 3:
        steps = [5, 1, 0]
    conj = [False] * R
    if R >= 3:
        conj[R - 1] = True
    if R >= 6:
        conj[4] = True
    return steps, conj


def step0_case(eng, logn, L, k, alpha, seed=5200, mext=None):
    mext = mext or P.P40[:L] + P.P50[:k]
    n = 1 << logn
    rng = SplitMix(seed + logn)
    ct = rng.poly((2, 2, L, n), mext[:L])
    key = rng.poly(((L + alpha - 1) // alpha, 2, L + k, n), mext)
    d_ct, d_key = eng.to_device(ct), eng.to_device(key)
    plain = eng.to_host(eng.ckks_rotate_hks(mext, k, alpha, d_ct, d_key, 0))
    hoisted = eng.to_host(eng.ckks_rotate_hoisted_hks(mext, k, alpha, d_ct, [d_key], [0]))
    return plain, hoisted[:, 0]


# ---- decryption --------------------------------------------------------------------------------------------------------------------
def centred(orc, moduli, poly_ntt):
    """the centred integer coefficients of an NTT-form RNS polynomial"""
    c = orc.poly_reduce_strict(moduli, orc.poly_intt(moduli, poly_ntt))
    vals = []
    for i in range(c.shape[1]):
        x, Q = crt([c[a][i] for a in range(len(moduli))], moduli)
        vals.append(x if x < Q // 2 else x - Q)
    return np.array(vals, dtype=object)


def decryption_setup(orc, rng, logn, mext, L, k, alpha, rots):
    """a ternary secret s, and for every (step, conj) the key that switches sigma(s) back to s, plus the NTT form of s"""
    n, q = 1 << logn, mext[:L]
    s = rng.words(n, 3).astype(np.int64) - 1
    s_ntt = orc.poly_reduce_strict(q, orc.poly_ntt(q, np.stack([(s % m).astype(U) for m in q])))
    keys = []
    for step, cj in rots:
        moved_s = centred(orc, q, move(orc, s_ntt, step, cj))
        keys.append(keygen(orc, rng, logn, mext, L, k, alpha, s, moved_s))
    return s_ntt, keys


def decryption_errors(orc, logn, q, ct, s_ntt, rots, outs):
    """max |coefficient| of out0 + out1 s - sigma_r(c0 + c1 s), per rotation"""
    plain = orc.poly_add(q, ct[0], orc.poly_mul(q, ct[1], s_ntt))
    worst = []
    for (step, cj), out in zip(rots, outs):
        lhs = orc.poly_add(q, np.ascontiguousarray(out[0]), orc.poly_mul(q, np.ascontiguousarray(out[1]), s_ntt))
        worst.append(centred_error(orc, logn, q, orc.poly_sub(q, lhs, move(orc, plain, step, cj))))
    return worst


# ---- the diagonal transform (hp_dev_ckks_lintrans_hks) -----------------------------------------------------------------------------
def model_lintrans(orc, logn, mext, L, k, alpha, ct, keys, steps, conj, diags):
    """ct [2][L][n], keys[r] [nd][2][E][n], diags[r] [E][n] or None -> the canonical residues of out, [2][L][n] (dtype object)"""
    n, E = 1 << logn, L + k
    D = model_digits(orc, logn, mext, L, k, alpha, ct[1])
    acc = [[np.zeros(n, dtype=object) for _ in range(E)] for _ in range(2)]
    c0sum = [np.zeros(n, dtype=object) for _ in range(L)]
    for key, step, cj, dg in zip(keys, steps, conj, diags):
        Dm = np.stack([move(orc, D[d], step, cj) for d in range(D.shape[0])]).astype(object)
        c0m = move(orc, ct[0], step, cj).astype(object)
        Ko = key.astype(object)
        for m in range(E):
            q, w = mext[m], (1 if dg is None else dg[m].astype(object))
            unmont = pow(1 << 64, -1, q)                                  # the inner sum's one Montgomery reduction
            for h in range(2):
                inner = sum(Dm[d, m] * Ko[d, h, m] for d in range(D.shape[0])) * unmont % q
                acc[h][m] = (acc[h][m] + w * inner) % q
            if m < L:
                c0sum[m] = (c0sum[m] + w * c0m[m]) % q
    # ModDown of model_rest: its inner product with the "key" (2^64 mod q on the diagonal) hands the accumulator through unchanged
    A = np.array(acc, dtype=object).astype(U)
    unit = np.zeros((2, 2, E, n), dtype=U)
    for m in range(E):
        unit[0, 0, m, :] = unit[1, 1, m, :] = (1 << 64) % mext[m]
    out = model_rest(orc, logn, mext, L, k, A, unit).astype(object)
    for m in range(L):
        out[0, m] = (out[0, m] + c0sum[m]) % mext[m]
        out[1, m] = out[1, m] % mext[m]
    return out


def random_diagonal(rng, mext, n):
    """[E][n] plain lazy words, half of them in [q, 2q)"""
    E = len(mext)
    d = rng.poly((E, n), mext)
    upper = rng.words(E * n, 2).reshape(E, n).astype(U)
    return d + upper * np.array(mext, dtype=U)[:, None]


def residues_match(got, exp, q):
    """got [2][L][n] u64 against exp [2][L][n] Python integers: the same residues, every word below 2q"""
    qa = np.array(q, dtype=U)[None, :, None]
    assert (got < 2 * qa).all()
    return np.array_equal((got % qa).astype(object), exp)


def single_case(eng, logn, L, k, alpha, seed=6200, mext=None):
    mext = mext or P.P40[:L] + P.P50[:k]
    n = 1 << logn
    rng = SplitMix(seed + logn)
    ct = rng.poly((2, 2, L, n), mext[:L])
    key = rng.poly(((L + alpha - 1) // alpha, 2, L + k, n), mext)
    d_ct, d_key = eng.to_device(ct), eng.to_device(key)
    hoisted = eng.to_host(eng.ckks_rotate_hoisted_hks(mext, k, alpha, d_ct, [d_key], [3]))[:, 0]
    lin = eng.to_host(eng.ckks_lintrans_hks(mext, k, alpha, d_ct, [d_key], [3], [None]))
    qa = np.array(mext[:L], dtype=U)[None, None, :, None]
    return hoisted % qa, lin % qa, bool((lin < 2 * qa).all())


# ---- its baby-step giant-step form (hp_dev_ckks_lintrans_bsgs_hks) -----------------------------------------------------------------
def mod_down(orc, logn, mext, L, k, acc):
    """acc [2][E] rows of Python integers -> ModDown, canonical residues [2][L][n] (dtype object): model_rest with the unit "key"
    (2^64 mod q on the diagonal), whose inner product hands the accumulator through unchanged"""
    n, E = 1 << logn, L + k
    A = np.array(acc, dtype=object).astype(U)
    unit = np.zeros((2, 2, E, n), dtype=U)
    for m in range(E):
        unit[0, 0, m, :] = unit[1, 1, m, :] = (1 << 64) % mext[m]
    out = model_rest(orc, logn, mext, L, k, A, unit).astype(object)
    for m in range(L):
        out[:, m] %= mext[m]
    return out


def model_switch_ext(orc, logn, mext, L, k, alpha, ct, key, step, cj, D=None):
    """one rotation's word set in the extended basis, [2][E] rows of Python integers: the contract's baby_i (and the giants' addend).
    D: the digit rows of ct[1], where the caller already has them"""
    n, E = 1 << logn, L + k
    Pprod = 1
    for p in mext[L:]:
        Pprod *= p
    if key is None:
        return [[(Pprod % mext[m]) * ct[h][m].astype(object) % mext[m] if m < L else np.zeros(n, dtype=object) for m in range(E)]
                for h in range(2)]
    if D is None:
        D = model_digits(orc, logn, mext, L, k, alpha, np.ascontiguousarray(ct[1]))
    Dm = np.stack([move(orc, D[d], step, cj) for d in range(D.shape[0])]).astype(object)
    c0m = move(orc, ct[0], step, cj).astype(object)
    Ko = key.astype(object)
    rows = [[None] * E for _ in range(2)]
    for m in range(E):
        q = mext[m]
        unmont = pow(1 << 64, -1, q)
        for h in range(2):
            w = sum(Dm[d, m] * Ko[d, h, m] for d in range(D.shape[0])) * unmont % q
            if h == 0 and m < L:
                w = (w + (Pprod % q) * c0m[m]) % q
            rows[h][m] = w
    return rows


def model_bsgs(orc, logn, mext, L, k, alpha, ct, bkeys, bsteps, bconj, gkeys, gsteps, gconj, diags):
    """ct [2][L][n]; keys [nd][2][E][n] or None; diags[g][i] [E][n] or None -> the canonical residues of out, [2][L][n] (dtype object)"""
    n, E = 1 << logn, L + k
    D = model_digits(orc, logn, mext, L, k, alpha, np.ascontiguousarray(ct[1]))
    baby = [model_switch_ext(orc, logn, mext, L, k, alpha, ct, key, s, c, D) for key, s, c in zip(bkeys, bsteps, bconj)]
    acc = [[np.zeros(n, dtype=object) for _ in range(E)] for _ in range(2)]
    for g, (key, s, c) in enumerate(zip(gkeys, gsteps, gconj)):
        pre = [[np.zeros(n, dtype=object) for _ in range(E)] for _ in range(2)]
        for i, dg in enumerate(diags[g]):
            if dg is None:
                continue
            for h in range(2):
                for m in range(E):
                    pre[h][m] = (pre[h][m] + dg[m].astype(object) * baby[i][h][m]) % mext[m]
        if key is not None:
            u = mod_down(orc, logn, mext, L, k, pre).astype(U)
            pre = model_switch_ext(orc, logn, mext, L, k, alpha, u, key, s, c)
        for h in range(2):
            for m in range(E):
                acc[h][m] = (acc[h][m] + pre[h][m]) % mext[m]
    return mod_down(orc, logn, mext, L, k, acc)


def dev(eng, xs):
    return [None if x is None else eng.to_device(x) for x in xs]


def flat_case(eng, logn, L, k, alpha, seed=7200, mext=None):
    mext = mext or P.P40[:L] + P.P50[:k]
    n = 1 << logn
    rng = SplitMix(seed + logn)
    steps, conj = [1, 0, 5], [False, True, False]
    ct = rng.poly((2, 2, L, n), mext[:L])
    dkeys = [eng.to_device(rng.poly(((L + alpha - 1) // alpha, 2, L + k, n), mext)) for _ in steps]
    ddiags = [eng.to_device(random_diagonal(rng, mext, n)) for _ in steps]
    d_ct = eng.to_device(ct)
    flat = eng.to_host(eng.ckks_lintrans_hks(mext, k, alpha, d_ct, dkeys, steps, ddiags, conj))
    bsgs = eng.to_host(eng.ckks_lintrans_bsgs_hks(mext, k, alpha, d_ct, dkeys, steps, [None], [0], [ddiags], conj))
    qa = np.array(mext[:L], dtype=U)[None, None, :, None]
    return flat % qa, bsgs % qa, bool((bsgs < 2 * qa).all())
