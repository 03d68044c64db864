"""Inputs and range arithmetic for the hoisted / diagonal / BSGS hybrid key switch on wide and off-table moduli
(tests/test_gpu_hks_moduli.py on the GPU, tests/test_hks_edges.py for the inputs' own conditions, no GPU).

Chains: the named chains of tests/moduli.py cut to (L, k), and WIDE58 -- every modulus 58 or 59 bits wide, just below and just above
the power of two and the 58-bit high_mid prime (kb = 59, large delta: hehub's lazy transform words exceed 2q there).  It is the chain
at which the carry out of the middle column of hp_mac2's carry-save sum (hp_device.h: cx) first fires and at which the 128-bit sums
of k_hks_inner_lintrans / k_hks_bsgs_presum come nearest to wrapping.

Range arithmetic: `sums` recomputes with Python integers what one launch of those kernels accumulates -- the digit sum of every
rotation, the word it reduces to (plus the folded c0 word), the sum over the rotations weighted by the diagonals -- from the words the
device really reads at level B: the caller's own words inside a digit, the oracle's lazy transform of the lifted value elsewhere
(hks_model.model_digits)."""
import numpy as np

import moduli as M
from hks_model import below_2q, crt, model_digits, move, random_diagonal, rotations_of

U = np.uint64
M64 = (1 << 64) - 1
TABLE = 32    # HP_HOIST_TABLE_MAX == HP_BSGS_TABLE_MAX: rotations / babies per launch
F = M.FAMILIES


# ---- chains --------------------------------------------------------------------------------------------------------------------
# Further primes of a chain's own kind, for the shapes a named chain is too short for: narrow ones join the ciphertext moduli,
# wide ones the special primes (in front of the chain's own last modulus).
EXTRA = {
    "ABOVE": {"q": [F[36]["above"], F[30]["above"]], "p": [F[50]["above"]]},
    "HIGHMID": {"q": [F[41]["high_mid"], F[36]["high_mid"]], "p": [F[50]["high_mid"]]},
    "LOWMID": {"q": [F[40]["low_mid_1.05"]], "p": [F[45]["low_mid_1.1"]]},
}


def cut(name, L, k):
    """the named chain cut to L ciphertext moduli and k special primes: chain[:L] + chain[-k:] where the chain is long enough"""
    chain = M.CHAINS[name]
    if L + k <= len(chain):
        return chain[:L] + chain[-k:]
    more = EXTRA[name]
    return (chain[:-1] + more["q"])[:L] + (more["p"] + chain[-1:])[-k:]


def _walk(first, up):
    """first, then the following primes = 1 (mod 2^17) on the same side of it"""
    q = first
    while True:
        yield q
        q = M.prime_at(q + 1 if up else q, M.step_bits(58), up)


def wide58(L, k):
    """L + k distinct primes drawn in turn from five positions of the 58- and 59-bit octaves (the FAMILIES member first, then
    prime_at's next ones at the same position); the k largest are the special primes, the others keep their order."""
    walks = [_walk(F[59]["above"], True), _walk(F[58]["high_mid"], True), _walk(F[59]["below"], False),
             _walk(F[58]["above"], True), _walk(F[58]["below"], False)]
    drawn = [next(walks[i % len(walks)]) for i in range(L + k)]
    special = sorted(drawn)[-k:]
    return [q for q in drawn if q not in special] + special


def chain_of(name, L, k):
    return wide58(L, k) if name == "WIDE58" else cut(name, L, k)


def digit_products(mext, L, alpha):
    out = []
    for first in range(0, L, alpha):
        prod = 1
        for q in mext[first:min(first + alpha, L)]:
            prod *= q
        out.append(prod)
    return out


def covers(mext, L, k, alpha):
    """the product of the special primes is at least every digit's product"""
    prod = 1
    for p in mext[L:]:
        prod *= p
    return all(d <= prod for d in digit_products(mext, L, alpha))


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def kind_rows(rng, shape, moduli, start=0, kinds=M.INPUT_KINDS):
    """[..., len(moduli), n]: every (polynomial, limb) row one of the edge input kinds, cycled as test_gpu_moduli._rows does"""
    shape = tuple(shape)
    x = np.empty(shape, dtype=U)
    flat = x.reshape(-1, shape[-2], shape[-1])
    for b in range(flat.shape[0]):
        for j, q in enumerate(moduli):
            flat[b, j] = M.edge_words(rng, kinds[(start + b + j) % len(kinds)], q, shape[-1])
    return x


def max_rows(shape, moduli):
    """every word 2q - 1"""
    return kind_rows(None, shape, moduli, kinds=("max",))


def lazy_uniform(rng, shape, moduli):
    """uniform words below 2q"""
    return rng.poly(shape, [2 * q for q in moduli])


# ---- range arithmetic ----------------------------------------------------------------------------------------------------------
def host_bound(mext, nd, R):
    """hpi::hks_lintrans_max_rotations' premise: (word, sum) = (w, w * 2q * R) with w = 4 nd ceil(q^2 / 2^64) + 3q for the largest q"""
    q = max(mext)
    w = 4 * nd * ((q * q >> 64) + 1) + 3 * q
    return w, w * 2 * q * R


def harvey_lazy(a, w, q):
    """hp_harvey_lazy on an object array: a * w - floor(a * floor(w 2^64 / q) / 2^64) * q in 64-bit words (below 2q for any a)"""
    wh = (w << 64) // q
    return (a * w - ((a * wh) >> 64) * q) & M64


def sums(orc, logn, mext, L, k, alpha, ct, rots, groups, D=None, carries=True):
    """What one launch accumulates for ciphertext ct [2][L][n].  rots: (key [nd][2][E][n] or None, step, conj) per rotation / baby, a
    None key the identity baby; groups: lists of one diagonal ([E][n], or None for the constant 1; "absent" for no term) per rotation --
    one list for the flat call, one per giant for the pre-sum.  Returns the largest
      digit   digit word read (`ratio`: the largest word / modulus quotient)
      inner   sum_d digit word * key word                                  (128-bit accumulator of the digit loop)
      word    Montgomery word of that sum + the folded c0 word             (a 64-bit register; the bound 4 nd t + 3q is about it)
      outer   sum_r diagonal word * word_r                                 (128-bit accumulator of the outer / pre-sum loop)
    each with the (modulus index, rotation or group) where it occurs, and with `carries` the largest counts cx_inner / cx_outer of
    carries out of the middle carry-save column of the two accumulators (0: the carry never fires)."""
    n, E = 1 << logn, L + k
    if D is None:
        D = model_digits(orc, logn, mext, L, k, alpha, np.ascontiguousarray(ct[1]))
    nd = D.shape[0]
    pprod = 1
    for p in mext[L:]:
        pprod *= p
    worst = {"digit": (0, None), "inner": (0, None), "word": (0, None), "outer": (0, None), "ratio": (0.0, None),
             "cx_inner": (0, None), "cx_outer": (0, None)}

    def note(what, value, where):
        if value > worst[what][0]:
            worst[what] = (value, where)

    def cross_carries(xs, ys):
        """hp_mac2's count cx for sum_j xs[j] * ys[j]: the carries out of the middle column sum_j (x0 y1 + x1 y0), each addition
        carrying at most once, so their number is the exact column sum's part above 2^64"""
        lo, col = (1 << 32) - 1, 0
        for x, y in zip(xs, ys):
            col = col + (x & lo) * (y >> 32) + (x >> 32) * (y & lo)
        return int((col >> 64).max())

    for m in range(E):
        dmax = int(D[:, m].max())
        note("digit", dmax, (m,))
        note("ratio", dmax / mext[m], (m,))
    words = []      # words[r][h][m]: object arrays, the 64-bit word rotation r hands the outer sum
    for r, (key, step, cj) in enumerate(rots):
        rows = [[None] * E for _ in range(2)]
        if key is None:
            for h in range(2):
                for m in range(E):
                    rows[h][m] = harvey_lazy(ct[h][m].astype(object), pprod % mext[m], mext[m]) if m < L else np.zeros(n, dtype=object)
            words.append(rows)
            continue
        Dm = np.stack([move(orc, D[d], step, cj) for d in range(nd)]).astype(object)
        c0m = move(orc, np.ascontiguousarray(ct[0]), step, cj).astype(object)
        Ko = key.astype(object)
        for m in range(E):
            q = mext[m]
            for h in range(2):
                acc = sum(Dm[d, m] * Ko[d, h, m] for d in range(nd))
                note("inner", int(acc.max()), (m, r))
                if carries:
                    note("cx_inner", cross_carries([Dm[d, m] for d in range(nd)], [Ko[d, h, m] for d in range(nd)]), (m, r))
                pairs = np.stack([(acc & M64).astype(U), (acc >> 64).astype(U)], axis=1)      # (asserted below 2^128 by the callers)
                w = orc.montgomery_128_lazy(q, pairs).astype(object)
                if h == 0 and m < L:
                    w = w + harvey_lazy(c0m[m], pprod % q, q)
                note("word", int(w.max()), (m, r))
                rows[h][m] = w
        words.append(rows)
    for g, diags in enumerate(groups):
        for m in range(E):
            for h in range(2):
                acc = np.zeros(n, dtype=object)
                xs, ys = [], []
                for r, dg in enumerate(diags):
                    if isinstance(dg, str):
                        continue
                    xs.append(words[r][h][m])
                    ys.append(1 if dg is None else dg[m].astype(object))
                    acc = acc + xs[-1] * ys[-1]
                note("outer", int(acc.max()), (m, g))
                if carries:
                    note("cx_outer", cross_carries(xs, ys), (m, g))
    return worst


def report(name, worst, mext, nd, R):
    """one line per case: the measured sums against 2^128 and against the host formula's premise"""
    w, s = host_bound(mext, nd, R)
    lg = lambda v: f"2^{np.log2(float(v)):.3f}" if v else "0"
    print(f"{name}: largest digit word {worst['ratio'][0]:.3f} q at modulus {worst['ratio'][1]}; inner sum {lg(worst['inner'][0])}; "
          f"word {lg(worst['word'][0])} (host premise 4 nd t + 3q = {lg(w)}); outer sum {lg(worst['outer'][0])} "
          f"(host premise w 2q R = {lg(s)}; limit 2^128)")
    return w, s


# ---- the flat transform at a spread of coefficients ------------------------------------------------------------------------------
def sampled_lintrans(orc, logn, mext, L, k, alpha, ct, keys, steps, conj, diags, sel, D=None):
    """hks_model.model_lintrans at the coefficients `sel` of every output row: the canonical residues [2][L][len(sel)].
    A None key is an identity term diag * (c0, c1) and the diagonal "absent" no term: the BSGS call with identity giants only.
    ModDown needs the special-prime rows of the accumulator whole (their inverse transform mixes all coefficients); the ciphertext
    moduli's rows only where they are compared.  With sel = range(n) this is model_lintrans (tests/test_hks_edges.py holds it to that)."""
    n, E = 1 << logn, L + k
    sel = np.asarray(sel)
    if D is None:
        D = model_digits(orc, logn, mext, L, k, alpha, np.ascontiguousarray(ct[1]))
    nd = D.shape[0]
    at = [sel if m < L else np.arange(n) for m in range(E)]
    acc = [[np.zeros(len(at[m]), dtype=object) for m in range(E)] for _ in range(2)]
    csum = [[np.zeros(len(sel), dtype=object) for _ in range(L)] for _ in range(2)]     # the c0 (and, for an identity term, c1) part
    for key, step, cj, dg in zip(keys, steps, conj, diags):
        if isinstance(dg, str):
            continue
        if key is None:                          # the identity: diag * (c0, c1), no key switch
            for m in range(L):
                for h in range(2):
                    csum[h][m] = (csum[h][m] + (1 if dg is None else dg[m][sel].astype(object)) * ct[h][m][sel].astype(object)) % mext[m]
            continue
        Dm = np.stack([move(orc, D[d], step, cj) for d in range(nd)])
        c0m = move(orc, np.ascontiguousarray(ct[0]), step, cj)
        for m in range(E):
            q, i = mext[m], at[m]
            w = 1 if dg is None else dg[m][i].astype(object)
            unmont = pow(1 << 64, -1, q)
            for h in range(2):
                inner = sum(Dm[d, m][i].astype(object) * key[d, h, m][i].astype(object) for d in range(nd)) * unmont % q
                acc[h][m] = (acc[h][m] + w * inner) % q
            if m < L:
                csum[0][m] = (csum[0][m] + w * c0m[m][i].astype(object)) % q
    # ModDown word for word as model_rest does it (the accumulator handed through its inner product with the unit "key", hehub's lazy
    # subtraction of the transformed remainder, * P^-1): the representatives matter where the remainder's lazy transform words exceed
    # 2q -- at high_mid moduli hehub's subtraction then wraps, and what comes out depends on the word it is subtracted from
    def handed(a, q):
        x = a * ((1 << 64) % q)
        return orc.montgomery_128_lazy(q, np.stack([(x & M64).astype(U), (x >> 64).astype(U)], axis=1))

    pm = mext[L:]
    pprod = 1
    for p in pm:
        pprod *= p
    out = np.empty((2, L, len(sel)), dtype=object)
    for h in range(2):
        yp = orc.poly_reduce_strict(pm, orc.poly_intt(pm, np.stack([handed(acc[h][m], mext[m]) for m in range(L, E)])))
        ys = [crt([yp[j][i] for j in range(k)], pm)[0] for i in range(n)]
        for m in range(L):
            q = mext[m]
            rem = orc.ntt(logn, q, np.array([(y % q) if y < pprod // 2 else q - ((pprod - y) % q) for y in ys], dtype=U))
            diff = orc.poly_sub([q], handed(acc[h][m], q)[None], below_2q(np.ascontiguousarray(rem[sel][None]), [q]))
            down = orc.poly_rns_scalar_mul([q], diff, [pow(pprod % q, -1, q)])[0].astype(object)
            out[h, m] = (down + csum[h][m]) % q
    return out


# ---- cases: the same inputs for the range arithmetic (no GPU) and for the comparison on the GPU -----------------------------------
FILLS = ("lazy", "kinds", "max", "edge")


def _pools(rng, fill, n, nd, mext, L):
    """(ciphertext builder, key pool, diagonal pool) of a fill:
      lazy   ciphertexts as a chained hehub call hands them in (moduli.lazy_rows), keys uniform below 2q, random lazy diagonals and a None
      kinds  every row of everything one of moduli.INPUT_KINDS, cycled
      max    every word of everything 2q - 1
      edge   ciphertext rows cycled over the kinds (the lifted digits then vary), every key and diagonal word 2q - 1: the largest sums
             real digit rows give"""
    E, q = len(mext), mext[:L]
    if fill == "lazy":
        return (lambda B: M.lazy_rows(rng, (B, 2, L, n), q), [lazy_uniform(rng, (nd, 2, E, n), mext) for _ in range(3)],
                [random_diagonal(rng, mext, n), None, random_diagonal(rng, mext, n), random_diagonal(rng, mext, n)])
    if fill == "kinds":
        return (lambda B: kind_rows(rng, (B, 2, L, n), q), [kind_rows(rng, (nd, 2, E, n), mext, start=s) for s in range(3)],
                [kind_rows(rng, (E, n), mext, start=s) for s in range(4)] + [None])
    ct = (lambda B: max_rows((B, 2, L, n), q)) if fill == "max" else (lambda B: kind_rows(rng, (B, 2, L, n), q))
    return ct, [max_rows((nd, 2, E, n), mext)], [max_rows((E, n), mext)]


def flat_inputs(name, logn, L, k, alpha, B, R, fill, seed, mext=None):
    """one case of the hoisted call (without the diagonals) or of the flat transform; mext: a chain of the caller's, name unused"""
    from oracle.pyoracle import SplitMix

    mext, n, nd = mext or chain_of(name, L, k), 1 << logn, (L + alpha - 1) // alpha
    make_ct, kpool, dpool = _pools(SplitMix(seed), fill, n, nd, mext, L)
    steps, conj = rotations_of(logn, R)
    return dict(mext=mext, logn=logn, L=L, k=k, alpha=alpha, ct=make_ct(B), kpool=kpool, dpool=dpool, steps=steps, conj=conj,
                which=[(r * 3 + 1) % len(kpool) for r in range(R)], wd=[(r * 2 + 1) % len(dpool) for r in range(R)])


def bsgs_inputs(name, logn, L, k, alpha, B, nb, ng, fill, seed, keyed_giants=True, mext=None):
    """one case of the BSGS transform: baby 0 and giant 0 the identity (no key), one diagonal absent where there are more than four;
    keyed_giants False: every giant the identity (the call is then a flat transform over giants x babies terms)"""
    from oracle.pyoracle import SplitMix

    mext, n, nd = mext or chain_of(name, L, k), 1 << logn, (L + alpha - 1) // alpha
    make_ct, kpool, dpool = _pools(SplitMix(seed), fill, n, nd, mext, L)
    dpool = [d for d in dpool if d is not None]
    bsteps, bconj = rotations_of(logn, nb)
    gsteps, gconj = rotations_of(logn, ng) if keyed_giants else ([0] * ng, [False] * ng)
    bsteps[0], bconj[0], gsteps[0], gconj[0] = 0, False, 0, False          # the identities
    bwhich = [None] + [(r * 3 + 1) % len(kpool) for r in range(1, nb)]
    gwhich = [None] + [((r * 3 + 2) % len(kpool) if keyed_giants else None) for r in range(1, ng)]
    wd = [[(g * nb + i) % len(dpool) for i in range(nb)] for g in range(ng)]
    if nb * ng > 4:
        wd[ng - 1][1] = None            # an absent diagonal
    return dict(mext=mext, logn=logn, L=L, k=k, alpha=alpha, ct=make_ct(B), kpool=kpool, dpool=dpool, bsteps=bsteps, bconj=bconj,
                gsteps=gsteps, gconj=gconj, bwhich=bwhich, gwhich=gwhich, wd=wd)


def pick(pool, idx):
    return [None if i is None else pool[i] for i in idx]


def flat_sums(orc, c, b=0):
    """sums() of ciphertext b of a flat_inputs case"""
    keys, diags = pick(c["kpool"], c["which"]), pick(c["dpool"], c["wd"])
    return sums(orc, c["logn"], c["mext"], c["L"], c["k"], c["alpha"], c["ct"][b], list(zip(keys, c["steps"], c["conj"])), [diags],
                carries=c["logn"] <= 6)


def presum_sums(orc, c, b=0):
    """sums() of the baby stage and the pre-sum of ciphertext b of a bsgs_inputs case (an absent diagonal: no term)"""
    keys = pick(c["kpool"], c["bwhich"])
    groups = [["absent" if i is None else c["dpool"][i] for i in row] for row in c["wd"]]
    return sums(orc, c["logn"], c["mext"], c["L"], c["k"], c["alpha"], c["ct"][b], list(zip(keys, c["bsteps"], c["bconj"])), groups,
                carries=c["logn"] <= 6)


# ---- the cases of tests/test_gpu_hks_moduli.py (tests/test_hks_edges.py checks their conditions without a GPU) ----------------------
MODEL_CHAINS = ("W59", "ABOVE", "PACKEDGE", "HIGHMID", "LOWMID", "WIDE58")
MODEL_SHAPES = [(5, 4, 2, 2), (5, 5, 2, 2), (11, 3, 2, 2)]         # (logn, L, k, alpha): a short last digit; tiled transforms, fused ModDown
EXTREMAL_CHAINS = ("W59", "HIGHMID", "WIDE58")
EXTREMAL_SHAPE = (5, 4, 2, 2)
ALL_MAX_SHAPE = (5, 2, 2, 2)                                       # alpha = L: every ciphertext-modulus digit row is the caller's own word
EDGE_SHAPE = (16, 2, 1)                                            # (L, k, alpha): 16 digits, the most the ABI takes
EDGE_CASES = [(5, "lazy"), (5, "edge"), (10, "edge")]              # (logn, fill)
CHUNK_LOGNS = (9, 10)                                              # n = one HKS_LT_CHUNK; two chunks, the last degree of the generic transforms
LEVEL_A_SHAPES = {"ABOVE": (3, 2, 2), "PACK40EDGE": (3, 1, 2), "WIDE_EDGE": (4, 2, 2)}       # logn 11
LEVEL_B_ONLY_SHAPES = {"LOWMID": (3, 2, 2), "OVER50": (3, 1, 1), "HIGHMID": (3, 2, 2)}      # logn 12
CROSS_CHAINS = ("WIDE58", "HIGHMID")                               # logn 11, (3, 2, 2)


def edge_flat(logn, fill):
    L, k, alpha = EDGE_SHAPE
    return flat_inputs("WIDE58", logn, L, k, alpha, 1, TABLE, fill, 8300 + logn + FILLS.index(fill))


def edge_bsgs(logn, fill):
    """32 babies; at logn 5 two giants, one keyed; at logn 10 two identity giants (the sampled model has no second key switch)"""
    L, k, alpha = EDGE_SHAPE
    return bsgs_inputs("WIDE58", logn, L, k, alpha, 1, TABLE, 2, fill, 8400 + logn + FILLS.index(fill), keyed_giants=logn <= 6)


def all_max_flat(name):
    logn, L, k, alpha = ALL_MAX_SHAPE
    return flat_inputs(name, logn, L, k, alpha, 1, TABLE, "max", 0)


def all_max_bsgs(name):
    logn, L, k, alpha = ALL_MAX_SHAPE
    return bsgs_inputs(name, logn, L, k, alpha, 1, TABLE, 2, "max", 0)
