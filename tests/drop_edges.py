"""Coefficient-domain edge values for the drop-last-prime step and the RNS base transforms (tests/test_drop_edges.py for the builders'
own conditions and the model, no GPU; tests/test_gpu_drop_edges.py and tests/test_gpu_base_edges.py on the GPU).

The drop acts on the coefficients c = strict(INTT_{q_last}(x_last)) of the limb that leaves: a centring compare c >= floor(q_last / 2)
and a remainder modulo every q_k that stays.  Random or extremal words in the NTT domain give uniform coefficients, which meet none of
the values at which those two statements change behaviour; here the coefficients themselves are chosen, and reach the kernels either
through x_last = NTT(planted) (the whole entry points) or directly as the coefficient rows of the limb-range stage.

Plain Python and numpy.  The model is exact integer arithmetic; the factors of the BGV form are those hp_drop.h and
include/hehub_amd.h state: out_k = ((x_k - NTT_k(t * centre(c))) * q_last^-1 * (q_last mod t)) + addend_k (mod q_k)."""
import numpy as np

import moduli as M
import params as P

U = np.uint64
M64 = (1 << 64) - 1
BLOCKS = 32          # the coverage claim: every edge value in each of the 32 contiguous blocks of n / 32 coefficients, at both parities
BATCH = 3            # ciphertexts per call: P2 = 6 polynomials
PLAIN = (65537, 2, 1)


# ---- chains --------------------------------------------------------------------------------------------------------------------
def chains(logn):
    """name -> q_0 .. q_{L-1} usable at ring degree 2^logn (N = 65536 needs q = 1 mod 2^17, which some table primes are not)"""
    a, b, c = sorted(P.P40[:3])
    p50 = [P.P50[1], P.ntt_primes(2, 16, 50)[1]]                       # both 1 (mod 2^17)
    w59 = [M.Q59, M.NARROW[4]] if logn <= 15 else P.ntt_primes(2, 16, 59)
    return {
        "SAME40": [c, a, b],                       # q_last = b: one limb above it, one below; q_last <= 2 q_k (SMALL)
        "WIDE_LAST": [a, c, p50[0]],               # 40-bit limbs under a 50-bit last prime: quotients up to 2^10
        "NARROW_LAST": [p50[0], p50[1], b],        # 50-bit limbs over a 40-bit last prime: every coefficient is its own remainder
        "W59ish": [w59[0], M.NARROW[0], w59[1]],   # a 59-bit and a 20-bit limb under a 59-bit last prime: Barrett quotient near 2^39
        # SAME40's shape (SMALL) with the limb below q_last in mid-octave, 1.6 * 2^40 under a last prime just below 2^41.  Next to a
        # power of two hehub's last fold returns the same transform words for a remainder c and for c - q_k, so there a SMALL
        # remainder left unreduced computes the very words of the reduced one; at this limb the words differ
        "SMALL_MID": [M.FAMILIES[41]["above"], M.FAMILIES[40]["high_mid"], M.FAMILIES[41]["below"]],
    }


LEVEL_B_CHAINS = ("SAME40", "WIDE_LAST", "NARROW_LAST", "W59ish", "SMALL_MID")
SMALL_CHAINS = ("SAME40", "NARROW_LAST", "SMALL_MID")
TABLE_CHAINS = ("SAME40", "WIDE_LAST", "NARROW_LAST", "PACK40EDGE")     # moduli next to a power of two: hehub's subtraction never wraps


def chains_a(logn):
    return {"SAME40": chains(logn)["SAME40"], "PACK40EDGE": M.PACK40EDGE}


LEVEL_A_CHAINS = ("SAME40", "PACK40EDGE")


def chain_of(name, logn):
    return chains(logn)[name] if name in LEVEL_B_CHAINS else chains_a(logn)[name]


def small(chain, k0=0, k1=None):
    """hpi::drop_small_rem for the limbs [k0, k1)"""
    return all(chain[-1] <= 2 * q for q in chain[:-1][k0:k1])


# ---- edge coefficients -----------------------------------------------------------------------------------------------------------
def edge_values(chain, extended=False):
    """the sorted edge coefficients of a chain; extended: also the words from q_last on, for the entry point that takes any u64"""
    ql = chain[-1]
    h = ql // 2
    vals = {0, 1, h - 1, h, h + 1, ql - 2, ql - 1}
    for q in chain[:-1]:
        r = ql % q
        cand = [q - 1, q, q + 1, 2 * q - 1,
                h - 1 - ((h - 1 - r) % q),       # the largest value below h congruent to r: no bump, remainder r
                h + ((r - h) % q),               # the smallest value >= h congruent to r: remainder + bump = q, the lazy word for 0
                ((h - 1) // q) * q,              # the multiples of q nearest h on each side: remainder 0 without and with the bump
                -(-h // q) * q]
        vals.update(v for v in cand if 0 <= v < ql)
    if extended:
        vals.update([ql, ql + 1, 2 * ql - 1, 1 << 63, M64])
    return sorted(vals)


def _blocks(n):
    return min(BLOCKS, n // 2)


def per_row(n, count):
    """the coverage holds in every mixed row on its own (else: in the mixed rows taken together)"""
    return n // _blocks(n) // 2 >= count


def covered(rows, values):
    """every value occurs in each of the 32 contiguous blocks at both index parities of `rows` [R][n] taken together"""
    n, nb = rows.shape[-1], _blocks(rows.shape[-1])
    cells = rows.reshape(rows.shape[0], nb, n // nb // 2, 2)
    want = set(int(v) for v in values)
    return all(want <= set(int(v) for v in cells[:, b, :, par].ravel()) for b in range(nb) for par in range(2))


def mixed_rows(rng, n, values, count):
    """[count][n]: the slots of one (block, parity) cell over the rows hold the values in turn from an offset drawn per cell, then all
    cells are shuffled alike by one drawn permutation -- every value in every cell as soon as a cell has as many slots as values.
    Where one row's cell holds all the values, every row is built on its own."""
    nb = _blocks(n)
    slots = n // nb // 2
    if count > 1 and slots >= len(values):
        return np.concatenate([mixed_rows(rng, n, values, 1) for _ in range(count)])
    vals = np.array(values, dtype=U)
    total = count * slots
    off = rng.words(nb * 2, len(vals)).astype(np.int64)
    perm = np.argsort(rng.words(total), kind="stable")
    idx = (np.arange(total)[None, :] + off[:, None]) % len(vals)                   # [cell][total]
    cell = vals[idx][:, perm].reshape(nb, 2, count, slots)                          # [block][parity][row][slot]
    return np.ascontiguousarray(cell.transpose(2, 0, 3, 1).reshape(count, n))


def coefficient_rows(chain, n, seed, extended=False, p2=2 * BATCH):
    """[p2][n] coefficient rows: constant rows of h - 1, h and q_last - 1, then mixed rows of the edge values.  The coverage of the mixed
    rows is asserted here where the ring is large enough to hold it: the register slot and the lane of the pair swap a coefficient
    lands in are functions of its index bits, and which bits depends on log N."""
    from oracle.pyoracle import SplitMix

    assert 4 <= p2 <= 6
    ql = chain[-1]
    h, values = ql // 2, edge_values(chain, extended)
    rows = np.empty((p2, n), dtype=U)
    for i, v in enumerate((h - 1, h, ql - 1)):
        rows[i] = U(v)
    rows[3:] = mixed_rows(SplitMix(seed), n, values, p2 - 3)
    if (p2 - 3) * (n // _blocks(n) // 2) >= len(values):
        assert covered(rows[3:], values), "the mixed rows miss an edge value in some block or parity"
        if per_row(n, len(values)):
            assert all(covered(rows[i:i + 1], values) for i in range(3, p2))
    return rows


# ---- the exact model ---------------------------------------------------------------------------------------------------------------
def cen(c, ql):
    """the centred representative the drop subtracts, for any word c < 2^64 (c < q_last: the centred residue)"""
    return c - ql if c >= ql // 2 else c


def model_remainders(chain, t, c, k0=0, k1=None):
    """[k1 - k0][n]: the remainder rows the transform reads, t * cen(c) modulo q_k (t = 0: CKKS, no factor), in the words
    rescaling.cpp:54-69 / mod_switch.cpp:52-70 form them: (c mod q_k) + [c >= h] (q_k - q_last mod q_k), BGV: times t by hehub's lazy
    Harvey product.  That each word is congruent to t * cen(c) is asserted: the words only matter where hehub's subtraction wraps
    (model_drop)."""
    ql = chain[-1]
    h = ql // 2
    co = c.astype(object)
    centred = np.where(c >= U(h), co - ql, co) * (t or 1)
    assert all(cen(int(v), ql) * (t or 1) == w for v, w in zip(c[:64], centred[:64]))
    out = []
    for q in chain[:-1][k0:k1]:
        w = co % q + np.where(c >= U(h), q - ql % q, 0).astype(object)
        if t:
            assert t < q
            w = (w * t - ((w * ((t << 64) // q)) >> 64) * q) & M64
        assert ((w - centred) % q == 0).all() and (w < 2 * q).all()
        out.append(w.astype(U))
    return np.stack(out)


def model_drop(orc, chain, t, x, c, k0=0, k1=None, addend=None, note=None):
    """canonical residues [k1 - k0][n] of the drop of one polynomial x [L][n] given its coefficient row c [n]:
        ((x_k - NTT_k(t cen(c))) q_last^-1 [(q_last mod t)]) [+ addend_k]  (mod q_k)
    with the transform (linear, exact modulo q_k) taken by the oracle on the remainder row.  The difference is formed as hehub forms
    it, x + 2 q_k - w in a 64-bit word: at a modulus far from a power of two hehub's lazy transform words w pass 2 q_k
    (tests/moduli.py), the difference then wraps where w > x + 2 q_k, and the reference's result -- which the engine reproduces -- is
    the formula's plus 2^64 q_last^-1.  note["wraps"] counts those words; everywhere else the result IS the formula's."""
    ql, n = chain[-1], len(c)
    logn = n.bit_length() - 1
    k1 = len(chain) - 1 if k1 is None else k1
    rem = model_remainders(chain, t, c, k0, k1)
    out = np.empty((k1 - k0, n), dtype=U)
    for i, k in enumerate(range(k0, k1)):
        q = chain[k]
        f = pow(ql, -1, q) * ((ql % t) if t else 1) % q
        d = x[k].astype(object) + 2 * q - orc.ntt(logn, q, rem[i]).astype(object)
        if note is not None:
            note["wraps"] = note.get("wraps", 0) + int((d < 0).sum())
        v = (d & M64) * f
        if addend is not None:
            v = v + addend[i].astype(object)
        out[i] = (v % q).astype(U)
    return out


def canon(a, moduli):
    return a % np.array(moduli, dtype=U)[:, None]


# ---- inputs of the whole entry points ------------------------------------------------------------------------------------------------
def planted_ct(orc, rng, chain, n, planted, t=0):
    """[B][2][L][n]: the limbs that stay as a chained call hands them in (moduli.lazy_rows), the last limb the transform of the planted
    coefficient rows (BGV: of planted * t, since the inverse transform of the last limb is followed by * t^-1)"""
    L, ql, logn = len(chain), chain[-1], n.bit_length() - 1
    B = planted.shape[0] // 2
    x = M.lazy_rows(rng, (B, 2, L, n), chain)
    for p2 in range(2 * B):
        row = planted[p2] if not t else ((planted[p2].astype(object) * t) % ql).astype(U)
        x[p2 // 2, p2 % 2, L - 1] = orc.ntt(logn, ql, row)
    return x


# ---- which copy of the drop a call reaches (hp_api_scheme.cpp: drop_apply; hp_ctx.h: tiled_ok, fused_drop_ok, split_ok) ---------------
ROUTES = ("default", "tiled", "unfused", "generic")      # engine: as created; HP_SPLIT_MAX_ITEMS=0; HP_NO_FUSED_DROP=1; force_generic


def routes(logn):
    out = ["default"]
    if logn >= 12:
        out.append("tiled")
    if logn in (11, 15):
        out += ["unfused", "generic"]
    return out


def copy_reached(logn, route, items, level_a=False):
    """the drop's copy a launch of `items` = limbs * polynomials takes -- "rem/fin" (hp_edge.hip: k_drop_rem, k_drop_fin), "eager"
    (hp_ntt_fast.hip, prologue of ntt_fwd_body), "DropPre" (hp_ntt_fast.hip), "split" (hp_ntt_split.hip), "DropPreA" (hp_ntt_a.hip).
    Flavour 0 at N = 32768 keeps the eager form (see flavour_copy)."""
    tiled_ok = route != "generic" and 11 <= logn <= 15
    fused = tiled_ok and route != "unfused"
    few = route != "generic" and 12 <= logn <= 16 and 0 < items <= (0 if route == "tiled" else 128) and not level_a
    if fused and not few:
        return "DropPreA" if level_a else ("DropPre" if logn == 15 else "eager")
    if few and route != "unfused":
        return "split"
    return "rem/fin"


def flavour_copy(copy, flavour):
    return "eager" if copy == "DropPre" and flavour == 0 else copy
