"""Cases and inputs for hp_dev_ckks_lincomb and hp_dev_ckks_eval_plan_hks on wide and off-table moduli (tests/test_gpu_polyeval_moduli.py
on the GPU, tests/test_polyeval_edges.py for the cases' own conditions, no GPU).  The pattern of tests/hks_bgv_edges.py, whose chains,
fills and premises (and those of tests/hks_edges.py and tests/moduli.py) are imported, not copied.

Whole plans (hehub_amd/polyeval.py: n1 = 4, input scale = target scale = Delta), each 5 steps with 4 switches:
  W59      (6, 1)  59, 40 x 5 | 50            Chebyshev CHEB15[:8]   Delta 2^40     the wide limb is q_0: every level keeps it
  W59LAST  (6, 2)  40 x 5, 59 | 50, 50        Chebyshev CHEB15[:8]   Delta 2^40     the wide limb is the first q_last
  ABOVE    (6, 1)  45 41 42 46 37 31 | 50     Chebyshev CHEB15[:8]   Delta 2^40     2^k + small; level A at a tiled degree
  PACKEDGE (6, 1)  59 46 47 47 48 48 | 50     Chebyshev CHEB15[:8]   Delta 2^47     a different width at every level
  WIDE58R  (5, 1)  all 58 / 59 bits           power POWER7           Delta 2^58     the largest sums of every launch
Every step's level passes hks_bgv_edges.premise and drop_premise at logn 4 and 11 (tests/test_polyeval_edges.py asserts it; nothing is
skipped at run time).  The chains that cannot have a model ending in hehub's drop are named in DROP_FAILS (a high_mid limb kept by the
drop: HIGHMID, WIDE58) and PREMISE_FAILS (LOWMID from N = 32 on); they run in the pure-integer section (hp_dev_ckks_lincomb) and --
HIGHMID, WIDE58 -- in the word-for-word section, never against a model that ends in hehub's drop."""
from fractions import Fraction

import numpy as np

import hks_bgv_edges as E
import hks_edges as H
import moduli as M
from hehub_amd.polyeval import Form, Plan, build_plan
from hks_levels import level_chain
from polyeval_model import CHEB15, POWER7

U = np.uint64
F = M.FAMILIES
BATCH = 2
N1 = 4
LOGNS = (4, 11)
TABLE = 32                                   # HP_LINCOMB_MAX: terms of one launch of k_ct_lincomb
E0 = Form([(0, None)])                       # the input, as it lies

# ---- whole plans: name -> (L, k, alpha, basis, coefficients, Delta) -----------------------------------------------------------------
# alpha = 2 beside k = 1 (and beside two 50-bit primes under the 59-bit limb of W59LAST): hks_edges.covers fails, which is what the
# NOISE of a switch needs, not its residues (hks_bgv_edges.UNCOVERED) -- these cases are compared on residues only.  alpha = 2 gives a
# partial last digit at the odd levels and a full one at the even levels.
PLAN_CASES = {
    "W59": (6, 1, 2, "chebyshev", CHEB15[:8], 1 << 40),
    "W59LAST": (6, 2, 2, "chebyshev", CHEB15[:8], 1 << 40),
    "ABOVE": (6, 1, 2, "chebyshev", CHEB15[:8], 1 << 40),
    "PACKEDGE": (6, 1, 2, "chebyshev", CHEB15[:8], 1 << 47),
    "WIDE58R": (5, 1, 2, "power", POWER7, 1 << 58),
}
LEVEL_A_PLAN = ("ABOVE", 11)                 # the one (chain, degree) here that level A serves
TOP_KEY_PLANS = ("W59", "ABOVE")             # run once more under a key for key_L0 = L + 1
# chains without a model that ends in hehub's drop, and why (tests/test_polyeval_edges.py asserts the reasons)
DROP_FAILS = ("HIGHMID", "WIDE58")           # hks_bgv_edges.drop_premise fails at every level: a high_mid limb is kept by the drop
PREMISE_FAILS = ("LOWMID",)                  # hks_bgv_edges.premise fails from N = 32 on


def plan_chain(name):
    L, k = PLAN_CASES[name][:2]
    return E.chain_of(name, L, k)


def plan_of(name):
    L, k, alpha, basis, coefs, delta = PLAN_CASES[name]
    return build_plan(coefs, basis, plan_chain(name)[:L], delta, delta, n1=N1)


def top_chain(name, key_L0):
    """a top chain of key_L0 = L + 1 ciphertext moduli whose level-L chain is the case's own: the named chain one limb longer where it
    has one, else one more prime of the ABOVE kind in between (no level of the plan reads that row)"""
    L, k = PLAN_CASES[name][:2]
    mext = plan_chain(name)
    assert key_L0 == L + 1
    top = E.chain_of(name, key_L0, k)
    if len(top) != key_L0 + k or level_chain(top, key_L0, L, k) != mext:
        top = mext[:L] + [F[48]["above"]] + mext[L:]
    assert len(set(top)) == key_L0 + k and level_chain(top, key_L0, L, k) == mext
    return top


def step_levels(name):
    """the level of every step of a case's plan, and of the two single steps of section 3 (levels L - 1 and L)"""
    L = PLAN_CASES[name][0]
    return sorted({s.level for s in plan_of(name).steps} | ({L - 1, L} if name in Z_CHAINS else set()))


def modelled_levels():
    """(name, logn, level, the level's chain) of everything that is held against model_plan"""
    out = []
    for name in PLAN_CASES:
        L, k = PLAN_CASES[name][:2]
        mext = plan_chain(name)
        for logn in LOGNS:
            out += [(name, logn, lv, level_chain(mext, L, lv, k)) for lv in step_levels(name)]
    return out


def signed(rng, bits=100):
    """an integer of either sign, uniform in [-2^(bits-1), 2^(bits-1))"""
    half = bits // 2
    v = (int(rng.words(1, 1 << half)[0]) << (bits - half)) | int(rng.words(1, 1 << (bits - half))[0])
    return v - (1 << (bits - 1))


def plan_inputs(name, logn, key_L0=None):
    """(mext_top, lext, ct [BATCH][2][L][n] lazy words -- two different ciphertexts --, a top-shaped key of lazy words)"""
    from oracle.pyoracle import SplitMix

    L, k, alpha = PLAN_CASES[name][:3]
    key_L0 = key_L0 or L
    mtop = plan_chain(name) if key_L0 == L else top_chain(name, key_L0)
    n = 1 << logn
    rng = SplitMix(11000 + 131 * sorted(PLAN_CASES).index(name) + 17 * logn + key_L0)
    ct = M.lazy_rows(rng, (BATCH, 2, L, n), mtop[:L])
    key = H.lazy_uniform(rng, (E.nd_of(key_L0, alpha), 2, key_L0 + k, n), mtop)
    return mtop, mtop[:L] + mtop[key_L0:], ct, key


# ---- 1. hp_dev_ckks_lincomb: pure integer arithmetic, no premise -----------------------------------------------------------------------
LINCOMB_EXTRA = (0, 1, 2)                    # limbs an operand is stored with beyond L, by term
LINCOMB_TERMS = (1, TABLE, TABLE + 1)        # one term, a full table, a second (accumulating) launch
LINCOMB_CHAINS = tuple(M.CHAINS) + ("WIDE58", "W59LAST")
LINCOMB_MAX_CHAINS = ("WIDE58", "NARROW")    # every operand word 2q - 1, every coefficient and the constant q - 1
LINCOMB_FULL_TILES = ("W59", 13)             # 2048-word tiles, once


def lincomb_chain(name):
    """(q_top, L): the whole named chain, special primes included (to this call they are moduli like any other), read in its first
    L = min(3, len - 2) limbs, so that operands with 0, 1 and 2 more limbs exist on every chain"""
    if name == "WIDE58":
        top = H.wide58(3, 2)                 # five primes of 58 / 59 bits
    elif name == "W59LAST":
        top = E.chain_of(name, 3, 2)         # the 59-bit prime as the last limb read
    else:
        top = list(M.CHAINS[name])
    return top, min(3, len(top) - 2)


PLANTED = (None, 0, None, 1, -1)             # residues planted over the (term, limb) grid: random, 0, random, 1, q - 1


def lincomb_inputs(name, logn, T):
    """(q, operands [BATCH][2][L + extra][n] of moduli.lazy_rows, coefs [T][L], cst [L]): signed integers up to 2^100 reduced per limb,
    the residues 0, 1 and q - 1 planted"""
    from oracle.pyoracle import SplitMix

    top, L = lincomb_chain(name)
    q, n = top[:L], 1 << logn
    rng = SplitMix(11500 + 131 * LINCOMB_CHAINS.index(name) + 17 * logn + T)
    cts = [M.lazy_rows(rng, (BATCH, 2, L + LINCOMB_EXTRA[j % 3], n), top[:L + LINCOMB_EXTRA[j % 3]]) for j in range(T)]

    def residues(at):
        c = signed(rng)
        out = []
        for m, qm in enumerate(q):
            plant = PLANTED[(at + m) % len(PLANTED)]
            out.append(c % qm if plant is None else plant % qm)
        return out

    coefs = [residues(j * L) for j in range(T)]
    return q, cts, coefs, residues(T * L + 4 - (T * L) % len(PLANTED))       # (the constant begins at q - 1)


# ---- 2. a step is the calls it is composed of, word for word ----------------------------------------------------------------------------
STEP_CHAINS = ("W59", "HIGHMID", "WIDE58", "WIDE58R")
STEP_SHAPES = (E.FIRST, E.TILED)
TOP_KEY_STEPS = ("W59", "WIDE58")            # key_L0 = L + 1: the plan reads a top-level key, the composed calls its compact sub-key
STEP_CASES = [(name,) + s for name in STEP_CHAINS for s in STEP_SHAPES]


def step_key_L0(case):
    return case[2] + 1 if case[0] in TOP_KEY_STEPS else case[2]


# ---- 3. Z added to the quad ---------------------------------------------------------------------------------------------------------------
Z_CHAINS = ("W59", "W59LAST", "WIDE58R")
Z_TERMS = TABLE + 1                          # (a): two launches, both accumulating into the 3-polynomial quad


def z_two_launch_plan(name, rng):
    """(a) one product of the input's first L - 1 limbs (materialised: the element has one limb more than the level) with itself, plus
    a Z of 33 terms over the same element and a constant"""
    L = PLAN_CASES[name][0]
    q = plan_chain(name)[:L]
    plan = Plan(q, 1)
    plan.add(L - 1, [(Form([(0, signed(rng))]), Form([(0, None)]))], Form([(0, signed(rng)) for _ in range(Z_TERMS)], signed(rng)), 1)
    return plan


def z_max_plan(name):
    """(b) the step [(E0, E0)] with Z = 32 x (E0, -1) - 1: every coefficient residue and the constant's are q - 1"""
    L = PLAN_CASES[name][0]
    plan = Plan(plan_chain(name)[:L], 1)
    plan.add(L, [(E0, E0)], Form([(0, -1)] * TABLE, -1), 1)
    return plan


def accumulate_max(q, terms=TABLE):
    """the largest sum an accumulating launch of `terms` terms forms: operand words 2q - 1, coefficients and the constant q - 1, on top
    of an accumulated word below 2q"""
    return terms * (q - 1) * (2 * q - 1) + (q - 1) + (2 * q - 1)


def montgomery_limit(q):
    """the largest 128-bit sum whose Montgomery word hi + mulhi(u, q) + 1 still fits 64 bits (tests/test_lincomb_host.py)"""
    return ((1 << 64) - q) * (1 << 64) - 1


def report_accumulate_max(name):
    """one line, as hks_bgv_edges.report_max_fill prints: how close the largest sum of 3(b) comes to 2^128"""
    L = PLAN_CASES[name][0]
    q = max(plan_chain(name)[:L])
    lg = float(np.log2(float(accumulate_max(q))))
    print(f"{name}: largest accumulate sum (32 terms, constant, accumulated word) 2^{lg:.3f} at the modulus 2^{np.log2(float(q)):.3f}, "
          f"2^128 / sum = 2^{128 - lg:.3f}; the Montgomery step's limit / sum = {montgomery_limit(q) / accumulate_max(q):.3f}")
    return 128 - lg


# ---- 5. by decryption ---------------------------------------------------------------------------------------------------------------------
# WIDE58R (5, 1) with alpha = 1: one 60-bit special prime covers every one-limb digit (hks_edges.covers), so the switches' noise is small
DECRYPT = dict(name="WIDE58R", L=5, k=1, alpha=1, n1=N1, delta=1 << 58, xs=(0.73, -0.5))
# max |dec - Delta p(x)| over all coefficients, measured in the CPU model alone (tests/test_polyeval_edges.py: model-made key and
# noise, the values above) at each ring degree; the device test's threshold is 8 x the measurement at its own degree -- the project's
# margin for other keys and errors than the model drew (polyeval_model.E2E_THRESHOLD)
DECRYPT_MEASURED = {4: 3, 11: 42}             # 2^-56.4 and 2^-52.6 of Delta: the rescales' roundings, about sqrt(N), whatever the scale
DECRYPT_THRESHOLD = {logn: 8 * v for logn, v in DECRYPT_MEASURED.items()}


def decrypt_chain():
    return E.chain_of(DECRYPT["name"], DECRYPT["L"], DECRYPT["k"])


def decrypt_plan():
    d = DECRYPT
    return build_plan(POWER7, "power", decrypt_chain()[:d["L"]], d["delta"], d["delta"], n1=d["n1"])


def exact_power(coefs, v, delta):
    """round(delta p(v / delta)) in exact rationals (a 58-bit scale is beyond a float's 53 bits)"""
    from hehub_amd.polyeval import _round

    x = Fraction(v, delta)
    return _round(sum(Fraction(c) * x ** j for j, c in enumerate(coefs)) * delta)
