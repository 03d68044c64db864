"""The drop-last-prime step on planted COEFFICIENTS (tests/drop_edges.py): floor(q_last / 2) and its neighbours, q_k and 2 q_k - 1,
the coefficients whose remainder (plus bump) is exactly 0 or q_k, q_last - 1 -- in every block of the ring and at both index parities,
so that every register slot and both lanes of the pair swap see them.  Every copy of the step is reached by a known route (the case
ids name it; tests/test_drop_edges.py checks the ids' claims against hp_drop_flavour_b / hp_drop_flavour_a and the routing of
drop_apply without a GPU):

  rem/fin   hp_edge.hip k_drop_rem + k_drop_fin    N <= 1024, N = 65536 without the split, HP_NO_FUSED_DROP, force_generic
  eager     hp_ntt_fast.hip, prologue of ntt_fwd_body    N = 2048 .. 16384 tiled; flavour 0 at N = 32768
  DropPre   hp_ntt_fast.hip                        N = 32768 tiled, flavours 1 .. 5
  split     hp_ntt_split.hip, DROP && FIRST        N >= 4096 by default (a launch of at most 128 limbs)
  DropPreA  hp_ntt_a.hip                           parity level A

(a) whole entry points, x_last = NTT(planted): the oracle's words.  (b) the limb-range stages with the planted rows handed in as the
coefficient rows: the exact model's residues, and the words of (a) where there is no addend; the form that takes any u64 also on words
from q_last up to 2^64 - 1.  (c) the same at parity level A.  Every comparison is exact, and every compared call follows the same
call on another input of the same shape (rows between the two split launches live in the context's workspace).

Not reached: the hybrid key switch's ModDown centring and the second centring of level A's two-drop launch (DropPre2A,
k_ntt_inv_mix_a) -- no entry point takes their coefficient rows.

What the cases notice, tried on libraries built with one line changed (274 cases in this file and test_gpu_base_edges.py):
  c > half for c >= half in k_drop_rem                       105 fail: every rem+fin case of the three drop tests
  ... in the split DROP && FIRST block                        75 fail: every split case
  ... in the eager prologue and DropPre                       81 fail: every eager / DropPre case, and level A (BGV, addend on polynomial 0)
  ... in DropPreA                                              6 fail: the level-A cases
  the SMALL remainder left unreduced (c for c - [c >= q] q)   10 fail: SMALL_MID, eager / DropPre, whole calls and strict stages.
The last one computes the same residues, and on moduli next to a power of two the same WORDS (tests/test_drop_edges.py:
test_where_an_unreduced_small_remainder_shows); only the mid-octave limb of SMALL_MID tells it apart."""
from collections import namedtuple

import numpy as np
import pytest

import drop_edges as DE
import moduli as M
from oracle.pyoracle import SplitMix

# (the shared inputs are read-only arrays: torch remarks on that when it copies them to the device)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
U = np.uint64
T = 65537
SENTINEL = 0x5EED5EED5EED5EED
KNOBS = ("HP_SPLIT_MAX_ITEMS", "HP_NO_FUSED_DROP", "HP_PARITY_LEVEL", "HP_DROP_GROUP", "HP_SPREAD_GROUP", "HP_NO_DOUBLE_DROP")
ROUTE_ENV = {"default": {}, "tiled": {"HP_SPLIT_MAX_ITEMS": "0"}, "unfused": {"HP_NO_FUSED_DROP": "1"}}

WHOLE_LOGNS = (3, 10, 11, 12, 13, 14, 15, 16)
STAGE_LOGNS = WHOLE_LOGNS
LEVEL_A_LOGNS = (11, 13, 15)
# (BGV, add_mask) -> the compiled flavour (hp_ntt_fast.hip / hp_ntt_a.hip have the lists); -1: level A has no kernel, level B's flavour 0 runs
FLAVOUR_B = {(False, 0): 1, (False, 3): 2, (False, 1): 5, (True, 0): 3, (True, 3): 4, (True, 1): 0}
FLAVOUR_A = {(False, 0): 1, (False, 3): 2, (False, 1): 5, (True, 0): 3, (True, 3): 4, (True, 1): -1}
ANY_WORD_CALLS = [(0, 0), (0, 1), (T, 3), (T, 1)]      # (t, add_mask) of the form that takes any u64, over the whole limb range

WHOLE_CASES = [(name, logn, route) for name in DE.LEVEL_B_CHAINS for logn in WHOLE_LOGNS for route in DE.routes(logn)]
STAGE_CASES = [(name, logn, route) for name in DE.LEVEL_B_CHAINS for logn in STAGE_LOGNS for route in DE.routes(logn)]
LEVEL_A_CASES = [(name, logn) for name in DE.LEVEL_A_CHAINS for logn in LEVEL_A_LOGNS]


def whole_copy(logn, route):
    """the copy of the drop a call of at most 128 limbs reaches, written out by hand (tests/test_drop_edges.py holds it to the routing)"""
    if route in ("unfused", "generic") or logn <= 10:
        return "rem/fin"
    if route == "default":
        return "eager" if logn == 11 else "split"
    return {12: "eager", 13: "eager", 14: "eager", 15: "DropPre", 16: "rem/fin"}[logn]


def case_id(name, logn, route):
    return f"{name}-n{logn}-{route}-{whole_copy(logn, route).replace('/', '+')}"


def ranges(L):
    return [(0, L - 1), (0, 1), (1, L - 1)]


Stage = namedtuple("Stage", "chain logn route level k0 k1 t mask strict")


def stage_calls():
    """every call of the limb-range stages this file makes"""
    for name, logn, route in STAGE_CASES:
        L = len(DE.chain_of(name, logn))
        for k0, k1 in ranges(L):
            for t in (0, T):
                for mask in (0, 3, 1):
                    yield Stage(name, logn, route, "B", k0, k1, t, mask, True)
        for t, mask in ANY_WORD_CALLS:
            yield Stage(name, logn, route, "B", 0, L - 1, t, mask, False)
        yield Stage(name, logn, route, "B", 1, L - 1, 0, 0, False)
    for name, logn in LEVEL_A_CASES:
        L = len(DE.chain_of(name, logn))
        for k0, k1 in ranges(L):
            for t in (0, T):
                for mask in (0, 3, 1):
                    yield Stage(name, logn, "default", "A", k0, k1, t, mask, True)


# ---- inputs, the oracle's words and the model's residues: once per (chain, log N), shared by the routes, read-only -------------------
class Case:
    def __init__(self, orc, name, logn):
        self.orc, self.name, self.logn = orc, name, logn
        self.chain = chain = DE.chain_of(name, logn)
        self.n = n = 1 << logn
        self.L = L = len(chain)
        seed = 5000 + 100 * logn + sum(map(ord, name))
        self.planted = DE.coefficient_rows(chain, n, seed)
        self.any_word = DE.coefficient_rows(chain, n, seed + 1, extended=True)
        rng = SplitMix(seed + 2)
        self.x = {0: DE.planted_ct(orc, SplitMix(seed + 3), chain, n, self.planted, 0)}
        for t in DE.PLAIN:                       # the limbs that stay are the same words: only the last limb depends on t
            self.x[t] = DE.planted_ct(orc, SplitMix(seed + 3), chain, n, self.planted, t)
            assert np.array_equal(self.x[t][:, :, :L - 1], self.x[0][:, :, :L - 1])
        self.other = M.lazy_rows(rng, (DE.BATCH, 2, L, n), chain)
        self.addend = M.lazy_rows(rng, (DE.BATCH, 2, L - 1, n), chain[:-1])
        self.other_addend = M.lazy_rows(rng, (DE.BATCH, 2, L - 1, n), chain[:-1])
        self.other_clast = rng.poly((2 * DE.BATCH, 1, n), chain[-1:]).reshape(2 * DE.BATCH, n)
        self._whole, self._base = {}, {}
        for a in (self.planted, self.any_word, self.other, self.addend, self.other_addend, self.other_clast, *self.x.values()):
            a.setflags(write=False)

    def whole(self, t):
        """the oracle's words [B][2][L-1][n] of the rescale (t = 0) / the mod switch"""
        if t not in self._whole:
            f = (lambda ct: self.orc.bgv_mod_drop(self.chain, t, ct)) if t else (lambda ct: self.orc.ckks_rescale(self.chain, ct))
            self._whole[t] = np.stack([f(self.x[t][b]) for b in range(DE.BATCH)])
            self._whole[t].setflags(write=False)
        return self._whole[t]

    def model(self, t, mask, any_word=False):
        """the model's residues [P2][L-1][n] for the planted rows (any_word: the rows with words from q_last on)"""
        key = (t, any_word)
        if key not in self._base:
            rows = self.any_word if any_word else self.planted
            x = self.x[0].reshape(2 * DE.BATCH, self.L, self.n)
            self._base[key] = np.stack([DE.model_drop(self.orc, self.chain, t, x[p2], rows[p2]) for p2 in range(2 * DE.BATCH)])
            self._base[key].setflags(write=False)
        out = self._base[key].copy()
        add = self.addend.reshape(2 * DE.BATCH, self.L - 1, self.n)
        for p2 in range(2 * DE.BATCH):
            if (mask >> (p2 & 1)) & 1:
                out[p2] = DE.canon(out[p2] + add[p2], self.chain[:-1])      # (< 2^59 + 2^60: no wrap)
        return out


_cases = {}


@pytest.fixture
def case(orc):
    def get(name, logn):
        if (name, logn) not in _cases:
            _cases.clear()                       # consecutive tests share a case; the large rings are not kept
            _cases[name, logn] = Case(orc, name, logn)
        return _cases[name, logn]
    return get


@pytest.fixture(scope="module")
def engines():
    """one engine per route, created under its knob (read once at hp_ctx_create); "generic" is the default engine with force_generic"""
    from hehub_amd.engine import Engine

    made = {}

    def get(route):
        key = "default" if route == "generic" else route
        if key not in made:
            with pytest.MonkeyPatch.context() as mp:
                for k in KNOBS:
                    mp.delenv(k, raising=False)
                for k, v in ROUTE_ENV[key].items():
                    mp.setenv(k, v)
                made[key] = Engine(0)
        return made[key]

    yield get
    for e in made.values():
        e.release_workspace()
        e.close()


class routed:
    """the engine of a route, at a parity level, for the duration of one test"""

    def __init__(self, engines, route, level="B"):
        self.eng, self.route, self.level = engines(route), route, level

    def __enter__(self):
        self.eng.force_generic(self.route == "generic")
        self.eng.set_parity_level(self.level)
        return self.eng

    def __exit__(self, *exc):
        self.eng.force_generic(False)
        self.eng.set_parity_level("B")


def run_whole(eng, c, t, other_first=True):
    call = (lambda d: eng.bgv_mod_switch(c.chain, t, d)) if t else (lambda d: eng.ckks_rescale(c.chain, d))
    if other_first:
        call(eng.to_device(c.other))
    return eng.to_host(call(eng.to_device(c.x[t])))


# ---- (a) whole entry points ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,logn,route", WHOLE_CASES, ids=[case_id(*c) for c in WHOLE_CASES])
def test_rescale_and_mod_switch_on_planted_coefficients(case, engines, name, logn, route):
    c = case(name, logn)
    with routed(engines, route) as eng:
        # the launches of the call: the unfused kernels where the id says so, one of the fused forms elsewhere
        eng.prof_begin("*")
        eng.ckks_rescale(c.chain, eng.to_device(c.other))
        fams = eng.prof_end_families()
        assert ("drop_rem" in fams and "drop_fin" in fams) == (whole_copy(logn, route) == "rem/fin"), fams
        assert ("ntt_drop" in fams) == (whole_copy(logn, route) != "rem/fin"), fams
        for t in (0,) + DE.PLAIN:
            got = run_whole(eng, c, t, other_first=t != 0)
            assert np.array_equal(got, c.whole(t)), (name, logn, route, t)


# ---- (b) the limb-range stages -----------------------------------------------------------------------------------------------------------
def run_stage(eng, c, rows, other_rows, t, mask, k0, k1, strict, out):
    """the stage on the planted rows after the same call on other rows; limbs outside [k0, k1) must keep the sentinel"""
    dev = eng.to_device
    add, other_add = (dev(c.addend), dev(c.other_addend)) if mask else (None, None)
    eng.drop_apply_range(c.chain, t, dev(c.other), dev(other_rows), k0, k1, other_add, mask, strict, out)
    out.fill_(SENTINEL)
    eng.drop_apply_range(c.chain, t, dev(c.x[0]), dev(rows), k0, k1, add, mask, strict, out)
    got = eng.to_host(out)
    kept = np.ones(c.L - 1, dtype=bool)
    kept[k0:k1] = False
    assert (got[:, kept] == U(SENTINEL)).all(), "a limb outside the range was written"
    return got[:, k0:k1]


def check_strict_stages(eng, c, level):
    q = c.chain[:-1]
    out = eng.empty((2 * DE.BATCH, c.L - 1, c.n))
    for k0, k1 in ranges(c.L):
        for t in (0, T):
            for mask in (0, 3, 1):
                got = run_stage(eng, c, c.planted, c.other_clast, t, mask, k0, k1, True, out)
                where = (c.name, c.logn, level, k0, k1, t, mask)
                assert np.array_equal(DE.canon(got, q[k0:k1]), c.model(t, mask)[:, k0:k1]), where
                if level == "A" and FLAVOUR_A[(t != 0, mask)] > 0:
                    assert (got < np.array(q[k0:k1], dtype=U)[:, None]).all(), where          # canonical residues
                if mask == 0:        # the words of (a): the oracle's at level B, their residues at level A
                    words = c.whole(t).reshape(2 * DE.BATCH, c.L - 1, c.n)[:, k0:k1]
                    assert np.array_equal(got, words if level == "B" else DE.canon(words, q[k0:k1])), where


@pytest.mark.parametrize("name,logn,route", STAGE_CASES, ids=[case_id(*c) + "-strict" for c in STAGE_CASES])
def test_strict_stage_on_planted_coefficients(case, engines, name, logn, route):
    c = case(name, logn)
    with routed(engines, route) as eng:
        check_strict_stages(eng, c, "B")


@pytest.mark.parametrize("name,logn,route", STAGE_CASES, ids=[case_id(*c) + "-any" for c in STAGE_CASES])
def test_stage_that_takes_any_word(case, engines, name, logn, route):
    """hp_dev_drop_apply_range: right for any u64 -- the planted rows also hold q_last, q_last + 1, 2 q_last - 1, 2^63 and 2^64 - 1"""
    c = case(name, logn)
    q = c.chain[:-1]
    with routed(engines, route) as eng:
        out = eng.empty((2 * DE.BATCH, c.L - 1, c.n))
        other_rows = np.ascontiguousarray(c.any_word[::-1])
        for (t, mask), (k0, k1) in [(tm, (0, c.L - 1)) for tm in ANY_WORD_CALLS] + [((0, 0), (1, c.L - 1))]:
            got = run_stage(eng, c, c.any_word, other_rows, t, mask, k0, k1, False, out)
            assert np.array_equal(DE.canon(got, q[k0:k1]), c.model(t, mask, any_word=True)[:, k0:k1]), (name, logn, route, t, mask, k0, k1)


# ---- (c) parity level A --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,logn", LEVEL_A_CASES, ids=[f"{n}-n{l}-DropPreA" for n, l in LEVEL_A_CASES])
def test_level_a_on_planted_coefficients(case, engines, name, logn):
    """canonical residues of the oracle's words; BGV with an addend on polynomial 0 alone has no level-A kernel and runs level B's
    flavour 0 under the level-A context (its residues are compared)"""
    c = case(name, logn)
    q = c.chain[:-1]
    with routed(engines, "default", "A") as eng:
        assert eng.parity_level() == "A"
        for t in (0,) + DE.PLAIN:
            assert np.array_equal(run_whole(eng, c, t), DE.canon(c.whole(t), q)), (name, logn, t)
        check_strict_stages(eng, c, "A")
