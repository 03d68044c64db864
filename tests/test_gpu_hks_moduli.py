"""hp_dev_ckks_rotate_hoisted_hks, hp_dev_ckks_lintrans_hks and hp_dev_ckks_lintrans_bsgs_hks on wide and off-table moduli: the chains of
tests/moduli.py cut to (L, k) and WIDE58 (tests/hks_edges.py: every modulus 58 or 59 bits, the 58-bit high_mid prime among them), where
  * the carry out of the middle carry-save column of hp_mac2 (hp_device.h: cx) fires, which no 40- / 50-bit table chain can make it do;
  * the 128-bit sums of k_hks_inner_lintrans and k_hks_bsgs_presum come within 2.5 bits of wrapping (tests/test_hks_edges.py has the
    figures, computed with Python integers, and asserts the registers' conditions without a GPU);
  * the fix = 1 fold, the per-limb pack-48 decision and the level-A eligibility decision switch.
The models are those of the three calls' own tests (tests/hks_model.py): Python integers around the oracle's primitives.
What these cases found: at a high_mid ciphertext modulus the lazy transform of ModDown's remainder has words of 2q and more, on which
hehub's lazy subtraction wraps -- the residues then depended on which representative the accumulator word happened to be, and the
three calls disagreed with each other on those limbs (case 6, which needs no model) and with plain integer arithmetic.  The ModDown kernels and
the model now bring the remainder's words below 2q first (hp_lazy_below_2q, hp_device.h; hks_model.below_2q), which changes no word
where they already were; tests/test_hks_edges.py holds the model's ModDown to plain integer arithmetic at such moduli.
  (1) the exact model on every chain: hoisted word for word at level B, the two transforms on residues with every word below 2q;
  (2) extremal rows: every (polynomial, limb) row of ciphertext, keys and diagonals one of moduli.INPUT_KINDS, and everything 2q - 1;
  (3) the accumulator edge: 16 digits, 32 rotations / babies on WIDE58, at N = 32 and N = 1024;
  (4) N = 512 (one HKS_LT_CHUNK) and N = 1024 (two; the last degree of the generic transforms);
  (5) level A follows eligibility;  (6) the three calls against each other."""
import numpy as np
import pytest

import hks_edges as H
import moduli as M
from hks_model import dev, flat_case, model_bsgs, model_hoisted, model_lintrans, residues_match, single_case, step0_case
from test_gpu_moduli import LEVEL_A_CHAINS

pytestmark = pytest.mark.gpu
U = np.uint64


@pytest.fixture(scope="module")
def eng():
    from hehub_amd.engine import Engine

    e = Engine(0)
    yield e
    e.release_workspace()
    e.close()


def seed_of(name, logn, L):
    return 9000 + 100 * (sorted(M.CHAINS).index(name) if name in M.CHAINS else 40) + 7 * logn + L


# ---- running a case of hks_edges on the device, and its model ----------------------------------------------------------------------
def run_hoisted(eng, c):
    dk = dev(eng, c["kpool"])
    return eng.to_host(eng.ckks_rotate_hoisted_hks(c["mext"], c["k"], c["alpha"], eng.to_device(c["ct"]), H.pick(dk, c["which"]), c["steps"],
                                                   c["conj"]))


def run_flat(eng, c):
    dk, dd = dev(eng, c["kpool"]), dev(eng, c["dpool"])
    return eng.to_host(eng.ckks_lintrans_hks(c["mext"], c["k"], c["alpha"], eng.to_device(c["ct"]), H.pick(dk, c["which"]), c["steps"],
                                             H.pick(dd, c["wd"]), c["conj"]))


def run_bsgs(eng, c):
    dk, dd = dev(eng, c["kpool"]), dev(eng, c["dpool"])
    return eng.to_host(eng.ckks_lintrans_bsgs_hks(c["mext"], c["k"], c["alpha"], eng.to_device(c["ct"]), H.pick(dk, c["bwhich"]), c["bsteps"],
                                                  H.pick(dk, c["gwhich"]), c["gsteps"], [H.pick(dd, row) for row in c["wd"]], c["bconj"],
                                                  c["gconj"]))


def hoisted_is_the_model(orc, c, got):
    B, R = c["ct"].shape[0], len(c["steps"])
    assert got.shape == (B, R, 2, c["L"], 1 << c["logn"])
    for b in range(B):
        exp = model_hoisted(orc, c["logn"], c["mext"], c["L"], c["k"], c["alpha"], c["ct"][b], H.pick(c["kpool"], c["which"]), c["steps"], c["conj"])
        for r in range(R):
            assert np.array_equal(got[b, r], exp[r]), (b, r, c["steps"][r], c["conj"][r], np.argwhere(got[b, r] != exp[r])[:3].tolist())


def flat_is_the_model(orc, c, got):
    q = c["mext"][:c["L"]]
    for b in range(c["ct"].shape[0]):
        exp = model_lintrans(orc, c["logn"], c["mext"], c["L"], c["k"], c["alpha"], c["ct"][b], H.pick(c["kpool"], c["which"]), c["steps"], c["conj"],
                             H.pick(c["dpool"], c["wd"]))
        assert residues_match(got[b], exp, q), (b, mismatches(got[b], exp, q))


def bsgs_is_the_model(orc, c, got):
    q = c["mext"][:c["L"]]
    for b in range(c["ct"].shape[0]):
        exp = model_bsgs(orc, c["logn"], c["mext"], c["L"], c["k"], c["alpha"], c["ct"][b], H.pick(c["kpool"], c["bwhich"]), c["bsteps"], c["bconj"],
                         H.pick(c["kpool"], c["gwhich"]), c["gsteps"], c["gconj"], [H.pick(c["dpool"], row) for row in c["wd"]])
        assert residues_match(got[b], exp, q), (b, mismatches(got[b], exp, q))


def mismatches(got, exp, q):
    """for the failure message: how many residues differ on each (polynomial, limb) row, and the first three places with both words"""
    qa = np.array(q, dtype=U)[None, :, None]
    bad = (got % qa).astype(object) != exp
    where = np.argwhere(bad)[:3].tolist()
    return bad.sum(axis=2).tolist(), [(w, int(got[tuple(w)]), int(exp[tuple(w)])) for w in where]


# ---- (1) the exact model on every chain ----------------------------------------------------------------------------------------------
MODEL_CASES = [(name,) + shape for name in H.MODEL_CHAINS for shape in H.MODEL_SHAPES]


@pytest.mark.parametrize("name,logn,L,k,alpha", MODEL_CASES)
def test_hoisted_matches_the_exact_model(eng, orc, name, logn, L, k, alpha):
    c = H.flat_inputs(name, logn, L, k, alpha, 2, 3, "lazy", seed_of(name, logn, L))
    hoisted_is_the_model(orc, c, run_hoisted(eng, c))


@pytest.mark.parametrize("name,logn,L,k,alpha", MODEL_CASES)
def test_lintrans_matches_the_exact_model(eng, orc, name, logn, L, k, alpha):
    c = H.flat_inputs(name, logn, L, k, alpha, 2, 3, "lazy", seed_of(name, logn, L) + 1)
    flat_is_the_model(orc, c, run_flat(eng, c))


@pytest.mark.parametrize("name,logn,L,k,alpha", MODEL_CASES)
def test_bsgs_matches_the_exact_model(eng, orc, name, logn, L, k, alpha):
    """3 babies x 3 giants, one identity each, one diagonal absent"""
    c = H.bsgs_inputs(name, logn, L, k, alpha, 2, 3, 3, "lazy", seed_of(name, logn, L) + 2)
    assert c["bwhich"][0] is None and c["gwhich"][0] is None and sum(i is None for row in c["wd"] for i in row) == 1
    bsgs_is_the_model(orc, c, run_bsgs(eng, c))


# ---- (2) extremal rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["hoisted", "lintrans", "bsgs"])
@pytest.mark.parametrize("name", H.EXTREMAL_CHAINS)
def test_rows_of_every_input_kind(eng, orc, name, call):
    """strict, lazy, all 2q - 1, and 2q - 1 / 0 alternating, cycled over the rows of the ciphertexts, the keys and the diagonals"""
    logn, L, k, alpha = H.EXTREMAL_SHAPE
    if call == "bsgs":
        c = H.bsgs_inputs(name, logn, L, k, alpha, 2, 3, 3, "kinds", 8200)
        bsgs_is_the_model(orc, c, run_bsgs(eng, c))
    else:
        c = H.flat_inputs(name, logn, L, k, alpha, 2, 3, "kinds", 8200)
        if call == "hoisted":
            hoisted_is_the_model(orc, c, run_hoisted(eng, c))
        else:
            flat_is_the_model(orc, c, run_flat(eng, c))


@pytest.mark.parametrize("name", H.EXTREMAL_CHAINS)
def test_everything_at_its_largest_word(eng, orc, name):
    """every word of the ciphertext, the keys and the diagonals 2q - 1, one digit (alpha = L: the digit rows of the ciphertext moduli are
    the caller's words, the digit sum there (2q - 1)^2), the full table: 32 rotations of the flat call, 32 babies x 2 giants"""
    c = H.all_max_flat(name)
    assert len(c["steps"]) == H.TABLE and all((x == 2 * np.array(c["mext"], dtype=U)[:, None] - U(1)).all() for x in c["dpool"])
    flat_is_the_model(orc, c, run_flat(eng, c))
    c = H.all_max_bsgs(name)
    assert len(c["bsteps"]) == H.TABLE and len(c["gsteps"]) == 2
    bsgs_is_the_model(orc, c, run_bsgs(eng, c))


# ---- (3) the accumulator edge ----------------------------------------------------------------------------------------------------------
SPREAD = 13      # at N = 1024 every 13th coefficient and the last one: 80 of the 1024 coefficients of every row


@pytest.mark.parametrize("logn,fill", H.EDGE_CASES)
def test_lintrans_at_the_accumulator_edge(eng, orc, logn, fill):
    """WIDE58, alpha = 1, 16 digits, 32 rotations.  tests/test_hks_edges.py::test_accumulator_edge_fits has this case's sums: digit sum
    up to 2^123.97, outer sum up to 2^125.50 of the 2^128 (the host's premise: 2^126.32), lifted digit words up to 4.24 q at N = 1024.
    N = 32: every coefficient against model_lintrans.  N = 1024: 80 of 1024 coefficients of every row (hks_edges.sampled_lintrans: the same
    arithmetic, the ciphertext moduli's rows only where compared), every word of every row held below 2q."""
    c = H.edge_flat(logn, fill)
    got = run_flat(eng, c)
    if logn <= 6:
        return flat_is_the_model(orc, c, got)
    n, q = 1 << logn, c["mext"][:c["L"]]
    sel = np.unique(np.r_[np.arange(0, n, SPREAD), n - 1])
    assert len(sel) >= 64
    exp = H.sampled_lintrans(orc, logn, c["mext"], c["L"], c["k"], c["alpha"], c["ct"][0], H.pick(c["kpool"], c["which"]), c["steps"], c["conj"],
                             H.pick(c["dpool"], c["wd"]), sel)
    qa = np.array(q, dtype=U)[None, :, None]
    assert (got[0] < 2 * qa).all()
    assert residues_match(got[0][:, :, sel], exp, q), mismatches(got[0][:, :, sel], exp, q)


@pytest.mark.parametrize("logn,fill", H.EDGE_CASES)
def test_bsgs_at_the_accumulator_edge(eng, orc, logn, fill):
    """32 babies over 16 digits, two giants.  N = 32: one giant keyed, every coefficient against model_bsgs.  N = 1024: both giants the
    identity, which makes the call a flat sum over 2 x 32 terms that the sampled model can follow; 80 of 1024 coefficients of every row."""
    c = H.edge_bsgs(logn, fill)
    got = run_bsgs(eng, c)
    if logn <= 6:
        return bsgs_is_the_model(orc, c, got)
    n, q = 1 << logn, c["mext"][:c["L"]]
    sel = np.unique(np.r_[np.arange(0, n, SPREAD), n - 1])
    assert len(sel) >= 64 and all(w is None for w in c["gwhich"])
    ng = len(c["gsteps"])
    diags = [("absent" if i is None else c["dpool"][i]) for row in c["wd"] for i in row]
    exp = H.sampled_lintrans(orc, logn, c["mext"], c["L"], c["k"], c["alpha"], c["ct"][0], H.pick(c["kpool"], c["bwhich"]) * ng, c["bsteps"] * ng,
                             c["bconj"] * ng, diags, sel)
    qa = np.array(q, dtype=U)[None, :, None]
    assert (got[0] < 2 * qa).all()
    assert residues_match(got[0][:, :, sel], exp, q), mismatches(got[0][:, :, sel], exp, q)


# ---- (4) chunk boundaries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", H.CHUNK_LOGNS)
def test_lintrans_at_one_and_two_chunks(eng, orc, logn):
    c = H.flat_inputs("W59", logn, 3, 2, 2, 2, 3, "lazy", 8600 + logn)
    flat_is_the_model(orc, c, run_flat(eng, c))


@pytest.mark.parametrize("logn", H.CHUNK_LOGNS)
def test_bsgs_at_one_and_two_chunks(eng, orc, logn):
    c = H.bsgs_inputs("W59", logn, 3, 2, 2, 2, 2, 2, "lazy", 8700 + logn)
    bsgs_is_the_model(orc, c, run_bsgs(eng, c))


def test_hoisted_at_the_last_generic_degree(eng, orc):
    c = H.flat_inputs("W59", 10, 3, 2, 2, 2, 3, "lazy", 8800)
    hoisted_is_the_model(orc, c, run_hoisted(eng, c))


# ---- (5) level A follows eligibility -----------------------------------------------------------------------------------------------------------
def three_calls(eng, cf, cb):
    return run_hoisted(eng, cf), run_flat(eng, cf), run_bsgs(eng, cb)


def level_a_inputs(mext, logn, L, k, alpha):
    """a flat and a BSGS case (3 x 3) over the chain mext"""
    return (H.flat_inputs(None, logn, L, k, alpha, 2, 3, "lazy", 8900 + logn + L, mext=mext),
            H.bsgs_inputs(None, logn, L, k, alpha, 2, 3, 3, "lazy", 8950 + logn + L, mext=mext))


@pytest.mark.parametrize("name", sorted(H.LEVEL_A_SHAPES))
def test_level_a_gives_the_residues_of_level_b_where_the_chain_is_eligible(eng, name):
    logn, (L, k, alpha) = 11, H.LEVEL_A_SHAPES[name]
    cf, cb = level_a_inputs(LEVEL_A_CHAINS[name][:L] + LEVEL_A_CHAINS[name][-k:], logn, L, k, alpha)
    assert M.level_a_chain(cf["mext"], logn)
    b_words = three_calls(eng, cf, cb)
    eng.set_parity_level("A")
    try:
        a_words = three_calls(eng, cf, cb)
        eng.sync()   # (HP_ERANGE here: a level-A kernel was handed a word outside its range)
    finally:
        eng.set_parity_level("B")
    qa = np.array(cf["mext"][:L], dtype=U)[:, None]
    for a, b in zip(a_words, b_words):
        assert (a < 2 * qa).all() and (b < 2 * qa).all()
        assert np.array_equal(a % qa, b % qa)


@pytest.mark.parametrize("name", sorted(H.LEVEL_B_ONLY_SHAPES))
def test_a_level_a_context_keeps_level_b_where_the_chain_is_not_eligible(eng, name):
    logn, (L, k, alpha) = 12, H.LEVEL_B_ONLY_SHAPES[name]
    cf, cb = level_a_inputs(H.cut(name, L, k), logn, L, k, alpha)
    assert not M.level_a_chain(cf["mext"], logn)
    b_words = three_calls(eng, cf, cb)
    eng.set_parity_level("A")
    try:
        a_words = three_calls(eng, cf, cb)
        eng.sync()
    finally:
        eng.set_parity_level("B")
    qa = np.array(cf["mext"][:L], dtype=U)[:, None]
    assert np.array_equal(a_words[0], b_words[0])                      # hoisted: the level-B words themselves
    for a, b in zip(a_words[1:], b_words[1:]):
        assert np.array_equal(a % qa, b % qa)


# ---- (6) the calls against each other ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.CROSS_CHAINS)
def test_the_three_calls_agree_where_they_must(eng, name):
    logn, L, k, alpha = 11, 3, 2, 2
    mext = H.chain_of(name, L, k)
    hoisted, lin, lazy = single_case(eng, logn, L, k, alpha, mext=mext)
    assert lazy and np.array_equal(hoisted, lin)                       # one rotation without a diagonal is the hoisted rotation
    flat, bsgs, lazy = flat_case(eng, logn, L, k, alpha, mext=mext)
    assert lazy and np.array_equal(flat, bsgs)                         # one identity giant is the flat call
    plain, hoisted = step0_case(eng, logn, L, k, alpha, mext=mext)
    assert np.array_equal(plain, hoisted)                              # hoisted step 0 is the unhoisted rotation (one switch plus c0)
