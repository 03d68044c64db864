// hp_api_eval.cpp -- C ABI, part 3 (extension): linear combinations of ciphertexts read at their own levels (kernel: hp_lincomb.hip)
// and the straight-line evaluator built over them and the hybrid calls -- the non-linear half of a CKKS program (a polynomial
// approximation of a sigmoid, a comparison, EvalMod) as a sequence of steps of ONE kind,
//     E_{s+1} = rescale( relin( sum_t X_t (x) Y_t ) + Z ),      X_t, Y_t, Z linear forms over earlier elements,
// whose recombination sum_g leaf_g (x) G_g pays ONE key switch (lazy relinearisation: hp_api_hks_mult.cpp).  The engine is exact integer
// arithmetic: which steps, which constants and what they mean as scales is the caller's business (hehub_amd/polyeval.py builds
// plans for the power and the Chebyshev basis).
#include "hp_hks_call.h"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace hpi;

namespace {

// a linear form as its launches see it: term j = coef[j] * the batch src[j] of limbs[j] limbs per polynomial (coef NULL: 1), + cst
struct Form {
    std::vector<const u64 *> src;
    std::vector<size_t> limbs;
    std::vector<const uint64_t *> coef;
    const uint64_t *cst = nullptr;
    size_t terms() const { return src.size(); }
    bool empty() const { return src.empty() && !cst; }
};

// `pass` terms per launch (lincomb_max_terms' answer); a form without terms is one launch of its constant
size_t form_launches(size_t terms, size_t pass) { return terms ? (terms + pass - 1) / pass : 1; }
// the device words of a form's coefficient blocks: one u64[cnt + 1][L] per launch
size_t form_coef_words(size_t terms, size_t pass, size_t L) { return (terms + form_launches(terms, pass)) * L; }

void form_coefs(const Form &f, size_t L, size_t pass, std::vector<u64> &host) {
    size_t t0 = 0;
    do {
        const size_t cnt = std::min(pass, f.terms() - t0);
        for (size_t j = t0; j < t0 + cnt; j++)
            for (size_t m = 0; m < L; m++) host.push_back(f.coef[j] ? f.coef[j][m] : 1);
        for (size_t m = 0; m < L; m++) host.push_back(t0 == 0 && f.cst ? f.cst[m] : 0);   // the constant goes in once
        t0 += cnt;
    } while (t0 < f.terms());
}

// out [batch][out_polys][L][N] (polynomials 0, 1) = [accumulate: out +] the form, over the blocks form_coefs wrote at d_coef
int form_launch(hp_ctx *ctx, const HpLimb *limbs, size_t L, size_t n, size_t batch, size_t pass, const Form &f, const u64 *d_coef,
                bool accumulate, u64 *out, u32 out_polys) {
    size_t t0 = 0;
    do {
        HpLincombTable tab;
        memset(&tab, 0, sizeof(tab));
        tab.terms = (u32)std::min(pass, f.terms() - t0);
        for (u32 j = 0; j < tab.terms; j++) {
            tab.src[j] = f.src[t0 + j];
            tab.limbs[j] = (u32)f.limbs[t0 + j];
        }
        ProfScope ps(ctx, "elem");
        int rc = chk(ctx, hp_launch_ct_lincomb(limbs, (u32)L, (u32)n, (u32)batch, tab, d_coef, accumulate || t0 != 0, out, out_polys,
                                               ctx->stream), "ct_lincomb");
        if (rc) return rc;
        d_coef += ((size_t)tab.terms + 1) * L;
        t0 += tab.terms;
    } while (t0 < f.terms());
    return HP_OK;
}

bool residues_ok(const uint64_t *v, const uint64_t *moduli, size_t L) {
    for (size_t m = 0; v && m < L; m++)
        if (v[m] >= moduli[m]) return false;
    return true;
}

// rows of one launch stay u32 and its workgroups below 2^31 (512 words per workgroup at the least)
bool batch_fits(size_t batch, size_t L, size_t n) { return batch <= ((size_t)1 << 29) / (L * ((n + 511) / 512)); }

} // namespace

extern "C" int hp_dev_ckks_lincomb(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch, size_t terms,
                                   const uint64_t *const *d_cts, const size_t *ct_limbs, const uint64_t *const *coefs, const uint64_t *cst,
                                   uint64_t *d_out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli, d_cts, ct_limbs, d_out);
    HP_ALIGNED(ctx, d_out);
    if (!logn_ok(logn)) return fail(ctx, HP_EUNSUPPORTED, HP_LOGN_MSG);
    if (L < 1 || L > HP_MAX_LIMBS) return fail(ctx, HP_EINVAL, "unsupported number of moduli");
    if (batch == 0) return fail(ctx, HP_EINVAL, "empty batch");
    if (terms == 0) return fail(ctx, HP_EINVAL, "lincomb: no terms");
    const size_t n = (size_t)1 << logn, out_bytes = batch * 2 * L * n * 8;
    if (!batch_fits(batch, L, n)) return fail(ctx, HP_EUNSUPPORTED, "lincomb: too many ciphertexts for one call");
    return contained(ctx, [&] {
        Form f;
        for (size_t t = 0; t < terms; t++) {
            const uint64_t *p = d_cts[t];
            if (!p || ((uintptr_t)p & 15u)) return fail(ctx, HP_EINVAL, "lincomb: NULL or misaligned operand");
            if (ct_limbs[t] < L || ct_limbs[t] > HP_MAX_LIMBS) return fail(ctx, HP_EINVAL, "lincomb: an operand with fewer limbs than L (or more than 32)");
            if (ranges_overlap(p, batch * 2 * ct_limbs[t] * n * 8, d_out, out_bytes))
                return fail(ctx, HP_EINVAL, "lincomb: the output overlaps an operand");
            if (coefs && !residues_ok(coefs[t], moduli, L)) return fail(ctx, HP_EINVAL, "lincomb: a coefficient residue is not below its modulus");
            f.src.push_back(p);
            f.limbs.push_back(ct_limbs[t]);
            f.coef.push_back(coefs ? coefs[t] : nullptr);
        }
        if (!residues_ok(cst, moduli, L)) return fail(ctx, HP_EINVAL, "lincomb: a constant residue is not below its modulus");
        f.cst = cst;
        const size_t pass = lincomb_max_terms(moduli, L, HP_LINCOMB_MAX);
        if (pass == 0) return fail(ctx, HP_EUNSUPPORTED, "lincomb: moduli too large for the 128-bit accumulators");
        const Plan *plan;
        int rc = get_plan(ctx, 0, moduli, L, false, &plan);
        if (rc) return rc;
        std::vector<u64> host;
        form_coefs(f, L, pass, host);
        if ((rc = ws_reserve(ctx, padded(host.size())))) return rc;
        u64 *d_coef = (u64 *)ctx->ws;
        if ((rc = stage_upload(ctx, host.data(), host.size() * 8, d_coef))) return rc;
        return form_launch(ctx, plan->d_limbs, L, n, batch, pass, f, d_coef, false, d_out, 2);
    });
}

// ---- the evaluator -------------------------------------------------------------------------------------------------------------------
// Workspace, reserved once before anything is enqueued (pad = rounded up to 256 bytes; level_s, products_s of step s; B = batch):
//   coefficient blocks   sum over every form of (terms + launches) * level words
//   elements             sum_s pad(B 2 (level_s - 1) N)           every element stays live (the last one is d_out when final_drops == 0)
//   final drops          2 pad(B 2 (out_limbs' - 1) N)            out_limbs' = level_last - 1; only with final_drops >= 2
//   scratch              max over the steps of
//                          products > 0:  materialised forms * pad(B 2 level N) + pad(B 3 level N) + the workspace of
//                                         hp_dev_ckks_relin_rescale_hks_at at that level
//                          products == 0: pad(B 2 level N) + the workspace of hp_dev_ckks_rescale at that level
//                        and of the final drops' hp_dev_ckks_rescale
namespace {

struct EvalStep {
    size_t level = 0;
    std::vector<Form> x, y;
    Form z;
    std::vector<u64> mext;   // q_0 .. q_{level-1}, p_0 .. p_{k-1}
    size_t pass_lin = 0, pass_ts = 0;
    size_t coef_at = 0;      // where the step's coefficient blocks begin (x_0, y_0, x_1, ..., z; pass-through forms have none)
};

// a form that is one earlier element as it lies: passed by address, no copy
bool pass_through(const Form &f, size_t level) { return f.terms() == 1 && !f.coef[0] && !f.cst && f.limbs[0] == level; }

} // namespace

extern "C" int hp_dev_ckks_eval_plan_hks(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                         size_t batch, size_t steps, const hp_eval_step *plan, size_t final_drops, const uint64_t *d_ct,
                                         const uint64_t *d_relin_key, uint64_t *d_out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, plan, d_ct, d_relin_key, d_out);
    HP_ALIGNED(ctx, d_ct, d_relin_key, d_out);
    if (!logn_ok(logn)) return fail(ctx, HP_EUNSUPPORTED, HP_LOGN_MSG);
    if (L < 1 || k < 1 || L + k > HP_MAX_LIMBS) return fail(ctx, HP_EINVAL, "unsupported number of moduli");
    if (batch == 0) return fail(ctx, HP_EINVAL, "empty batch");
    // what every hybrid call refuses on the shape alone, whether or not a step of the plan switches
    if (int lim = HksCall(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, 0).rc) return lim;
    if (steps == 0 || steps > 64) return fail(ctx, HP_EINVAL, "eval_plan: 1 .. 64 steps");
    const size_t n = (size_t)1 << logn;
    if (!batch_fits(batch, L, n)) return fail(ctx, HP_EUNSUPPORTED, "eval_plan: too many ciphertexts for one call");
    const auto bad = [&](const char *what) { return fail(ctx, HP_EINVAL, std::string("eval_plan: ") + what); };
    return contained(ctx, [&] {
        // ---- everything that is refused, before anything is enqueued ----
        std::vector<size_t> limbs(steps + 1);   // limb count of every element
        std::vector<EvalStep> st(steps);
        limbs[0] = L;
        // a form of step s with its elements' addresses still open (src filled in once the workspace is carved): elem index in `el`
        std::vector<std::vector<size_t>> el;
        const auto read_form = [&](const hp_eval_form &in, size_t s, size_t level, bool needs_term, Form &f) -> int {
            if (needs_term && in.terms == 0) return bad("a product form without a term");
            if (in.terms && !in.term) return bad("a NULL term list");
            el.emplace_back();
            for (size_t j = 0; j < in.terms; j++) {
                const hp_eval_term &t = in.term[j];
                if (t.elem > s) return bad("a reference to an element that is not computed yet");
                if (limbs[t.elem] < level) return bad("a step's level is above an operand's limb count");
                if (!residues_ok(t.coef, moduli_ext, level)) return bad("a coefficient residue is not below its modulus");
                f.src.push_back(nullptr);
                f.limbs.push_back(limbs[t.elem]);
                f.coef.push_back(t.coef);
                el.back().push_back(t.elem);
            }
            if (!residues_ok(in.cst, moduli_ext, level)) return bad("a constant residue is not below its modulus");
            f.cst = in.cst;
            return HP_OK;
        };
        int rc;
        for (size_t s = 0; s < steps; s++) {
            const hp_eval_step &in = plan[s];
            EvalStep &e = st[s];
            e.level = in.level;
            if (in.level < 2) return bad("a step needs a level of at least 2");
            if (in.level > L) return bad("a step's level is above an operand's limb count");
            if (in.products && (!in.x || !in.y)) return bad("a NULL form list");
            e.x.resize(in.products);
            e.y.resize(in.products);
            for (size_t t = 0; t < in.products; t++)
                if ((rc = read_form(in.x[t], s, in.level, true, e.x[t])) || (rc = read_form(in.y[t], s, in.level, true, e.y[t]))) return rc;
            if ((rc = read_form(in.z, s, in.level, false, e.z))) return rc;
            if (in.products == 0 && e.z.terms() == 0) return bad("a step without a product and without a term");
            limbs[s + 1] = in.level - 1;
        }
        if (final_drops >= limbs[steps]) return bad("the final drops leave no limb");
        const size_t out_limbs = limbs[steps] - final_drops;
        if (ranges_overlap(d_ct, batch * 2 * L * n * 8, d_out, batch * 2 * out_limbs * n * 8)) return bad("the output overlaps the input");
        // the levels' own refusals (the _at calls', with their code), the range of the sums, and the sizes
        size_t coef_words = 0, scratch = 0, elem_words = 0;
        for (size_t s = 0; s < steps; s++) {
            EvalStep &e = st[s];
            const size_t lv = e.level;
            e.mext.assign(moduli_ext, moduli_ext + lv);
            e.mext.insert(e.mext.end(), moduli_ext + L, moduli_ext + L + k);
            e.pass_lin = lincomb_max_terms(moduli_ext, lv, HP_LINCOMB_MAX);
            e.pass_ts = tensor_sum_max_terms(moduli_ext, lv, HP_TENSOR_SUM_MAX);
            if (e.pass_lin == 0 || e.pass_ts == 0) return fail(ctx, HP_EUNSUPPORTED, "eval_plan: moduli too large for the 128-bit accumulators");
            e.coef_at = coef_words;
            const Plan *limbs_plan;   // (the run loop fetches it again: then a hit in the cache, nothing that can fail half-way)
            if ((rc = get_plan(ctx, 0, moduli_ext, lv, false, &limbs_plan))) return rc;
            size_t mat = 0, need;
            for (size_t t = 0; t < e.x.size(); t++)
                for (const Form *f : {&e.x[t], &e.y[t]})
                    if (!pass_through(*f, lv)) mat++, coef_words += form_coef_words(f->terms(), e.pass_lin, lv);
            if (!e.z.empty()) coef_words += form_coef_words(e.z.terms(), e.pass_lin, lv);
            if (!e.x.empty()) {
                HksCall c(ctx, logn, lv, key_L0, k, alpha, e.mext.data(), batch, 0);   // (scoped: its level ends with this block)
                if (c.rc) return c.rc;
                if (lv < 2) return fail(ctx, HP_EINVAL, "Unable to drop the only one prime.");
                if (c.open()) return c.rc;
                need = mat * (padded(batch * 2 * lv * n) / 8) + padded(batch * 3 * lv * n) / 8 + relin_rescale_words(c, batch);
            } else {
                const Plan *p;
                if ((rc = get_plan(ctx, logn, moduli_ext, lv, true, &p))) return rc;
                need = padded(batch * 2 * lv * n) / 8 + drop_ws_words(n, lv, 2 * batch);
            }
            scratch = std::max(scratch, need);
            if (s + 1 < steps || final_drops) elem_words += padded(batch * 2 * (lv - 1) * n) / 8;
        }
        const size_t last = limbs[steps], half = final_drops >= 2 ? padded(batch * 2 * (last - 1) * n) / 8 : 0;
        for (size_t d = 0; d < final_drops; d++) {
            const Plan *p;
            if ((rc = get_plan(ctx, logn, moduli_ext, last - d, true, &p))) return rc;
            scratch = std::max(scratch, drop_ws_words(n, last - d, 2 * batch));
        }
        const size_t coef_pad = padded(coef_words) / 8;
        if ((rc = ws_reserve(ctx, (coef_pad + elem_words + 2 * half + scratch) * 8))) return rc;

        // ---- carve, upload the constants, run ----
        Carver top(ctx->ws);
        u64 *d_coef = top.take(coef_words);
        std::vector<const u64 *> elem(steps + 1);
        std::vector<u64 *> dst(steps);
        elem[0] = d_ct;
        for (size_t s = 0; s < steps; s++) {
            dst[s] = (s + 1 < steps || final_drops) ? top.take(batch * 2 * (st[s].level - 1) * n) : d_out;
            elem[s + 1] = dst[s];
        }
        u64 *tmp[2] = {nullptr, nullptr};
        if (half) tmp[0] = top.take(half), tmp[1] = top.take(half);
        char *scratch_base = top.base + top.off;
        {
            std::vector<u64> host;
            host.reserve(coef_words);
            size_t fi = 0;
            for (size_t s = 0; s < steps; s++) {
                EvalStep &e = st[s];
                const auto bind = [&](Form &f, bool coefs) {
                    for (size_t j = 0; j < f.terms(); j++) f.src[j] = elem[el[fi][j]];
                    fi++;
                    if (coefs) form_coefs(f, e.level, e.pass_lin, host);
                };
                for (size_t t = 0; t < e.x.size(); t++) {
                    bind(e.x[t], !pass_through(e.x[t], e.level));
                    bind(e.y[t], !pass_through(e.y[t], e.level));
                }
                bind(e.z, !e.z.empty());
            }
            if (host.size() != coef_words) return fail(ctx, HP_ELOGIC, "eval_plan: coefficient blocks do not match their count");
            if ((rc = stage_upload(ctx, host.data(), host.size() * 8, d_coef))) return rc;
        }
        for (size_t s = 0; s < steps; s++) {
            const EvalStep &e = st[s];
            const size_t lv = e.level, T = e.x.size();
            const u64 *dc = d_coef + e.coef_at;
            Carver cv(scratch_base);
            const Plan *lp;   // the level's limbs, for the coefficient-wise kernels
            if ((rc = get_plan(ctx, 0, moduli_ext, lv, false, &lp))) return rc;
            const auto materialise = [&](const Form &f, const u64 **out) -> int {
                if (pass_through(f, lv)) { *out = f.src[0]; return HP_OK; }
                u64 *buf = cv.take(batch * 2 * lv * n);
                *out = buf;
                int e2 = form_launch(ctx, lp->d_limbs, lv, n, batch, e.pass_lin, f, dc, false, buf, 2);
                dc += form_coef_words(f.terms(), e.pass_lin, lv);
                return e2;
            };
            if (T == 0) {   // rescale(Z): hp_dev_ckks_rescale's code on the materialised form
                const u64 *zb;
                if ((rc = materialise(e.z, &zb))) return rc;
                const Plan *p;
                if ((rc = get_plan(ctx, logn, moduli_ext, lv, true, &p))) return rc;
                LevelScope lvl(ctx, p);
                if (lvl.rc) return lvl.rc;
                if ((rc = drop_last(ctx, p, logn, lv, 2 * batch, false, 0, zb, Addend(), dst[s], cv))) return rc;
                continue;
            }
            std::vector<const u64 *> a(T), b(T);
            for (size_t t = 0; t < T; t++)
                if ((rc = materialise(e.x[t], &a[t])) || (rc = materialise(e.y[t], &b[t]))) return rc;
            u64 *quad = cv.take(batch * 3 * lv * n);
            if (T == 1) {   // one product: the tensor product of hp_dev_ckks_mult_relin_rescale_hks_at, its words
                ProfScope ps(ctx, "tensor");
                if ((rc = chk(ctx, hp_launch_tensor(lp->d_limbs, (u32)lv, 0, (u32)lv, (u32)n, (u32)batch, a[0], b[0], quad, ctx->stream), "tensor")))
                    return rc;
            } else if ((rc = tensor_sum(ctx, lp->d_limbs, n, lv, batch, e.pass_ts, {T, a.data(), b.data()}, quad))) {   // several: hp_dev_ckks_tensor_sum's launches
                return rc;
            }
            if (!e.z.empty() && (rc = form_launch(ctx, lp->d_limbs, lv, n, batch, e.pass_lin, e.z, dc, true, quad, 3))) return rc;
            HksCall c(ctx, logn, lv, key_L0, k, alpha, e.mext.data(), batch, 0);   // one call, and with it one level, per step
            if (c.rc || c.open()) return c.rc;
            if ((rc = relin_rescale(c, batch, quad, d_relin_key, dst[s], cv))) return rc;
        }
        const u64 *src = elem[steps];
        for (size_t d = 0; d < final_drops; d++) {   // hp_dev_ckks_rescale_n's sequence
            u64 *to = (d + 1 == final_drops) ? d_out : tmp[d & 1];
            const Plan *p;
            if ((rc = get_plan(ctx, logn, moduli_ext, last - d, true, &p))) return rc;
            LevelScope lvl(ctx, p);
            if (lvl.rc) return lvl.rc;
            Carver cv(scratch_base);
            if ((rc = drop_last(ctx, p, logn, last - d, 2 * batch, false, 0, src, Addend(), to, cv))) return rc;
            src = to;
        }
        return (int)HP_OK;
    });
}
