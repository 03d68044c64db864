// hp_api_hks_mult.cpp -- C ABI, part 3 (extension): the multiplication tails over the hybrid key switch (hp_hks_call.h) -- CKKS mult /
// relin_rescale / dot, the tensor sum, the BGV relin_modswitch / mult, BFV's mult_relin.  The six keyed entry points check in
// orders of their own: which message a doubly wrong call reports is part of each one's contract.
#include "hp_hks_call.h"

#include <algorithm>

using namespace hpi;

int hpi::tensor_quad(const HksCall &c, size_t batch, const u64 *ct1, const u64 *ct2, u64 *quad) {
    ProfScope ps(c.ctx, "tensor");
    return chk(c.ctx, hp_launch_tensor(c.plan->d_limbs, (u32)c.L, 0, (u32)c.L, (u32)c.n, (u32)batch, ct1, ct2, quad, c.ctx->stream), "tensor");
}

size_t hpi::relin_rescale_words(const HksCall &c, size_t batch) {
    return padded(batch * 2 * c.L * c.n) / 8 + c.switch_words(batch) + drop_ws_words(c.n, c.L, 2 * batch) + 2 * (padded(2 * batch * c.n) / 8);
}
int hpi::relin_rescale(const HksCall &c, size_t batch, const u64 *quad, const u64 *key, u64 *out, Carver &cv) {
    hp_ctx *ctx = c.ctx;
    const Plan *plan = c.plan;
    const uint64_t *moduli_ext = c.mext;
    const size_t logn = c.logn, L = c.L, n = c.n;
    int rc;
    u64 *lin = cv.take(batch * 2 * L * n);
    if (fused_drop_ok(ctx, logn) && !ctx->hks_two_step) {
        // ModDown and the rescale in ONE transform per remaining limb.  With c = the coefficients of the relinearised limb L-1,
        //   ((ks_i - NTT(rem_i)) P^-1 + quad_i - NTT(centre_i(c))) q_last^-1 = ((ks_i - NTT(rem_i + P centre_i(c))) P^-1 + quad_i) q_last^-1
        // so: ModDown of limb L-1 alone -> its coefficients -> rem_i += P centre_i(c) -> one fused transform over limbs 0..L-2.
        // The same residues as the two-step composition below (another lazy representative of them).
        const size_t P2 = 2 * batch, E = c.E;
        const Addend add(quad, L, 3 * L, 3);
        HksTail t;
        if ((rc = c.front(batch, quad + 2 * L * n, 3 * L, key, t, cv)) || (rc = c.pdown(batch, t))) return rc;
        u64 *r_last = cv.take(P2 * n), *c_last = cv.take(P2 * n);
        {
            HpDropArgs da = drop_args(t.ks + (L - 1) * n, E, add.from((L - 1) * n), r_last, 1);
            if ((rc = c.down_fused(L - 1, 1, P2, t.rem, da, ctx->cur_a, "hks ModDown of the last limb", "hks ModDown of the last limb (level A)")))
                return rc;
        }
        {
            HpNttJob lj = batch_job(plan, logn, 1, P2, r_last, c_last, 1, 1, 1, 1);
            lj.limbs = plan->d_limbs + (L - 1);
            if (ctx->cur_a) lj.limbs_a = plan->d_limbs_a + (L - 1);
            if ((rc = run_ntt(ctx, lj))) return rc;
        }
        const bool in_loads = !ctx->hks_combine_kernel;   // HP_HKS_COMBINE_KERNEL: the combination as its own kernel
        if (!in_loads) {
            ProfScope ps(ctx, "hks_combine");
            if ((rc = chk(ctx, hp_launch_hks_combine(plan->d_limbs, c.he->dev, (u32)L, (u32)n, (u32)P2, c_last, t.rem, ctx->stream), "hks_combine")))
                return rc;
        }
        HpNttJob fj = batch_job(plan, logn, L - 1, P2, t.rem, nullptr, L, 0, 0, 0);
        HpDropArgs da = drop_args(t.ks, E, add, out, L - 1);
        hks_down_rescale_consts(c.he->host, moduli_ext, L, in_loads ? c_last : nullptr, da);
        ProfScope ps(ctx, "ntt_drop");
        if (ctx->cur_a && in_loads) {
            // the two-drops flavour of hp_ntt_a.hip (DropPre2A has the algebra): z = ((A x + a) - NTT(m c1 + c2)) B with x = ks, a = quad,
            // c1 = the remainders (as they are), c2 = the centred coefficients of the relinearised last limb, A = m = P^-1, B = q_last^-1 --
            // by linearity the level-B line above: ((ks - NTT(rem + P centre(c))) P^-1 + quad) q_last^-1
            fj.limbs_a = plan->d_limbs_a;
            hks_down_rescale_consts_a(moduli_ext, L, da);
            return chk(ctx, hp_launch_ntt_a_drop(fj, da, ctx->stream), "hks fused ModDown + rescale (level A)");
        }
        return chk(ctx, hp_launch_ntt_fast_drop(fj, da, ctx->stream), "hks fused ModDown + rescale");
    }
    if ((rc = c.key_switch(batch, quad + 2 * L * n, 3 * L, key, Addend(quad, L, 3 * L, 3), lin, cv))) return rc;
    return drop_last(ctx, plan, logn, L, 2 * batch, false, 0, lin, Addend(), out, cv);
}

// ckks::mult_low_level + relinearisation with a hybrid key + rescale by the last ciphertext modulus
extern "C" int hp_dev_ckks_mult_relin_rescale_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                                     const uint64_t *moduli_ext, size_t batch, const uint64_t *ct1, const uint64_t *ct2,
                                                     const uint64_t *key, uint64_t *out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, ct1, ct2, key, out);
    HP_ALIGNED(ctx, ct1, ct2, key, out);
    HksCall c(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, 0);
    if (c.rc) return c.rc;
    if (L < 2) return fail(ctx, HP_EINVAL, "Unable to drop the only one prime.");
    if (c.open()) return c.rc;
    const size_t n = c.n;
    int rc = ws_reserve(ctx, (padded(batch * 3 * L * n) / 8 + relin_rescale_words(c, batch)) * 8);
    if (rc) return rc;
    Carver cv(ctx->ws);
    u64 *quad = cv.take(batch * 3 * L * n);
    if ((rc = tensor_quad(c, batch, ct1, ct2, quad))) return rc;
    return relin_rescale(c, batch, quad, key, out, cv);
}
extern "C" int hp_dev_ckks_mult_relin_rescale_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                       size_t batch, const uint64_t *ct1, const uint64_t *ct2, const uint64_t *key,
                                       uint64_t *out) {
    return hp_dev_ckks_mult_relin_rescale_hks_at(ctx, logn, L, L, k, alpha, moduli_ext, batch, ct1, ct2, key, out);
}

// the tail alone, on the caller's quadratic ciphertexts (hp_dev_mult_low_level's or hp_dev_ckks_tensor_sum's)
extern "C" int hp_dev_ckks_relin_rescale_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                                const uint64_t *moduli_ext, size_t batch, const uint64_t *d_quad, const uint64_t *d_key,
                                                uint64_t *d_out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, d_quad, d_key, d_out);
    HP_ALIGNED(ctx, d_quad, d_key, d_out);
    HksCall c(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, 0);
    if (c.rc) return c.rc;
    if (L < 2) return fail(ctx, HP_EINVAL, "Unable to drop the only one prime.");
    int rc = no_overlap(ctx, "relin_rescale", d_quad, batch * 3 * L * c.n * 8, d_out, batch * 2 * (L - 1) * c.n * 8);
    if (rc) return rc;
    if (c.open()) return c.rc;
    if ((rc = ws_reserve(ctx, relin_rescale_words(c, batch) * 8))) return rc;
    Carver cv(ctx->ws);
    return relin_rescale(c, batch, d_quad, d_key, d_out, cv);
}
extern "C" int hp_dev_ckks_relin_rescale_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                             size_t batch, const uint64_t *d_quad, const uint64_t *d_key, uint64_t *d_out) {
    return hp_dev_ckks_relin_rescale_hks_at(ctx, logn, L, L, k, alpha, moduli_ext, batch, d_quad, d_key, d_out);
}

// ---- sums of products: lazy relinearisation (hp_hks_call.h: TensorSumTerms) ------------------------------------------------------------
int hpi::tensor_sum_ok(hp_ctx *ctx, const char *call, size_t n, size_t L, size_t batch, const TensorSumTerms &ts, const void *out,
                       size_t out_bytes) {
    const auto bad = [&](const char *what) { return fail(ctx, HP_EINVAL, std::string(call) + ": " + what); };
    if (ts.terms == 0) return bad("no terms");
    // (512 words per workgroup at the least: every launch stays below 2^30 workgroups, and every u32 row count with it)
    if (batch > ((size_t)1 << 30) / (L * ((n + 511) / 512)))
        return fail(ctx, HP_EUNSUPPORTED, std::string(call) + ": too many ciphertexts for one call");
    const size_t in_bytes = batch * 2 * L * n * 8;
    for (size_t t = 0; t < ts.terms; t++)
        for (const uint64_t *p : {ts.a[t], ts.b[t]}) {
            if (!p || ((uintptr_t)p & 15u)) return bad("NULL or misaligned operand");
            if (ranges_overlap(p, in_bytes, out, out_bytes)) return bad("the output overlaps an operand");
        }
    return HP_OK;
}
int hpi::tensor_sum(hp_ctx *ctx, const HpLimb *limbs, size_t n, size_t L, size_t batch, size_t pass, const TensorSumTerms &ts, u64 *quad) {
    for (size_t t0 = 0; t0 < ts.terms; t0 += pass) {
        HpTensorSumTable tab;
        memset(&tab, 0, sizeof(tab));
        tab.terms = (u32)std::min(pass, ts.terms - t0);
        std::copy(ts.a + t0, ts.a + t0 + tab.terms, tab.a);
        std::copy(ts.b + t0, ts.b + t0 + tab.terms, tab.b);
        ProfScope ps(ctx, "tensor");
        int rc = chk(ctx, hp_launch_tensor_sum(limbs, (u32)L, (u32)n, (u32)batch, tab, t0 != 0, quad, ctx->stream), "tensor_sum");
        if (rc) return rc;
    }
    return HP_OK;
}

extern "C" int hp_dev_ckks_tensor_sum(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch, size_t terms,
                                      const uint64_t *const *d_a, const uint64_t *const *d_b, uint64_t *d_quad) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli, d_a, d_b, d_quad);
    HP_ALIGNED(ctx, d_quad);
    if (!logn_ok(logn)) return fail(ctx, HP_EUNSUPPORTED, HP_LOGN_MSG);
    if (L < 1 || L > HP_MAX_LIMBS) return fail(ctx, HP_EINVAL, "unsupported number of moduli");
    if (batch == 0) return fail(ctx, HP_EINVAL, "empty batch");
    const size_t n = (size_t)1 << logn;
    const TensorSumTerms ts = {terms, d_a, d_b};
    int rc = tensor_sum_ok(ctx, "tensor_sum", n, L, batch, ts, d_quad, batch * 3 * L * n * 8);
    if (rc) return rc;
    const size_t pass = tensor_sum_max_terms(moduli, L, HP_TENSOR_SUM_MAX);   // terms per launch
    if (pass == 0) return fail(ctx, HP_EUNSUPPORTED, "tensor_sum: moduli too large for the 128-bit accumulators");
    const Plan *plan;
    if ((rc = get_plan(ctx, 0, moduli, L, false, &plan))) return rc;
    return tensor_sum(ctx, plan->d_limbs, n, L, batch, pass, ts, d_quad);
}

// the composition: the sum into a workspace quad, then the tail.  One reservation, a function of the shape alone, never of `terms`
extern "C" int hp_dev_ckks_dot_relin_rescale_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                                    const uint64_t *moduli_ext, size_t batch, size_t terms, const uint64_t *const *d_a,
                                                    const uint64_t *const *d_b, const uint64_t *d_key, uint64_t *d_out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, d_a, d_b, d_key, d_out);
    HP_ALIGNED(ctx, d_key, d_out);
    HksCall c(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, 0);
    if (c.rc) return c.rc;
    if (L < 2) return fail(ctx, HP_EINVAL, "Unable to drop the only one prime.");
    const size_t n = c.n;
    const TensorSumTerms ts = {terms, d_a, d_b};
    int rc = tensor_sum_ok(ctx, "dot_relin_rescale", n, L, batch, ts, d_out, batch * 2 * (L - 1) * n * 8);
    if (rc) return rc;
    const size_t pass = tensor_sum_max_terms(moduli_ext, L, HP_TENSOR_SUM_MAX);
    if (pass == 0) return fail(ctx, HP_EUNSUPPORTED, "dot_relin_rescale: moduli too large for the 128-bit accumulators");
    if (c.open()) return c.rc;
    if ((rc = ws_reserve(ctx, (padded(batch * 3 * L * n) / 8 + relin_rescale_words(c, batch)) * 8))) return rc;
    Carver cv(ctx->ws);
    u64 *quad = cv.take(batch * 3 * L * n);
    if ((rc = tensor_sum(ctx, c.plan->d_limbs, n, L, batch, pass, ts, quad))) return rc;
    return relin_rescale(c, batch, quad, d_key, d_out, cv);
}
extern "C" int hp_dev_ckks_dot_relin_rescale_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                                 size_t batch, size_t terms, const uint64_t *const *d_a, const uint64_t *const *d_b,
                                                 const uint64_t *d_key, uint64_t *d_out) {
    return hp_dev_ckks_dot_relin_rescale_hks_at(ctx, logn, L, L, k, alpha, moduli_ext, batch, terms, d_a, d_b, d_key, d_out);
}

// ---- BGV over the hybrid path --------------------------------------------------------------------------------------------------------
// Only ModDown knows the scheme (HksCall::pmod, k_hks_moddown_t; hehub_amd.h has the convention): a multiplication is the tensor
// product, the switch of d2 with (d0, d1) as its addend, then hehub's own mod_drop_one_prime_inplace (drop_last with bgv = true: its
// q_last mod t factor included) -- the two-step composition of relin_rescale above.  ModDown_t and the mod switch are NOT merged into
// one transform: that path is CKKS's.
int hpi::bgv_relin_modswitch(const HksCall &c, size_t batch, const u64 *quad, const u64 *key, u64 *out, Carver &cv) {
    const size_t L = c.L, n = c.n;
    u64 *lin = cv.take(batch * 2 * L * n);
    int rc = c.key_switch(batch, quad + 2 * L * n, 3 * L, key, Addend(quad, L, 3 * L, 3), lin, cv);
    if (rc) return rc;
    return drop_last(c.ctx, c.plan, c.logn, L, 2 * batch, true, c.pmod, lin, Addend(), out, cv);
}

// The tail on the caller's quadratic ciphertexts -- hp_dev_mult_low_level's, or a sum of products by hp_dev_ckks_tensor_sum, whose
// arithmetic is scheme-free (residues of sums of products: nothing in it is CKKS's): T products pay one switch and one mod switch.
extern "C" int hp_dev_bgv_relin_modswitch_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                                 const uint64_t *moduli_ext, uint64_t plain_modulus, size_t batch, const uint64_t *d_quad,
                                                 const uint64_t *d_key, uint64_t *d_out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, d_quad, d_key, d_out);
    HP_ALIGNED(ctx, d_quad, d_key, d_out);
    HksCall c(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, plain_modulus);
    if (c.rc) return c.rc;
    if (L < 2) return fail(ctx, HP_EINVAL, "Unable to drop the only one prime.");
    if (c.plain_ok()) return c.rc;
    int rc = no_overlap(ctx, "bgv_relin_modswitch", d_quad, batch * 3 * L * c.n * 8, d_out, batch * 2 * (L - 1) * c.n * 8);
    if (rc) return rc;
    if (c.open()) return c.rc;
    if ((rc = ws_reserve(ctx, relin_rescale_words(c, batch) * 8))) return rc;
    Carver cv(ctx->ws);
    return bgv_relin_modswitch(c, batch, d_quad, d_key, d_out, cv);
}
extern "C" int hp_dev_bgv_relin_modswitch_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                              uint64_t plain_modulus, size_t batch, const uint64_t *d_quad, const uint64_t *d_key,
                                              uint64_t *d_out) {
    return hp_dev_bgv_relin_modswitch_hks_at(ctx, logn, L, L, k, alpha, moduli_ext, plain_modulus, batch, d_quad, d_key, d_out);
}

// bgv::mult_low_level + relinearisation with a hybrid key + mod switch: the tensor product into a workspace quad, then the tail
extern "C" int hp_dev_bgv_mult_relin_modswitch_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                                      const uint64_t *moduli_ext, uint64_t plain_modulus, size_t batch, const uint64_t *ct1,
                                                      const uint64_t *ct2, const uint64_t *key, uint64_t *out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, ct1, ct2, key, out);
    HP_ALIGNED(ctx, ct1, ct2, key, out);
    HksCall c(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, plain_modulus);
    if (c.rc) return c.rc;
    if (L < 2) return fail(ctx, HP_EINVAL, "Unable to drop the only one prime.");
    if (c.plain_ok() || c.open()) return c.rc;
    const size_t n = c.n;
    int rc = ws_reserve(ctx, (padded(batch * 3 * L * n) / 8 + relin_rescale_words(c, batch)) * 8);
    if (rc) return rc;
    Carver cv(ctx->ws);
    u64 *quad = cv.take(batch * 3 * L * n);
    if ((rc = tensor_quad(c, batch, ct1, ct2, quad))) return rc;
    return bgv_relin_modswitch(c, batch, quad, key, out, cv);
}
extern "C" int hp_dev_bgv_mult_relin_modswitch_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                                   uint64_t plain_modulus, size_t batch, const uint64_t *ct1, const uint64_t *ct2,
                                                   const uint64_t *key, uint64_t *out) {
    return hp_dev_bgv_mult_relin_modswitch_hks_at(ctx, logn, L, L, k, alpha, moduli_ext, plain_modulus, batch, ct1, ct2, key, out);
}

// ---- BFV over the hybrid path ----------------------------------------------------------------------------------------------------------
// BFV's multiplication differs from the others before the switch, not in it: the quadratic ciphertext comes from the scale-invariant
// product over Q B (bfv_mult, hp_api_bfv.cpp) as canonical residues, and the switch of y2 with (y0, y1) as its addend is the CKKS one
// (keys with error e, no factor t: the plain ModDown).  The BFV refusals come first, then everything the switch refuses.
extern "C" int hp_dev_bfv_mult_relin_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                            size_t M, const uint64_t *aux_moduli, uint64_t t, size_t batch, const uint64_t *ct1,
                                            const uint64_t *ct2, const uint64_t *key, uint64_t *out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, aux_moduli, ct1, ct2, key, out);
    HP_ALIGNED(ctx, ct1, ct2, key, out);
    int rc = bfv_check(ctx, logn, L, M, moduli_ext, aux_moduli, true, t, batch);
    if (rc) return rc;
    const size_t n = (size_t)1 << logn;
    if ((rc = no_overlap(ctx, "bfv_mult_relin", ct1, batch * 2 * L * n * 8, out, batch * 2 * L * n * 8)) ||
        (rc = no_overlap(ctx, "bfv_mult_relin", ct2, batch * 2 * L * n * 8, out, batch * 2 * L * n * 8)))
        return rc;
    HksCall c(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, 0);
    if (c.rc) return c.rc;
    BfvShape s;
    if ((rc = bfv_open(ctx, logn, L, M, moduli_ext, aux_moduli, true, t, s))) return rc;
    if (c.open()) return c.rc;
    if ((rc = ws_reserve(ctx, padded(batch * 3 * L * n) + bfv_mult_bytes(s, batch) + c.switch_words(batch) * 8))) return rc;
    Carver cv(ctx->ws);
    u64 *quad = cv.take(batch * 3 * L * n);
    if ((rc = bfv_mult(ctx, s, batch, ct1, ct2, quad, cv))) return rc;
    return c.key_switch(batch, quad + 2 * L * n, 3 * L, key, Addend(quad, L, 3 * L, 3), out, cv);
}
extern "C" int hp_dev_bfv_mult_relin_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t M,
                                         const uint64_t *aux_moduli, uint64_t t, size_t batch, const uint64_t *ct1, const uint64_t *ct2,
                                         const uint64_t *key, uint64_t *out) {
    return hp_dev_bfv_mult_relin_hks_at(ctx, logn, L, L, k, alpha, moduli_ext, M, aux_moduli, t, batch, ct1, ct2, key, out);
}
