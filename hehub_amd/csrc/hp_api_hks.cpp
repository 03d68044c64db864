// hp_api_hks.cpp -- C ABI, part 3 (extension): hybrid key switch -- digits of several moduli, several special primes; the call object
// of hp_hks_call.h and what runs on its digit rows (switch, rotations, hoisted rotations, the diagonal transforms); kernels in
// hp_hks.hip.  Exact integer arithmetic throughout (ModUp / ModDown by mixed-radix composition); keys have
// their own format, so results are pinned by an exact integer model and by decryption, not by hehub's words.
#include "hp_hks_call.h"
#include "hp_ntt_job.h"   // item counts

#include <algorithm>
#include <vector>

using namespace hpi;

static int get_hks_consts(hp_ctx *ctx, const uint64_t *mext, size_t L, size_t k, size_t alpha, const HksEntry **out) {
    return contained(ctx, [&] {
        const size_t E = L + k, nd = (L + alpha - 1) / alpha;
        auto key = std::make_pair(std::vector<u64>(mext, mext + E), std::make_pair(k, alpha));
        auto it = ctx->hks.find(key);
        if (it == ctx->hks.end()) {
            if (ctx->hks.size() >= MAX_HKS) {   // bounded cache (an entry is ~150 KB of device memory)
                HIP_TRY(ctx, hipDeviceSynchronize());
                for (auto &kv : ctx->hks) (void)hipFree(kv.second.dev);
                ctx->hks.clear();
            }
            typedef unsigned __int128 u128;
            std::vector<HpHksConsts> hold(1);
            HpHksConsts &c = hold[0];
            memset(&c, 0, sizeof(c));
            c.L = (u32)L; c.k = (u32)k; c.alpha = (u32)alpha; c.nd = (u32)nd; c.E = (u32)E;
            for (size_t d = 0; d < nd; d++) {
                const size_t first = d * alpha, cnt = std::min(alpha, L - first);
                for (size_t a = 0; a < cnt; a++)
                    for (size_t b = 0; b < a; b++) {
                        const u64 qa = mext[first + a], qb = mext[first + b];
                        if (qb % qa == 0) return fail(ctx, HP_EINVAL, "moduli are not pairwise coprime");
                        c.inv[d][b][a] = hp::inverse_mod_prime(qb % qa, qa) % qa;
                        c.inv_h[d][b][a] = hp::harvey_quotient(c.inv[d][b][a], qa);
                    }
                for (size_t m = 0; m < E; m++) {
                    u64 prod = 1 % mext[m];
                    for (size_t a = 0; a < cnt; a++) {
                        c.pref[d][m][a] = prod;
                        c.pref_h[d][m][a] = hp::harvey_quotient(prod, mext[m]);
                        prod = (u64)((u128)prod * (mext[first + a] % mext[m]) % mext[m]);
                    }
                }
            }
            HksEntry e;   // P^-1 and P mod q_i (the latter for the merged ModDown + rescale whatever k is): also kept on the host
            if (!hks_limb_consts(mext, L, k, e.host)) return fail(ctx, HP_EINVAL, "moduli are not pairwise coprime");
            for (size_t i = 0; i < L; i++) {
                c.pinv[i] = e.host.pinv[i]; c.pinv_h[i] = e.host.pinv_h[i];
                c.p_mod_q[i] = e.host.p_mod_q[i]; c.p_mod_q_h[i] = e.host.p_mod_q_h[i];
            }
            const uint64_t *pm = mext + L;
            if (k <= HP_HKS_MAX_ALPHA) {   // Garner tables of the one-kernel ModDown conversion
                for (size_t a = 0; a < k; a++)
                    for (size_t b = 0; b < a; b++) {
                        if (pm[b] % pm[a] == 0) return fail(ctx, HP_EINVAL, "moduli are not pairwise coprime");
                        c.pg_inv[b][a] = hp::inverse_mod_prime(pm[b] % pm[a], pm[a]) % pm[a];
                        c.pg_inv_h[b][a] = hp::harvey_quotient(c.pg_inv[b][a], pm[a]);
                    }
                for (size_t a = 0; a < k; a++) {   // digits of floor(P/2): residues (p_a - 1)/2
                    u64 u = (pm[a] - 1) / 2;
                    for (size_t b = 0; b < a; b++) u = (u64)((u128)((u + pm[a] - c.p_half[b] % pm[a]) % pm[a]) * c.pg_inv[b][a] % pm[a]);
                    c.p_half[a] = u;
                }
                for (size_t i = 0; i < L; i++) {
                    u64 prod = 1 % mext[i];
                    for (size_t a = 0; a < k; a++) {
                        c.p_pref[i][a] = prod;
                        c.p_pref_h[i][a] = hp::harvey_quotient(prod, mext[i]);
                        prod = (u64)((u128)prod * (pm[a] % mext[i]) % mext[i]);
                    }
                }
            }
            int rc = upload(ctx, &c, sizeof(c), (void **)&e.dev);
            if (rc) return rc;
            it = ctx->hks.emplace(key, std::move(e)).first;
        }
        *out = &it->second;
        return (int)HP_OK;
    });
}

// Parity level A for the drops that end a hybrid key switch (round 6; DESIGN section 7 item 1 of round 5): the FP64 drop kernels of
// hp_ntt_a.hip take them as they are -- their compile-time flavours 1 / 2 / 5 (no addend / addend on both polynomials / on polynomial 0)
// for ModDown, flavour 6 (two drops in one transform) for ModDown merged with the rescale.  What differs from hehub's drops is only
// that the transform's input rows already ARE the per-limb remainders (hp_drop.h: a_raw_rows).
static bool a_drop_shape(const Addend &add) { return add.mask == 0 || add.mask == 3u || add.mask == 1u; }

namespace hpi {   // hp_hks_call.h has the contracts of what follows
HksCall::HksCall(hp_ctx *c, size_t logn_, size_t L_, size_t key_L0_, size_t k_, size_t alpha_, const uint64_t *moduli_ext, size_t batch,
                 uint64_t plain_modulus)
    : ctx(c), mext(moduli_ext), logn(logn_), L(L_), key_L0(key_L0_), k(k_), alpha(alpha_), pmod(plain_modulus), rc(limits(batch)) {
    if (!rc) n = (size_t)1 << logn, E = L + k, KE = key_L0 + k, nd = (L + alpha - 1) / alpha;
}
int HksCall::limits(size_t batch) const {
    if (!logn_ok(logn)) return fail(ctx, HP_EUNSUPPORTED, HP_LOGN_MSG);
    if (L < 1 || k < 1 || k > HP_CRT_MAX_LIMBS || L + k > HP_MAX_LIMBS) return fail(ctx, HP_EINVAL, "unsupported number of moduli");
    if (alpha < 1 || alpha > HP_HKS_MAX_ALPHA || (L + alpha - 1) / alpha > HP_HKS_MAX_DIGITS)
        return fail(ctx, HP_EINVAL, "unsupported digit size");
    if (batch == 0) return fail(ctx, HP_EINVAL, "empty batch");
    if (key_L0 < L) return fail(ctx, HP_EINVAL, "the key has fewer moduli than the ciphertext");
    // (after L's own limits: with key_L0 == L these two can never be what refuses a call)
    if (key_L0 > HP_MAX_LIMBS || key_L0 + k > HP_MAX_LIMBS) return fail(ctx, HP_EINVAL, "unsupported number of key moduli");
    if ((key_L0 + alpha - 1) / alpha > HP_HKS_MAX_DIGITS) return fail(ctx, HP_EINVAL, "unsupported digit size of the key");
    return HP_OK;
}
int HksCall::open() {
    if ((rc = get_plan(ctx, logn, mext, E, true, &plan)) || (rc = get_hks_consts(ctx, mext, L, k, alpha, &he))) return rc;
    lvl.emplace(ctx, plan);   // level A: the digit stages (lifted digits, coefficient rows) and the drops on the FP64 kernels
    if (pmod) plain_consts();
    return rc = lvl->rc;
}
int HksCall::plain_ok() {
    if (rc) return rc;
    if (pmod == 0) return rc = fail(ctx, HP_EINVAL, "plain modulus must be positive");
    for (size_t m = 0; m < L + k; m++)
        if (pmod >= mext[m]) return rc = fail(ctx, HP_EINVAL, "plain modulus must be below every modulus of the chain");
    if (k > HP_HKS_MAX_ALPHA) return rc = fail(ctx, HP_EUNSUPPORTED, "more than 8 special primes with a plain modulus");
    return HP_OK;
}
void HksCall::plain_consts() {
    memset(&plain, 0, sizeof(plain));
    for (size_t a = 0; a < k; a++) {
        const u64 p = mext[L + a];
        plain.tinv_p[a] = hp::inverse_mod_prime(pmod % p, p) % p;
        plain.tinv_p_h[a] = hp::harvey_quotient(plain.tinv_p[a], p);
    }
    for (size_t i = 0; i < L; i++) {
        plain.t_mod_q[i] = pmod % mext[i];
        plain.t_mod_q_h[i] = hp::harvey_quotient(plain.t_mod_q[i], mext[i]);
    }
}

int HksCall::digits(size_t P, const u64 *pt, size_t pt_pstride, u64 **lifted_out, Carver &cv) const {
    u64 *coef = cv.take(P * L * n), *lifted = cv.take(P * nd * E * n);
    *lifted_out = lifted;
    int e;
    // coefficients of the input, strictly reduced (as rgsw.cpp:103-105)
    if ((e = ks_coef(ctx, plan, logn, L, P, 0, L, pt, pt_pstride, coef))) return e;
    {   // ModUp: every digit's exact integer into every modulus outside the digit
        ProfScope ps(ctx, "hks_modup");
        if ((e = chk(ctx, hp_launch_hks_modup(plan->d_limbs, he->dev, (u32)alpha, (u32)nd, (u32)n, (u32)P, coef, lifted, ctx->stream),
                     "hks_modup")))
            return e;
    }
    // transforms of the lifted limbs, in place
    HpNttJob j;
    memset(&j, 0, sizeof(j));
    j.limbs = plan->d_limbs; j.src = lifted; j.dst = lifted; j.logn = (u32)logn; j.L = (u32)L; j.P = (u32)P;
    j.hks_nd = (u32)nd; j.hks_E = (u32)E; j.hks_alpha = (u32)alpha; j.mode = HP_NTT_HKS;
    j.W = hp_hks_items((u32)L, (u32)nd, (u32)k, (u32)P);
    // parity level A: the lifted rows are canonical residues (ModUp's exact conversion), the inner product takes any
    // representative, and hybrid results have no word-level contract with hehub (other keys): the FP64 transform where allowed
    if (ctx->cur_a) j.limbs_a = plan->d_limbs_a;
    return run_ntt(ctx, j);
}

int HksCall::front(size_t P, const u64 *pt, size_t pt_pstride, const u64 *key, HksTail &t, Carver &cv) const {
    u64 *lifted;
    int e = digits(P, pt, pt_pstride, &lifted, cv);
    if (e) return e;
    t = tail(P, cv);
    ProfScope ps(ctx, "ks_inner");
    return chk(ctx, hp_launch_hks_inner(plan->d_limbs, (u32)L, (u32)E, (u32)KE, (u32)nd, (u32)alpha, (u32)n, (u32)P, lifted, pt, (u32)pt_pstride, key,
                                        t.ks, ctx->stream), "hks_inner");
}

int HksCall::pdown(size_t P, const HksTail &t) const {
    int e;
    {
        HpNttJob j = batch_job(plan, logn, k, 2 * P, t.ks + L * n, t.yp, E, k, 1, 1);
        j.limbs = plan->d_limbs + L;
        if (ctx->cur_a) j.limbs_a = plan->d_limbs_a + L;   // (strict either way: the same words)
        if ((e = run_ntt(ctx, j))) return e;
    }
    if (pmod) {   // (k <= HP_HKS_MAX_ALPHA: plain_ok)
        ProfScope ps(ctx, "hks_moddown_t");
        return chk(ctx, hp_launch_hks_moddown_t(plan->d_limbs, he->dev, plain, (u32)k, (u32)n, (u32)(2 * P), t.yp, t.rem, ctx->stream),
                   "hks_moddown_t");
    }
    if (k <= HP_HKS_MAX_ALPHA) {
        ProfScope ps(ctx, "hks_moddown");
        return chk(ctx, hp_launch_hks_moddown(plan->d_limbs, he->dev, (u32)k, (u32)n, (u32)(2 * P), t.yp, t.rem, ctx->stream), "hks_moddown");
    }
    // many special primes: one composition per target modulus (hp_edge.hip)
    const Plan *pplan;
    if ((e = get_plan(ctx, 0, mext + L, k, false, &pplan))) return e;
    for (size_t i = 0; i < L; i++) {
        const HpCrtConsts *cc;
        if ((e = get_crt_consts(ctx, mext + L, k, mext[i], &cc))) return e;
        ProfScope ps(ctx, "hks_moddown");
        if ((e = chk(ctx, hp_launch_base_to_single_crt(pplan->d_limbs, cc, (u32)k, (u32)n, (u32)(2 * P), t.yp, t.rem + i * n, (u32)L, nullptr,
                                                       ctx->stream), "hks_moddown")))
            return e;
    }
    return HP_OK;
}

int HksCall::down_fused(size_t i0, size_t cnt, size_t P2, const u64 *rem, HpDropArgs &da, bool level_a, const char *what, const char *what_a) const {
    HpNttJob fj = batch_job(plan, logn, cnt, P2, rem + i0 * n, nullptr, L, 0, 0, 0);
    fj.limbs = plan->d_limbs + i0;
    hks_down_consts(he->host, i0, cnt, da);
    ProfScope ps(ctx, "ntt_drop");
    if (!level_a) return chk(ctx, hp_launch_ntt_fast_drop(fj, da, ctx->stream), what);
    fj.limbs_a = plan->d_limbs_a + i0;
    hks_down_consts_a(mext, i0, cnt, da);
    return chk(ctx, hp_launch_ntt_a_drop(fj, da, ctx->stream), what_a);
}

int HksCall::down(size_t P, const u64 *ks, u64 *rem, const Addend &add, u64 *out) const {
    if (fused_drop_ok(ctx, logn)) {
        HpDropArgs da = drop_args(ks, E, add, out, L);
        return down_fused(0, L, 2 * P, rem, da, ctx->cur_a && a_drop_shape(add), "hks fused ModDown", "hks fused ModDown (level A)");
    }
    int e = run_ntt(ctx, batch_job(plan, logn, L, 2 * P, rem, rem, L, L, 0, 0));
    if (e) return e;
    ProfScope ps(ctx, "hks_down_fin");
    return chk(ctx, hp_launch_hks_down_fin(plan->d_limbs, he->dev, (u32)L, (u32)n, (u32)(2 * P), ks, rem, add.rows, add.poly_stride,
                                           add.ct_stride, add.mask, out, ctx->stream), "hks_down_fin");
}

int rotations_ok(hp_ctx *ctx, const char *call, const HksRotations &rot, const uint64_t *const *diags, bool identity_ok) {
    const auto bad = [&](const char *what) { return fail(ctx, HP_EINVAL, std::string(call) + ": " + what); };
    for (size_t r = 0; r < rot.count; r++) {
        const bool cj = rot.conj && rot.conj[r], far = !cj && !rot_step_ok(rot.steps[r]);
        if (identity_ok && far) return fail(ctx, HP_EINVAL, "rotation step out of range");
        if (!rot.keys[r] && !(identity_ok && !cj && rot.steps[r] == 0))
            return bad(identity_ok ? "a NULL key on an entry that is not the identity" : "NULL or misaligned key");
        if ((uintptr_t)rot.keys[r] & 15u) return bad(identity_ok ? "misaligned key" : "NULL or misaligned key");
        if (diags && ((uintptr_t)diags[r] & 15u)) return bad("misaligned diagonal");
        if (far) return fail(ctx, HP_EINVAL, "rotation step out of range");
    }
    return HP_OK;
}

int no_overlap(hp_ctx *ctx, const char *call, const void *in, size_t in_bytes, const void *out, size_t out_bytes) {
    if (ranges_overlap(in, in_bytes, out, out_bytes)) return fail(ctx, HP_EINVAL, std::string(call) + ": the output overlaps the input");
    return HP_OK;
}

} // namespace hpi

// Every call that takes a key is written once, as its _at form (a key generated for key_L0 >= L ciphertext moduli; hehub_amd.h has
// the row map); the plain entry point is the case key_L0 == L of the same code.
// The calls that exist for both schemes are written once more: bgv_t == NULL is the CKKS call, else *bgv_t is the plain modulus of
// its BGV twin (hp_dev_bgv_*_hks), whose own refusals (HksCall::plain_ok) come right after the limits the two share.
static int dev_hks_switch(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext,
                          const uint64_t *bgv_t, size_t batch, const uint64_t *pt, const uint64_t *key, uint64_t *out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, pt, key, out);
    HP_ALIGNED(ctx, pt, key, out);
    HksCall c(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, bgv_t ? *bgv_t : 0);
    if (c.rc || (bgv_t && c.plain_ok()) || c.open()) return c.rc;
    int rc = ws_reserve(ctx, c.switch_words(batch) * 8);
    if (rc) return rc;
    Carver cv(ctx->ws);
    return c.key_switch(batch, pt, L, key, Addend(), out, cv);
}
extern "C" int hp_dev_hks_switch_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                    size_t batch, const uint64_t *pt, const uint64_t *key, uint64_t *out) {
    return dev_hks_switch(ctx, logn, L, key_L0, k, alpha, moduli_ext, nullptr, batch, pt, key, out);
}
extern "C" int hp_dev_hks_switch(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t batch,
                      const uint64_t *pt, const uint64_t *key, uint64_t *out) {
    return hp_dev_hks_switch_at(ctx, logn, L, L, k, alpha, moduli_ext, batch, pt, key, out);
}

// ckks rotate / conjugate with a hybrid key: moved = gather(ct); out = key_switch(moved[1]); out[0] += moved[0]
static int dev_hks_automorphism(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *mext, size_t batch,
                                bool conj, size_t step, const uint64_t *ct, const uint64_t *key, uint64_t *out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, mext, ct, key, out);
    HP_ALIGNED(ctx, ct, key, out);
    HksCall c(ctx, logn, L, key_L0, k, alpha, mext, batch, 0);
    if (c.rc) return c.rc;
    if (!conj && !rot_step_ok(step)) return fail(ctx, HP_EINVAL, "rotation step out of range");
    if (c.open()) return c.rc;
    const size_t n = c.n;
    int rc = ws_reserve(ctx, (padded(batch * 2 * L * n) / 8 + c.switch_words(batch)) * 8);
    if (rc) return rc;
    Carver cv(ctx->ws);
    u64 *moved = cv.take(batch * 2 * L * n);
    if ((rc = move_rows(ctx, logn, batch * 2 * L, conj, step, ct, moved))) return rc;
    return c.key_switch(batch, moved + L * n, 2 * L, key, Addend(moved, L, 2 * L, 1), out, cv);
}
extern "C" int hp_dev_ckks_rotate_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t batch,
                           size_t step, const uint64_t *ct, const uint64_t *rot_key, uint64_t *out) {
    return dev_hks_automorphism(ctx, logn, L, L, k, alpha, moduli_ext, batch, false, step, ct, rot_key, out);
}
extern "C" int hp_dev_ckks_rotate_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                         size_t batch, size_t step, const uint64_t *ct, const uint64_t *rot_key, uint64_t *out) {
    return dev_hks_automorphism(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, false, step, ct, rot_key, out);
}
extern "C" int hp_dev_ckks_conjugate_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t batch,
                              const uint64_t *ct, const uint64_t *conj_key, uint64_t *out) {
    return dev_hks_automorphism(ctx, logn, L, L, k, alpha, moduli_ext, batch, true, 0, ct, conj_key, out);
}
extern "C" int hp_dev_ckks_conjugate_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                            const uint64_t *moduli_ext, size_t batch, const uint64_t *ct, const uint64_t *conj_key,
                                            uint64_t *out) {
    return dev_hks_automorphism(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, true, 0, ct, conj_key, out);
}

// Hoisted rotations: `rotations` automorphisms of every ciphertext, each with its own key, over ONE digit stage.  The digit rows are
// those of the unrotated c1; rotation r reads them through its map inside the inner product (k_hks_inner_hoisted).  Moving a
// transformed digit row is the transform of the moved digit read as a SIGNED integer -- the automorphism negates some coefficients,
// and -x stays -x in every modulus instead of becoming q_j - x inside the digit and being lifted from there -- so the lifted limbs
// hold another representative than hp_dev_ckks_rotate_hks's, of the same magnitude bound |x| < Q_d: different words, the same
// decryption.  Everything after the inner product runs as for any switch, on the polynomials (b, r) -> b * rotations + r.
// The rotations are processed HOIST_POLYS / batch at a time (at least one, at most one argument table) against the same digit
// rows: the working set of a pass is that of an unhoisted rotation of HOIST_POLYS ciphertexts, whatever `rotations` is.
constexpr size_t HOIST_POLYS = 32;
static int dev_rotate_hoisted_hks(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                  const uint64_t *bgv_t, size_t batch, size_t rotations, const size_t *steps, const unsigned char *conj,
                                  const uint64_t *ct, const uint64_t *const *keys, uint64_t *out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, steps, ct, keys, out);
    HP_ALIGNED(ctx, ct, out);
    HksCall c(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, bgv_t ? *bgv_t : 0);
    if (c.rc || (bgv_t && c.plain_ok())) return c.rc;
    if (rotations == 0) return fail(ctx, HP_EINVAL, "rotate_hoisted: no rotations");
    const HksRotations rot = {rotations, steps, conj, keys};
    int rc = rotations_ok(ctx, "rotate_hoisted", rot, nullptr, false);
    if (rc) return rc;
    const size_t n = c.n, E = c.E, nd = c.nd;
    // the output is written while later rotations still read the input
    if ((rc = no_overlap(ctx, "rotate_hoisted", ct, batch * 2 * L * n * 8, out, batch * rotations * 2 * L * n * 8))) return rc;
    if (c.open()) return c.rc;
    size_t pass = std::max<size_t>(1, HOIST_POLYS / batch);   // rotations per pass
    pass = std::min(std::min(pass, rotations), (size_t)HP_HOIST_TABLE_MAX);
    const size_t PP = batch * pass;                            // switched polynomials per pass
    if ((rc = ws_reserve(ctx, (c.digits_words(batch) + padded(PP * L * n) / 8 + c.tail_words(PP)) * 8))) return rc;
    Carver cv(ctx->ws);
    u64 *lifted;
    if ((rc = c.digits(batch, ct + L * n, 2 * L, &lifted, cv))) return rc;
    u64 *moved0 = cv.take(PP * L * n);
    const HksTail t = c.tail(PP, cv);
    for (size_t r0 = 0; r0 < rotations; r0 += pass) {
        const size_t cnt = std::min(pass, rotations - r0), P = batch * cnt;   // this pass: polynomial b * cnt + r
        HpHoistTable ht;
        if ((rc = c.fill(ht, rot, nullptr, r0, cnt))) return rc;
        {   // the moved c0 of every (b, r), for the addend
            ProfScope ps(ctx, "elem");
            for (size_t e0 = 0; e0 < P; e0 += HP_GATHER_TABLE_MAX) {
                const size_t ec = std::min<size_t>(HP_GATHER_TABLE_MAX, P - e0);
                HpGatherTable gt;
                memset(&gt, 0, sizeof(gt));
                for (size_t e = e0; e < e0 + ec; e++) {
                    gt.src[e - e0][0] = ct + (e / cnt) * 2 * L * n;
                    gt.perm[e - e0] = ht.map[e % cnt];
                }
                if ((rc = chk(ctx, hp_launch_gather_many(gt, (u32)ec, (u32)n, (u32)L, moved0 + e0 * L * n, ctx->stream, 1), "cycle / involution")))
                    return rc;
            }
        }
        {
            ProfScope ps(ctx, "ks_inner");
            if ((rc = chk(ctx, hp_launch_hks_inner_hoisted(c.plan->d_limbs, (u32)L, (u32)E, (u32)c.KE, (u32)nd, (u32)alpha, (u32)n, (u32)batch, (u32)cnt,
                                                           lifted, ct + L * n, (u32)(2 * L), ht, t.ks, ctx->stream), "hks_inner_hoisted")))
                return rc;
        }
        if ((rc = c.pdown(P, t))) return rc;
        // out[b][r0 + r]: one launch when the pass holds every rotation, else one per ciphertext (its rotations are adjacent in out)
        const size_t launches = cnt == rotations ? 1 : batch, per = P / launches;
        for (size_t b = 0; b < launches; b++) {
            const Addend add(moved0 + b * per * L * n, L, L, 1);
            if ((rc = c.down(per, t.ks + b * per * 2 * E * n, t.rem + b * per * 2 * L * n, add, out + (b * rotations + r0) * 2 * L * n))) return rc;
        }
    }
    return HP_OK;
}
extern "C" int hp_dev_ckks_rotate_hoisted_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                                 const uint64_t *moduli_ext, size_t batch, size_t rotations, const size_t *steps,
                                                 const unsigned char *conj, const uint64_t *ct, const uint64_t *const *keys, uint64_t *out) {
    return dev_rotate_hoisted_hks(ctx, logn, L, key_L0, k, alpha, moduli_ext, nullptr, batch, rotations, steps, conj, ct, keys, out);
}
extern "C" int hp_dev_ckks_rotate_hoisted_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                              size_t batch, size_t rotations, const size_t *steps, const unsigned char *conj,
                                              const uint64_t *ct, const uint64_t *const *keys, uint64_t *out) {
    return hp_dev_ckks_rotate_hoisted_hks_at(ctx, logn, L, L, k, alpha, moduli_ext, batch, rotations, steps, conj, ct, keys, out);
}

// Diagonal linear transform, double hoisted: out = sum_r diag_r * rot_r(ct) with one key per rotation, the weighted sum formed in the
// extended basis Q P BEFORE ModDown.  Everything after the inner product of a switch is linear in its accumulator, so
//   sum_r diag_r * ModDown(acc_r)  ~  ModDown( sum_r diag_r * acc_r )
// up to the roundings: R of them, each scaled by its diagonal, on the left; ONE on the right.  The flow is that of a single switch of
// `batch` polynomials -- digits, the accumulate launches (k_hks_inner_lintrans, at most one argument table of rotations each, the
// later ones adding to the reduced words of the earlier), finish -- and so is the workspace, whatever `rotations` is: no [b][r] row
// set, no yp / rem per rotation, no moved c0 (the kernel folds (P mod q_i) diag_r move_r(c0) into polynomial 0 of the accumulator,
// which ModDown divides by P exactly: finish runs without an addend).
extern "C" int hp_dev_ckks_lintrans_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                           const uint64_t *moduli_ext, size_t batch, size_t rotations, const size_t *steps,
                                           const unsigned char *conj, const uint64_t *ct, const uint64_t *const *keys,
                                           const uint64_t *const *diags, uint64_t *out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, steps, ct, keys, diags, out);
    HP_ALIGNED(ctx, ct, out);
    HksCall c(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, 0);
    if (c.rc) return c.rc;
    if (rotations == 0) return fail(ctx, HP_EINVAL, "lintrans: no rotations");
    const HksRotations rot = {rotations, steps, conj, keys};
    int rc = rotations_ok(ctx, "lintrans", rot, diags, false);
    if (rc) return rc;
    const size_t n = c.n, E = c.E;
    if ((rc = no_overlap(ctx, "lintrans", ct, batch * 2 * L * n * 8, out, batch * 2 * L * n * 8))) return rc;
    const size_t pass = hks_lintrans_max_rotations(moduli_ext, E, c.nd, HP_HOIST_TABLE_MAX);   // rotations per launch
    if (pass == 0) return fail(ctx, HP_EUNSUPPORTED, "lintrans: moduli too large for the 128-bit accumulators");
    if (c.open()) return c.rc;
    if ((rc = ws_reserve(ctx, c.switch_words(batch) * 8))) return rc;
    Carver cv(ctx->ws);
    u64 *lifted;
    if ((rc = c.digits(batch, ct + L * n, 2 * L, &lifted, cv))) return rc;
    const HksTail t = c.tail(batch, cv);
    for (size_t r0 = 0; r0 < rotations; r0 += pass) {
        const size_t cnt = std::min(pass, rotations - r0);
        HpLinTable ht;
        if ((rc = c.fill(ht, rot, nullptr, r0, cnt))) return rc;
        std::copy(diags + r0, diags + r0 + cnt, ht.diag);
        ProfScope ps(ctx, "ks_inner");
        if ((rc = chk(ctx, hp_launch_hks_inner_lintrans(c.plan->d_limbs, c.he->dev, (u32)E, (u32)c.KE, (u32)n, (u32)batch, (u32)cnt, lifted, ct, ht, r0 != 0,
                                                        t.ks, ctx->stream), "hks_inner_lintrans")))
            return rc;
    }
    return c.finish(batch, t, Addend(), out);
}
extern "C" int hp_dev_ckks_lintrans_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                        size_t batch, size_t rotations, const size_t *steps, const unsigned char *conj, const uint64_t *ct,
                                        const uint64_t *const *keys, const uint64_t *const *diags, uint64_t *out) {
    return hp_dev_ckks_lintrans_hks_at(ctx, logn, L, L, k, alpha, moduli_ext, batch, rotations, steps, conj, ct, keys, diags, out);
}

// Baby-step giant-step form of the diagonal transform: out = sum_g rot_g( sum_i diag_{g,i} * rot_i(ct) ), babies + giants keys for
// babies * giants diagonals.  The linearity argument above, twice: the baby results stay in the extended basis (no ModDown), every
// giant's weighted sum is formed there and pays ONE ModDown, and the giants' switches are summed in the extended basis again before
// the last ModDown.  All giants go through each stage together, as P = batch * (giants that are not the identity) polynomials:
//   1. digits of c1                                          (batch polynomials)
//   2. baby rows [b][i][2][E][N], c0 folded in               (k_hks_inner_lintrans<BABY>, one launch per argument table)
//   3. pre[b][g'][2][E][N] = sum_i diag_{g,i} * baby_i       (k_hks_bsgs_presum; an identity giant's row goes straight into acc)
//   4. finish (pdown + down) of pre -> u[b][g'][2][L][N]     (P polynomials)
//   5. digits of the u1 rows                                 (P polynomials)
//   6. acc[b][2][E][N] (+)= sum_g' switch_g'(u)              (k_hks_inner_lintrans<GIANT>, one launch per argument table)
//   7. finish of acc -> out                                  (batch polynomials)
// The workspace and the pass plan are hpi::hks_bsgs_plan's (hp_drop.h): a function of the shape alone.  The first digit rows and the
// baby rows are dead after stage 3; the digit rows of stage 5 take their place.
extern "C" int hp_dev_ckks_lintrans_bsgs_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                                const uint64_t *moduli_ext, size_t batch, size_t babies, const size_t *baby_steps,
                                                const unsigned char *baby_conj, const uint64_t *const *baby_keys, size_t giants,
                                                const size_t *giant_steps, const unsigned char *giant_conj,
                                                const uint64_t *const *giant_keys, const uint64_t *const *diags, const uint64_t *ct,
                                                uint64_t *out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, baby_steps, baby_keys, giant_steps, giant_keys, diags, ct, out);
    HP_ALIGNED(ctx, ct, out);
    HksCall c(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, 0);
    if (c.rc) return c.rc;
    if (babies == 0 || giants == 0) return fail(ctx, HP_EINVAL, "lintrans_bsgs: no baby steps or no giant steps");
    const HksRotations baby_rot = {babies, baby_steps, baby_conj, baby_keys}, giant_rot = {giants, giant_steps, giant_conj, giant_keys};
    int rc;
    if ((rc = rotations_ok(ctx, "lintrans_bsgs", baby_rot, nullptr, true)) || (rc = rotations_ok(ctx, "lintrans_bsgs", giant_rot, nullptr, true)))
        return rc;
    for (size_t g = 0; g < giants; g++) {
        bool any = false;
        for (size_t i = 0; i < babies; i++) {
            if ((uintptr_t)diags[g * babies + i] & 15u) return fail(ctx, HP_EINVAL, "lintrans_bsgs: misaligned diagonal");
            any = any || diags[g * babies + i];
        }
        if (!any) return fail(ctx, HP_EINVAL, "lintrans_bsgs: a giant step without a diagonal");
    }
    const size_t n = c.n, E = c.E, nd = c.nd;
    if ((rc = no_overlap(ctx, "lintrans_bsgs", ct, batch * 2 * L * n * 8, out, batch * 2 * L * n * 8))) return rc;
    HksBsgsPlan bp;
    if (!hks_bsgs_plan(moduli_ext, n, L, k, alpha, batch, babies, giants, bp))
        return fail(ctx, HP_EUNSUPPORTED, "lintrans_bsgs: moduli too large for the 128-bit accumulators");
    if (c.open()) return c.rc;
    if ((rc = ws_reserve(ctx, bp.words * 8))) return rc;
    std::vector<size_t> keyed;   // the giants that switch, in order: polynomial b * GK + (index here) from stage 3 to stage 6
    for (size_t g = 0; g < giants; g++)
        if (giant_keys[g]) keyed.push_back(g);
    const size_t GK = keyed.size(), rows = 2 * E * n;
    Carver cv(ctx->ws), late(ctx->ws);   // `late`: stage 5's digit rows, over the first digit rows and the baby rows
    u64 *lifted;
    if ((rc = c.digits(batch, ct + L * n, 2 * L, &lifted, cv))) return rc;
    u64 *baby = cv.take(batch * babies * rows);
    cv.off = bp.overlay_words * 8;
    u64 *acc = cv.take(batch * rows), *pre = cv.take(batch * giants * rows), *yp = cv.take(2 * batch * giants * k * n),
        *rem = cv.take(2 * batch * giants * L * n), *u = cv.take(batch * giants * 2 * L * n);
    for (size_t i0 = 0; i0 < babies; i0 += HP_HOIST_TABLE_MAX) {   // stage 2
        const size_t cnt = std::min<size_t>(HP_HOIST_TABLE_MAX, babies - i0);
        HpLinTable ht;
        if ((rc = c.fill(ht, baby_rot, nullptr, i0, cnt))) return rc;
        ProfScope ps(ctx, "ks_inner");
        if ((rc = chk(ctx, hp_launch_hks_bsgs_babies(c.plan->d_limbs, c.he->dev, (u32)E, (u32)c.KE, (u32)n, (u32)batch, (u32)cnt, (u32)babies, lifted, ct, ht,
                                                     baby + i0 * rows, ctx->stream), "hks_bsgs_babies")))
            return rc;
    }
    // stage 3.  A launch holds giants that write DIFFERENT rows: the keyed giants presum_giants at a time into pre, every identity
    // giant alone into acc (two of them in one launch would race on it)
    bool acc_written = false;
    const auto presum = [&](const size_t *gs, size_t gcnt, bool to_acc) {
        for (size_t i0 = 0; i0 < babies; i0 += bp.baby_pass) {
            const size_t cnt = std::min(bp.baby_pass, babies - i0);
            HpPreTable pt;
            memset(&pt, 0, sizeof(pt));
            for (size_t j = 0; j < gcnt; j++) {
                const size_t g = gs[j];
                for (size_t i = 0; i < cnt; i++) pt.diag[j * cnt + i] = diags[g * babies + i0 + i];
                pt.dst[j] = to_acc ? acc : pre + (size_t)(gs + j - keyed.data()) * rows;
            }
            const bool add = to_acc ? acc_written : i0 != 0;
            ProfScope ps(ctx, "ks_inner");
            int e = chk(ctx, hp_launch_hks_bsgs_presum(c.plan->d_limbs, (u32)L, (u32)E, (u32)c.KE, (u32)n, (u32)batch, (u32)gcnt, (u32)cnt, baby + i0 * rows,
                                                       babies * rows, pt, to_acc ? rows : GK * rows, add, ctx->stream), "hks_bsgs_presum");
            if (e) return e;
            if (to_acc) acc_written = true;
        }
        return (int)HP_OK;
    };
    for (size_t g = 0; g < giants; g++)
        if (!giant_keys[g] && (rc = presum(&g, 1, true))) return rc;
    for (size_t c0 = 0; c0 < GK; c0 += bp.presum_giants)
        if ((rc = presum(keyed.data() + c0, std::min(bp.presum_giants, GK - c0), false))) return rc;
    if (GK) {
        const size_t P = batch * GK;
        if ((rc = c.finish(P, {pre, yp, rem}, Addend(), u))) return rc;                                          // stage 4
        u64 *lifted2;
        if ((rc = c.digits(P, u + L * n, 2 * L, &lifted2, late))) return rc;                                     // stage 5
        for (size_t c0 = 0; c0 < GK; c0 += bp.giant_pass) {                                                     // stage 6
            const size_t cnt = std::min(bp.giant_pass, GK - c0);
            HpLinTable ht;
            if ((rc = c.fill(ht, giant_rot, keyed.data(), c0, cnt))) return rc;
            ProfScope ps(ctx, "ks_inner");
            if ((rc = chk(ctx, hp_launch_hks_bsgs_giants(c.plan->d_limbs, c.he->dev, (u32)E, (u32)c.KE, (u32)n, (u32)batch, (u32)cnt, (u32)GK,
                                                         lifted2 + c0 * nd * E * n, u + c0 * 2 * L * n, ht, acc_written, acc, ctx->stream),
                          "hks_bsgs_giants")))
                return rc;
            acc_written = true;
        }
    }
    return c.finish(batch, {acc, yp, rem}, Addend(), out);                                                      // stage 7
}
extern "C" int hp_dev_ckks_lintrans_bsgs_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                             size_t batch, size_t babies, const size_t *baby_steps, const unsigned char *baby_conj,
                                             const uint64_t *const *baby_keys, size_t giants, const size_t *giant_steps,
                                             const unsigned char *giant_conj, const uint64_t *const *giant_keys,
                                             const uint64_t *const *diags, const uint64_t *ct, uint64_t *out) {
    return hp_dev_ckks_lintrans_bsgs_hks_at(ctx, logn, L, L, k, alpha, moduli_ext, batch, babies, baby_steps, baby_conj, baby_keys, giants,
                                            giant_steps, giant_conj, giant_keys, diags, ct, out);
}

// ---- BGV over the hybrid path --------------------------------------------------------------------------------------------------------
// Only ModDown knows the scheme (HksCall::pmod, k_hks_moddown_t; hehub_amd.h has the convention): the switch and the hoisted rotations
// are their CKKS twins with the plain modulus handed on; the multiplications are in hp_api_hks_mult.cpp.
extern "C" int hp_dev_bgv_hks_switch_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                        uint64_t plain_modulus, size_t batch, const uint64_t *pt, const uint64_t *key, uint64_t *out) {
    return dev_hks_switch(ctx, logn, L, key_L0, k, alpha, moduli_ext, &plain_modulus, batch, pt, key, out);
}
extern "C" int hp_dev_bgv_hks_switch(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                     uint64_t plain_modulus, size_t batch, const uint64_t *pt, const uint64_t *key, uint64_t *out) {
    return dev_hks_switch(ctx, logn, L, L, k, alpha, moduli_ext, &plain_modulus, batch, pt, key, out);
}
extern "C" int hp_dev_bgv_rotate_hoisted_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                                const uint64_t *moduli_ext, uint64_t plain_modulus, size_t batch, size_t rotations,
                                                const size_t *steps, const unsigned char *conj, const uint64_t *ct,
                                                const uint64_t *const *keys, uint64_t *out) {
    return dev_rotate_hoisted_hks(ctx, logn, L, key_L0, k, alpha, moduli_ext, &plain_modulus, batch, rotations, steps, conj, ct, keys, out);
}
extern "C" int hp_dev_bgv_rotate_hoisted_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                             uint64_t plain_modulus, size_t batch, size_t rotations, const size_t *steps,
                                             const unsigned char *conj, const uint64_t *ct, const uint64_t *const *keys, uint64_t *out) {
    return dev_rotate_hoisted_hks(ctx, logn, L, L, k, alpha, moduli_ext, &plain_modulus, batch, rotations, steps, conj, ct, keys, out);
}
