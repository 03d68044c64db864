// hp_api_hks.cpp -- C ABI, part 3 (extension): hybrid key switch -- digits of several moduli, several special primes;
// kernels in hp_hks.hip.  Exact integer arithmetic throughout (ModUp / ModDown by mixed-radix composition); keys have
// their own format, so results are pinned by an exact integer model and by decryption, not by hehub's words.
#include "hp_ctx.h"
#include "hp_ntt_job.h"   // item counts

#include <algorithm>
#include <cstring>
#include <optional>
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

// what follows an inner product: its accumulator ks [P][2][E][N] (NTT form), ModDown's scratch yp [2P][k][N], the remainders rem [2P][L][N]
struct HksTail {
    u64 *ks, *yp, *rem;
};
// a list of rotations as the entry points take it; entry r is a conjugation where conj && conj[r], else the cycle by steps[r]
struct HksRotations {
    size_t count;
    const size_t *steps;
    const unsigned char *conj;
    const uint64_t *const *keys;
};

// A hybrid call in progress: the shape, what the caches hold for it and the parity level, as every stage reads them.  Built in two
// steps because every entry point has argument checks of its own between them: the constructor checks the limits all calls share
// (rc), open() fetches the plan and the constants and decides the level, which then holds until the entry point returns.
// key_L0 >= L: the ciphertext moduli the caller's keys (and diagonals) were generated for; the plain entry points are key_L0 == L.
// It reaches the inner-product launches as KE = key_L0 + k, the rows of one key digit, and nothing else: the plan, the constants,
// the workspace, the digit stage and ModDown are those of the level's own chain.
// pmod: the plain modulus of the BGV calls, 0 for CKKS.  It reaches ModDown's conversion kernel (pdown) and nothing else: digits, ModUp,
// the inner products, the transforms and the drops never see the plaintext.
struct HksCall {
    hp_ctx *ctx;
    const uint64_t *mext;
    size_t logn, L, key_L0, k, alpha, n = 0, E = 0, KE = 0, nd = 0;
    uint64_t pmod;
    HpHksPlain plain;   // t != 0: the constants of k_hks_moddown_t, built by open()
    const Plan *plan = nullptr;
    const HksEntry *he = nullptr;
    std::optional<LevelScope> lvl;
    int rc;

    HksCall(hp_ctx *c, size_t logn_, size_t L_, size_t key_L0_, size_t k_, size_t alpha_, const uint64_t *moduli_ext, size_t batch,
            uint64_t plain_modulus)
        : ctx(c), mext(moduli_ext), logn(logn_), L(L_), key_L0(key_L0_), k(k_), alpha(alpha_), pmod(plain_modulus), rc(limits(batch)) {
        if (!rc) n = (size_t)1 << logn, E = L + k, KE = key_L0 + k, nd = (L + alpha - 1) / alpha;
    }
    HksCall(const HksCall &) = delete;   // (one LevelScope per call)
    int limits(size_t batch) const {
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
    int open() {
        if ((rc = get_plan(ctx, logn, mext, E, true, &plan)) || (rc = get_hks_consts(ctx, mext, L, k, alpha, &he))) return rc;
        lvl.emplace(ctx, plan);   // level A: the digit stages (lifted digits, coefficient rows) and the drops on the FP64 kernels
        if (pmod) plain_consts();
        return rc = lvl->rc;
    }
    // What a BGV entry point refuses on top of its CKKS sibling, after the shared limits: t must be invertible modulo every modulus
    // of the chain (they are primes: 0 < t < each of them is enough), and ModDown_t exists as the one-kernel conversion only.
    int plain_ok() {
        if (rc) return rc;
        if (pmod == 0) return rc = fail(ctx, HP_EINVAL, "plain modulus must be positive");
        for (size_t m = 0; m < L + k; m++)
            if (pmod >= mext[m]) return rc = fail(ctx, HP_EINVAL, "plain modulus must be below every modulus of the chain");
        if (k > HP_HKS_MAX_ALPHA) return rc = fail(ctx, HP_EUNSUPPORTED, "more than 8 special primes with a plain modulus");
        return HP_OK;
    }
    void plain_consts() {
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

    // The digit stage of P polynomials pt (NTT form, L limbs, row stride pt_pstride): lifted [P][nd][E][N] = every digit's exact
    // integer, in NTT form, in every modulus outside the digit (the slots inside a digit stay unwritten: there D_d is the input limb
    // itself).  All that depends on the input alone -- a rotation that is applied to these rows afterwards
    // (hp_dev_ckks_rotate_hoisted_hks) shares them with every other rotation.
    size_t digits_words(size_t P) const { return padded(P * L * n) / 8 + padded(P * nd * E * n) / 8; }
    int digits(size_t P, const u64 *pt, size_t pt_pstride, u64 **lifted_out, Carver &cv) const {
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

    size_t tail_words(size_t P) const { return padded(P * 2 * E * n) / 8 + padded(2 * P * k * n) / 8 + padded(2 * P * L * n) / 8; }
    HksTail tail(size_t P, Carver &cv) const { return {cv.take(P * 2 * E * n), cv.take(2 * P * k * n), cv.take(2 * P * L * n)}; }

    // a plain switch up to its inner product: t.ks [P][2][E][N] = sum_d D_d * key_d over the digit rows of pt
    int front(size_t P, const u64 *pt, size_t pt_pstride, const u64 *key, HksTail &t, Carver &cv) const {
        u64 *lifted;
        int e = digits(P, pt, pt_pstride, &lifted, cv);
        if (e) return e;
        t = tail(P, cv);
        ProfScope ps(ctx, "ks_inner");
        return chk(ctx, hp_launch_hks_inner(plan->d_limbs, (u32)L, (u32)E, (u32)KE, (u32)nd, (u32)alpha, (u32)n, (u32)P, lifted, pt, (u32)pt_pstride, key,
                                            t.ks, ctx->stream), "hks_inner");
    }

    // The first half of ModDown: t.rem = the centred exact conversion of the P-part of t.ks into every q_i (coefficient form) --
    // coefficients of the P-part (strict), then the conversion; the transform, the subtraction and * P^-1 are down()'s
    int pdown(size_t P, const HksTail &t) const {
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

    // ModDown of the limbs [i0, i0 + cnt) with the transform of the remainders fused in: out = (ks - NTT(rem)) * P^-1 [+ addend]
    // (level A: the canonical residues of that)
    int down_fused(size_t i0, size_t cnt, size_t P2, const u64 *rem, HpDropArgs &da, bool level_a, const char *what, const char *what_a) const {
        HpNttJob fj = batch_job(plan, logn, cnt, P2, rem + i0 * n, nullptr, L, 0, 0, 0);
        fj.limbs = plan->d_limbs + i0;
        hks_down_consts(he->host, i0, cnt, da);
        ProfScope ps(ctx, "ntt_drop");
        if (!level_a) return chk(ctx, hp_launch_ntt_fast_drop(fj, da, ctx->stream), what);
        fj.limbs_a = plan->d_limbs_a + i0;
        hks_down_consts_a(mext, i0, cnt, da);
        return chk(ctx, hp_launch_ntt_a_drop(fj, da, ctx->stream), what_a);
    }

    // the end of a switch: out [P][2][L][N] = (ks - NTT(rem)) * P^-1 [+ addend rows (p2>>1)*add.ct_stride + (p2&1)*add.poly_stride + i]
    int down(size_t P, const u64 *ks, u64 *rem, const Addend &add, u64 *out) const {
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

    // all of ModDown on the rows of one tail
    int finish(size_t P, const HksTail &t, const Addend &add, u64 *out) const {
        int e = pdown(P, t);
        return e ? e : down(P, t.ks, t.rem, add, out);
    }

    // key switch of P polynomials pt with a hybrid key u64[nd][2][L+k][N]: out [P][2][L][N] = ModDown( sum_d D_d * key_d ) [+ addend]
    size_t switch_words(size_t P) const { return digits_words(P) + tail_words(P); }
    int key_switch(size_t P, const u64 *pt, size_t pt_pstride, const u64 *key, const Addend &add, u64 *out, Carver &cv) const {
        HksTail t;
        int e = front(P, pt, pt_pstride, key, t, cv);
        return e ? e : finish(P, t, add, out);
    }

    // The rotation table of one launch: entries idx[r0 + r] (idx == NULL: r0 + r) of a list, r < cnt.  A conjugation has no map; a NULL
    // key with a NULL map is the identity (the BSGS call's babies only: of its giants the keyed ones come here)
    template <class Table> int fill(Table &ht, const HksRotations &rot, const size_t *idx, size_t r0, size_t cnt) const {
        memset(&ht, 0, sizeof(ht));
        int e = reserve_cycle_perms(ctx, cnt);   // (a miss in a full map cache empties it: not between these)
        for (size_t r = 0; r < cnt && !e; r++) {
            const size_t at = idx ? idx[r0 + r] : r0 + r;
            ht.key[r] = rot.keys[at];
            if (rot.keys[at] && !(rot.conj && rot.conj[at])) e = get_cycle_perm(ctx, logn, rot.steps[at], &ht.map[r]);
        }
        return e;
    }
};

// The entries of a rotation list, and their diagonals where the list has its own (the flat transform).  identity_ok: an entry that is
// the identity (step 0, no conjugation) may have a NULL key.  (The BSGS call has always looked at an entry's step before its key, the
// other calls after: a list that is wrong in two ways reports what it always did.)
static int rotations_ok(hp_ctx *ctx, const char *call, const HksRotations &rot, const uint64_t *const *diags, bool identity_ok) {
    const auto bad = [&](const char *what) { return fail(ctx, HP_EINVAL, std::string(call) + ": " + what); };
    for (size_t r = 0; r < rot.count; r++) {
        const bool cj = rot.conj && rot.conj[r], far = !cj && rot.steps[r] >= ((size_t)1 << 17);
        if (identity_ok && far) return fail(ctx, HP_EINVAL, "rotation step out of range");
        if (!rot.keys[r] && !(identity_ok && !cj && rot.steps[r] == 0))
            return bad(identity_ok ? "a NULL key on an entry that is not the identity" : "NULL or misaligned key");
        if ((uintptr_t)rot.keys[r] & 15u) return bad(identity_ok ? "misaligned key" : "NULL or misaligned key");
        if (diags && ((uintptr_t)diags[r] & 15u)) return bad("misaligned diagonal");
        if (far) return fail(ctx, HP_EINVAL, "rotation step out of range");
    }
    return HP_OK;
}

// the calls that write their output while they still read their input
static int no_overlap(hp_ctx *ctx, const char *call, const void *in, size_t in_bytes, const void *out, size_t out_bytes) {
    const uintptr_t c0 = (uintptr_t)in, o0 = (uintptr_t)out;
    if (o0 < c0 + in_bytes && c0 < o0 + out_bytes) return fail(ctx, HP_EINVAL, std::string(call) + ": the output overlaps the input");
    return HP_OK;
}

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
    if (!conj && step >= ((size_t)1 << 17)) return fail(ctx, HP_EINVAL, "rotation step out of range");
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

// What follows the tensor product of a hybrid multiplication, on an open call: hybrid relinearisation of d2, + (d0, d1), rescale by the
// last ciphertext modulus.  quad [batch][3][L][N], words below 2q: the workspace block of hp_dev_ckks_mult_relin_rescale_hks and
// hp_dev_ckks_dot_relin_rescale_hks, the caller's memory in hp_dev_ckks_relin_rescale_hks -> out [batch][2][L-1][N].  Everything here
// is linear in quad, which is why a sum of products pays it once.
static size_t relin_rescale_words(const HksCall &c, size_t batch) {
    return padded(batch * 2 * c.L * c.n) / 8 + c.switch_words(batch) + drop_ws_words(c.n, c.L, 2 * batch) + 2 * (padded(2 * batch * c.n) / 8);
}
static int relin_rescale(const HksCall &c, size_t batch, const u64 *quad, const u64 *key, u64 *out, Carver &cv) {
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
    {
        ProfScope ps(ctx, "tensor");
        if ((rc = chk(ctx, hp_launch_tensor(c.plan->d_limbs, (u32)L, 0, (u32)L, (u32)n, (u32)batch, ct1, ct2, quad, ctx->stream), "tensor")))
            return rc;
    }
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

// the same tail for a caller inside the engine that already holds the context lock (hp_api_eval.cpp: one per step of a plan)
namespace hpi {
int hks_limits(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t batch) {
    return HksCall(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, 0).rc;
}
int hks_relin_rescale_shape(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext,
                            size_t batch, size_t *ws_words) {
    HksCall c(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, 0);
    if (c.rc) return c.rc;
    if (L < 2) return fail(ctx, HP_EINVAL, "Unable to drop the only one prime.");
    if (c.open()) return c.rc;
    *ws_words = relin_rescale_words(c, batch);
    return HP_OK;
}
int hks_relin_rescale_step(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext,
                           size_t batch, const u64 *quad, const u64 *key, u64 *out, Carver &cv) {
    HksCall c(ctx, logn, L, key_L0, k, alpha, moduli_ext, batch, 0);
    if (c.rc || c.open()) return c.rc;
    return relin_rescale(c, batch, quad, key, out, cv);
}
} // namespace hpi

// ---- sums of products: lazy relinearisation ----------------------------------------------------------------------------------------
// rescale(relin(sum_t a_t (x) b_t)) = rescale(sum_t (d0_t, d1_t) + switch(sum_t d2_t)), residue for residue: T products pay one switch
// and one rounding.  The quadratic sum is one streaming kernel (k_tensor_sum, hp_ks.hip), one launch per argument table.
struct TensorSumTerms {
    size_t terms;
    const uint64_t *const *a, *const *b;   // HOST arrays of device addresses, each u64[batch][2][L][N]
};
// before anything is enqueued: the list itself, and `out` (the call's output, out_bytes long) against every operand
static int tensor_sum_ok(hp_ctx *ctx, const char *call, size_t n, size_t L, size_t batch, const TensorSumTerms &ts, const void *out,
                         size_t out_bytes) {
    const auto bad = [&](const char *what) { return fail(ctx, HP_EINVAL, std::string(call) + ": " + what); };
    if (ts.terms == 0) return bad("no terms");
    // (512 words per workgroup at the least: every launch stays below 2^30 workgroups, and every u32 row count with it)
    if (batch > ((size_t)1 << 30) / (L * ((n + 511) / 512)))
        return fail(ctx, HP_EUNSUPPORTED, std::string(call) + ": too many ciphertexts for one call");
    const size_t in_bytes = batch * 2 * L * n * 8;
    const uintptr_t o0 = (uintptr_t)out;
    for (size_t t = 0; t < ts.terms; t++)
        for (const uint64_t *p : {ts.a[t], ts.b[t]}) {
            if (!p || ((uintptr_t)p & 15u)) return bad("NULL or misaligned operand");
            if (o0 < (uintptr_t)p + in_bytes && (uintptr_t)p < o0 + out_bytes) return bad("the output overlaps an operand");
        }
    return HP_OK;
}
// quad [batch][3][L][N] = the sum over the list, `pass` terms per launch (tensor_sum_max_terms' answer)
static int tensor_sum(hp_ctx *ctx, const HpLimb *limbs, size_t n, size_t L, size_t batch, size_t pass, const TensorSumTerms &ts, u64 *quad) {
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
// Only ModDown knows the scheme (HksCall::pmod, k_hks_moddown_t; hehub_amd.h has the convention): the switch and the hoisted rotations
// are their CKKS twins with the plain modulus handed on, and a multiplication is the tensor product, the switch of d2 with (d0, d1) as
// its addend, then hehub's own mod_drop_one_prime_inplace (drop_last with bgv = true: its q_last mod t factor included) -- the
// two-step composition of relin_rescale above.  ModDown_t and the mod switch are NOT merged into one transform: that path is CKKS's.
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

// quad [batch][3][L][N], words below 2q -> out [batch][2][L-1][N] on an open BGV call; the workspace is relin_rescale_words'
static int bgv_relin_modswitch(const HksCall &c, size_t batch, const u64 *quad, const u64 *key, u64 *out, Carver &cv) {
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
    {
        ProfScope ps(ctx, "tensor");
        if ((rc = chk(ctx, hp_launch_tensor(c.plan->d_limbs, (u32)L, 0, (u32)L, (u32)n, (u32)batch, ct1, ct2, quad, ctx->stream), "tensor")))
            return rc;
    }
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

// ---- key generation ----------------------------------------------------------------------------------------------------------------
// The uniform rows a and the error polynomials e are inputs (the caller's, or the device samplers' in the seeded forms further down);
// what runs here is the arithmetic:
// spread (k_spread_signed) -> one batched forward transform -> one fused multiply-add (k_hks_keygen).  The error rows are spread
// into d_keys[r][d][0] and transformed there in place (a batch job with a polynomial stride of 2E rows); the fused kernel reads each
// word before it overwrites it.  No workspace.
constexpr size_t KEYGEN_MAX_BLOCKS = (size_t)1 << 30;   // workgroups per launch (and, with it, every u32 row count below)
static size_t keygen_chunks(size_t n) { return (n + 2047) / 2048; }   // (ELEM_CHUNK words per workgroup, hp_elem.h)

// small signed polynomials -> NTT form
extern "C" int hp_dev_poly_from_signed(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch, const int64_t *d_coeffs,
                                       uint64_t *d_out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli, d_coeffs, d_out);
    HP_ALIGNED(ctx, d_coeffs, d_out);
    if (!logn_ok(logn)) return fail(ctx, HP_EUNSUPPORTED, HP_LOGN_MSG);
    if (L < 1 || L > HP_MAX_LIMBS) return fail(ctx, HP_EINVAL, "unsupported number of moduli");
    if (batch == 0) return fail(ctx, HP_EINVAL, "empty batch");
    const size_t n = (size_t)1 << logn, chunks = keygen_chunks(n);
    if (batch > KEYGEN_MAX_BLOCKS / (L * chunks)) return fail(ctx, HP_EUNSUPPORTED, "poly_from_signed: too many polynomials for one call");
    int rc = no_overlap(ctx, "poly_from_signed", d_coeffs, batch * n * 8, d_out, batch * L * n * 8);
    if (rc) return rc;
    const Plan *plan;
    if ((rc = get_plan(ctx, logn, moduli, L, true, &plan))) return rc;
    {
        ProfScope ps(ctx, "spread_signed");
        if ((rc = chk(ctx, hp_launch_spread_signed(plan->d_limbs, (u32)L, (u32)n, (u32)batch, (const long long *)d_coeffs, d_out, (u32)L,
                                                   ctx->stream), "spread_signed")))
            return rc;
    }
    return run_ntt(ctx, batch_job(plan, logn, L, batch, d_out, d_out, L, L, 0, 0));   // hp_dev_ntt's launch: its words
}

// rot == NULL: d_from = s_from [keys][E][N]; else the source secret of key r is move_r(d_s_to), read through the rotation's map.
// draw(c, d_e): called once every check has passed and before the generator's first launch; the seeded forms sample there (the
// uniform rows into d_keys[r][d][1], the error rows into workspace, which d_e then names) and the plain forms do nothing.
struct KeygenNoDraw {
    int operator()(const HksCall &, const int64_t *&) const { return HP_OK; }
};
template <class Draw = KeygenNoDraw>
static int dev_hks_keygen(hp_ctx *ctx, const char *call, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *mext, size_t keys,
                          const HksRotations *rot, const uint64_t *d_s_to, const uint64_t *d_from, const uint64_t *d_a, const int64_t *d_e,
                          uint64_t *d_keys, Draw draw = Draw()) {
    HksCall c(ctx, logn, L, L, k, alpha, mext, keys, 0);
    if (c.rc) return c.rc;
    const size_t n = c.n, E = c.E, nd = c.nd, chunks = keygen_chunks(n);
    int rc;
    for (size_t r = 0; rot && r < keys; r++)
        if (!(rot->conj && rot->conj[r]) && rot->steps[r] >= ((size_t)1 << 17)) return fail(ctx, HP_EINVAL, "rotation step out of range");
    if (keys > KEYGEN_MAX_BLOCKS / (nd * 2 * E * chunks)) return fail(ctx, HP_EUNSUPPORTED, std::string(call) + ": too many keys for one call");
    const size_t out_bytes = keys * nd * 2 * E * n * 8;
    if ((rc = no_overlap(ctx, call, d_s_to, E * n * 8, d_keys, out_bytes)) ||
        (d_e && (rc = no_overlap(ctx, call, d_e, keys * nd * n * 8, d_keys, out_bytes))) ||
        (d_from && (rc = no_overlap(ctx, call, d_from, keys * E * n * 8, d_keys, out_bytes))) ||
        (d_a && (rc = no_overlap(ctx, call, d_a, keys * nd * E * n * 8, d_keys, out_bytes))))
        return rc;
    if (c.open()) return c.rc;
    const Plan *plan = c.plan;
    if ((rc = draw(c, d_e))) return rc;
    {
        ProfScope ps(ctx, "spread_signed");
        if ((rc = chk(ctx, hp_launch_spread_signed(plan->d_limbs, (u32)E, (u32)n, (u32)(keys * nd), (const long long *)d_e, d_keys, (u32)(2 * E),
                                                   ctx->stream), "spread_signed")))
            return rc;
    }
    {
        HpNttJob j = batch_job(plan, logn, E, keys * nd, d_keys, d_keys, 2 * E, 2 * E, 0, 0);
        if (ctx->cur_a) j.limbs_a = plan->d_limbs_a;   // strict rows in, any representative out: the FP64 transform where allowed
        if ((rc = run_ntt(ctx, j))) return rc;
    }
    // one launch; a rotation list longer than one argument table: one launch per table
    const size_t pass = rot ? std::min<size_t>(keys, HP_HOIST_TABLE_MAX) : keys;
    for (size_t r0 = 0; r0 < keys; r0 += pass) {
        const size_t cnt = std::min(pass, keys - r0);
        HpKeygenMaps maps;
        memset(&maps, 0, sizeof(maps));
        if (rot) {
            if ((rc = reserve_cycle_perms(ctx, cnt))) return rc;   // (a miss in a full map cache empties it: not between these)
            for (size_t r = 0; r < cnt; r++)
                if (!(rot->conj && rot->conj[r0 + r]) && (rc = get_cycle_perm(ctx, logn, rot->steps[r0 + r], &maps.map[r]))) return rc;
        }
        ProfScope ps(ctx, "hks_keygen");
        if ((rc = chk(ctx, hp_launch_hks_keygen(plan->d_limbs, c.he->dev, (u32)E, (u32)nd, (u32)n, (u32)cnt, d_s_to,
                                                d_from ? d_from + r0 * E * n : nullptr, rot ? &maps : nullptr,
                                                d_a ? d_a + r0 * nd * E * n : nullptr, d_keys + r0 * nd * 2 * E * n, ctx->stream), call)))
            return rc;
    }
    return HP_OK;
}

extern "C" int hp_dev_hks_keygen(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t keys,
                                 const uint64_t *d_s_to, const uint64_t *d_s_from, const uint64_t *d_a, const int64_t *d_e, uint64_t *d_keys) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, d_s_to, d_s_from, d_e, d_keys);
    HP_ALIGNED(ctx, d_s_to, d_s_from, d_a, d_e, d_keys);
    return dev_hks_keygen(ctx, "hks_keygen", logn, L, k, alpha, moduli_ext, keys, nullptr, d_s_to, d_s_from, d_a, d_e, d_keys);
}

// the key that switches move_r(s) back to s: what hp_dev_ckks_rotate_hks and its kin apply to a ciphertext rotated by the same entry
extern "C" int hp_dev_hks_keygen_rot(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t keys,
                                     const size_t *steps, const unsigned char *conj, const uint64_t *d_s, const uint64_t *d_a,
                                     const int64_t *d_e, uint64_t *d_keys) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, steps, d_s, d_e, d_keys);
    HP_ALIGNED(ctx, d_s, d_a, d_e, d_keys);
    const HksRotations rot = {keys, steps, conj, nullptr};
    return dev_hks_keygen(ctx, "hks_keygen_rot", logn, L, k, alpha, moduli_ext, keys, &rot, d_s, nullptr, d_a, d_e, d_keys);
}

// ---- device sampling (kernels in hp_sample.hip, the stream layout in hp_sample.h) ---------------------------------------------------------
// Everything is a function of (seed, stream): ChaCha20 blocks of 8 words, one thread each.  The seeded key generators are the plain
// ones after two sampler launches -- the uniform rows straight into the keys' [1] halves (the stride form of the uniform sampler),
// the error rows into workspace -- so a seeded key is word for word the key hp_dev_hks_keygen writes for those rows.
static int sample_logn_ok(hp_ctx *ctx, size_t logn) {
    return (logn >= 3 && logn_ok(logn)) ? (int)HP_OK : fail(ctx, HP_EINVAL, "sampling: ring degrees 2^3 .. 2^16 are supported");
}
static int sample_rows(hp_ctx *ctx, size_t L, const uint64_t *moduli, const uint32_t *limb_ids, HpSampleRows &rows) {
    memset(&rows, 0, sizeof(rows));
    for (size_t m = 0; m < L; m++) {
        if (moduli[m] < 2 || moduli[m] >> 63) return fail(ctx, HP_EINVAL, "sampling: a modulus must be at least 2 and below 2^63");
        if (limb_ids && limb_ids[m] >= HP_SAMPLE_MAX_LIMB_ID) return fail(ctx, HP_EINVAL, "sampling: a limb id must be below 256");
        rows.q[m] = moduli[m];
        rows.id[m] = (unsigned char)(limb_ids ? limb_ids[m] : m);
    }
    return HP_OK;
}
// the largest number of rows of n words one sampler launch takes
static size_t sample_max_rows(size_t n) { return (size_t)(HP_SAMPLE_MAX_BLOCKS * 256 * 8 / n); }

extern "C" int hp_dev_sample_uniform(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, const uint32_t *limb_ids, size_t batch,
                                     const uint8_t *seed, uint64_t stream, size_t stride_words, uint64_t *d_out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli, seed, d_out);
    HP_ALIGNED(ctx, d_out);
    int rc = sample_logn_ok(ctx, logn);
    if (rc) return rc;
    if (L < 1 || L > HP_MAX_LIMBS) return fail(ctx, HP_EINVAL, "unsupported number of moduli");
    if (batch == 0) return fail(ctx, HP_EINVAL, "empty batch");
    const size_t n = (size_t)1 << logn;
    if (stride_words && (stride_words < L * n || (stride_words & 1))) return fail(ctx, HP_EINVAL, "sample_uniform: the stride must be even and at least L * N words");
    HpSampleRows rows;
    if ((rc = sample_rows(ctx, L, moduli, limb_ids, rows))) return rc;
    if (batch > sample_max_rows(n) / L) return fail(ctx, HP_EUNSUPPORTED, "sample_uniform: too many polynomials for one call");
    ProfScope ps(ctx, "sample_uniform");
    return chk(ctx, hp_launch_sample_uniform(hp_sample_seed(seed), rows, nullptr, (u32)L, (u32)logn, batch, stream,
                                             stride_words ? stride_words : L * n, d_out, ctx->stream), "sample_uniform");
}

static int dev_sample_signed(hp_ctx *ctx, u32 kind, const char *call, size_t logn, size_t batch, const uint8_t *seed, uint64_t stream,
                             int64_t *d_out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, seed, d_out);
    HP_ALIGNED(ctx, d_out);
    int rc = sample_logn_ok(ctx, logn);
    if (rc) return rc;
    if (batch == 0) return fail(ctx, HP_EINVAL, "empty batch");
    if (batch > sample_max_rows((size_t)1 << logn)) return fail(ctx, HP_EUNSUPPORTED, std::string(call) + ": too many polynomials for one call");
    ProfScope ps(ctx, call);
    return chk(ctx, hp_launch_sample_signed(kind, hp_sample_seed(seed), (u32)logn, batch, stream, 1, (long long *)d_out, ctx->stream), call);
}
extern "C" int hp_dev_sample_ternary(hp_ctx *ctx, size_t logn, size_t batch, const uint8_t *seed, uint64_t stream, int64_t *d_out) {
    return dev_sample_signed(ctx, HP_SAMPLE_TERNARY, "sample_ternary", logn, batch, seed, stream, d_out);
}
extern "C" int hp_dev_sample_cbd(hp_ctx *ctx, size_t logn, size_t batch, const uint8_t *seed, uint64_t stream, int64_t *d_out) {
    return dev_sample_signed(ctx, HP_SAMPLE_CBD, "sample_cbd", logn, batch, seed, stream, d_out);
}

// the a rows of a key set from the seed: key r, digit d has the polynomial id stream + r * dnum + d and the limb ids 0 .. E-1.
// mont: times 2^64 mod q_m, the finished [1] halves (hp_dev_hks_key_expand); else plain, for the generator to convert in place
static int sample_key_rows(const HksCall &c, size_t keys, const uint8_t *seed, uint64_t stream, bool mont, uint64_t *d_keys) {
    HpSampleRows rows;
    int rc = sample_rows(c.ctx, c.E, c.mext, nullptr, rows);
    if (rc) return rc;
    ProfScope ps(c.ctx, "sample_uniform");
    return chk(c.ctx, hp_launch_sample_uniform(hp_sample_seed(seed), rows, mont ? c.plan->d_limbs : nullptr, (u32)c.E, (u32)c.logn, keys * c.nd,
                                               stream, 2 * c.E * c.n, d_keys + c.E * c.n, c.ctx->stream), "sample_uniform");
}

// what the seeded calls refuse on top of the plain ones (before them: a ring degree below 8 has no whole block)
static int seeded_ok(hp_ctx *ctx, size_t logn, size_t keys, const uint8_t *seed, uint64_t error_scale) {
    HP_REQUIRE(ctx, seed);
    int rc = sample_logn_ok(ctx, logn);
    if (rc) return rc;
    if (keys == 0) return fail(ctx, HP_EINVAL, "empty batch");
    if (error_scale == 0 || error_scale >= HP_SAMPLE_MAX_SCALE) return fail(ctx, HP_EINVAL, "error_scale must be positive and below 2^58");
    return HP_OK;
}
// the draw of a seeded generator: a into the [1] halves, error_scale * e into workspace (i64[keys][dnum][N]: a function of
// (N, dnum, keys) alone)
struct KeygenSeededDraw {
    size_t keys;
    const uint8_t *seed;
    uint64_t stream, error_scale;
    uint64_t *d_keys;
    int operator()(const HksCall &c, const int64_t *&d_e) const {
        int rc = ws_reserve(c.ctx, padded(keys * c.nd * c.n));
        if (rc) return rc;
        Carver cv(c.ctx->ws);
        long long *e = (long long *)cv.take(keys * c.nd * c.n);
        if ((rc = sample_key_rows(c, keys, seed, stream, false, d_keys))) return rc;
        d_e = (const int64_t *)e;
        ProfScope ps(c.ctx, "sample_cbd");
        return chk(c.ctx, hp_launch_sample_signed(HP_SAMPLE_CBD, hp_sample_seed(seed), (u32)c.logn, keys * c.nd, stream, (long long)error_scale, e,
                                                  c.ctx->stream), "sample_cbd");
    }
};

extern "C" int hp_dev_hks_keygen_seeded(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t keys,
                                        const uint64_t *d_s_to, const uint64_t *d_s_from, const uint8_t *seed, uint64_t stream,
                                        uint64_t error_scale, uint64_t *d_keys) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, d_s_to, d_s_from, d_keys);
    HP_ALIGNED(ctx, d_s_to, d_s_from, d_keys);
    int rc = seeded_ok(ctx, logn, keys, seed, error_scale);
    if (rc) return rc;
    return dev_hks_keygen(ctx, "hks_keygen_seeded", logn, L, k, alpha, moduli_ext, keys, nullptr, d_s_to, d_s_from, nullptr, nullptr, d_keys,
                          KeygenSeededDraw{keys, seed, stream, error_scale, d_keys});
}

extern "C" int hp_dev_hks_keygen_rot_seeded(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t keys,
                                            const size_t *steps, const unsigned char *conj, const uint64_t *d_s, const uint8_t *seed,
                                            uint64_t stream, uint64_t error_scale, uint64_t *d_keys) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, steps, d_s, d_keys);
    HP_ALIGNED(ctx, d_s, d_keys);
    int rc = seeded_ok(ctx, logn, keys, seed, error_scale);
    if (rc) return rc;
    const HksRotations rot = {keys, steps, conj, nullptr};
    return dev_hks_keygen(ctx, "hks_keygen_rot_seeded", logn, L, k, alpha, moduli_ext, keys, &rot, d_s, nullptr, nullptr, nullptr, d_keys,
                          KeygenSeededDraw{keys, seed, stream, error_scale, d_keys});
}

// a key set kept as its [0] halves and (seed, stream): the [1] halves again, the [0] halves as the caller loaded them
extern "C" int hp_dev_hks_key_expand(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t keys,
                                     const uint8_t *seed, uint64_t stream, uint64_t *d_keys) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, d_keys);
    HP_ALIGNED(ctx, d_keys);
    int rc = seeded_ok(ctx, logn, keys, seed, 1);
    if (rc) return rc;
    HksCall c(ctx, logn, L, L, k, alpha, moduli_ext, keys, 0);
    if (c.rc) return c.rc;
    if (keys > KEYGEN_MAX_BLOCKS / (c.nd * 2 * c.E * keygen_chunks(c.n))) return fail(ctx, HP_EUNSUPPORTED, "hks_key_expand: too many keys for one call");
    if (c.open()) return c.rc;
    return sample_key_rows(c, keys, seed, stream, true, d_keys);
}

// ---- fresh ciphertexts from a seed (kernels in hp_sample.hip) ---------------------------------------------------------------------------
// The small polynomials (errors, the public-key form's u) go from the keystream straight to the residues of every modulus
// (k_sample_spread) and through the batched forward transform where the ciphertext will lie; one fused kernel then finishes the
// rows.  The transforms are the level-B launches at either parity level and the last kernel reduces to the canonical residue, so
// the words do not depend on the level.
static const char *ENC_SCALE_MSG = "the scale must be positive and below 2^58";

// what the three calls refuse alike, before their own checks; polys = the small polynomials of the call's largest spread launch
static int enc_seeded_ok(hp_ctx *ctx, const char *call, size_t logn, size_t L, const uint64_t *moduli, size_t batch, size_t polys,
                         uint64_t scale, HpSampleRows &rows) {
    int rc = sample_logn_ok(ctx, logn);
    if (rc) return rc;
    if (L < 1 || L > HP_MAX_LIMBS) return fail(ctx, HP_EINVAL, "unsupported number of moduli");
    if (batch == 0) return fail(ctx, HP_EINVAL, "empty batch");
    if (scale == 0 || scale >= HP_SAMPLE_MAX_SCALE) return fail(ctx, HP_EINVAL, ENC_SCALE_MSG);
    if ((rc = sample_rows(ctx, L, moduli, nullptr, rows))) return rc;
    const size_t n = (size_t)1 << logn;
    if (polys > std::min(sample_max_rows(n), KEYGEN_MAX_BLOCKS / keygen_chunks(n)) / L)
        return fail(ctx, HP_EUNSUPPORTED, std::string(call) + ": too many polynomials for one call");
    return HP_OK;
}
// `polys` small polynomials (ids stream + p * id_step) as residues into the rows dst + p * pstride_rows * N, transformed in place
static int small_ntt_rows(hp_ctx *ctx, const Plan *plan, const HpSampleRows &rows, u32 kind, size_t logn, size_t L, size_t polys,
                          const uint8_t *seed, uint64_t stream, uint64_t id_step, uint64_t scale, size_t pstride_rows, u64 *dst) {
    int rc;
    {
        ProfScope ps(ctx, "sample_spread");
        if ((rc = chk(ctx, hp_launch_sample_spread(kind, hp_sample_seed(seed), rows, (u32)L, (u32)logn, polys, stream, id_step, (long long)scale,
                                                   pstride_rows << logn, dst, ctx->stream), "sample_spread")))
            return rc;
    }
    return run_ntt(ctx, batch_job(plan, logn, L, polys, dst, dst, pstride_rows, pstride_rows, 0, 0));
}

extern "C" int hp_dev_sample_small_ntt(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch, uint32_t kind,
                                       const uint8_t *seed, uint64_t stream, uint64_t scale, uint64_t *d_out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli, seed, d_out);
    HP_ALIGNED(ctx, d_out);
    if (kind != HP_SAMPLE_TERNARY && kind != HP_SAMPLE_CBD) return fail(ctx, HP_EINVAL, "sample_small_ntt: kind is 2 (ternary) or 3 (centred binomial)");
    HpSampleRows rows;
    int rc = enc_seeded_ok(ctx, "sample_small_ntt", logn, L, moduli, batch, batch, scale, rows);
    if (rc) return rc;
    const Plan *plan;
    if ((rc = get_plan(ctx, logn, moduli, L, true, &plan))) return rc;
    if ((rc = small_ntt_rows(ctx, plan, rows, kind, logn, L, batch, seed, stream, 1, scale, L, d_out))) return rc;
    ProfScope ps(ctx, "elem");
    return chk(ctx, hp_launch_sample_canonical(plan->d_limbs, (u32)L, (u32)1 << logn, (u32)(batch * L), d_out, ctx->stream), "sample_canonical");
}

extern "C" int hp_dev_rlwe_encrypt_seeded(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch, const uint64_t *d_sk,
                                          const uint64_t *d_pt, const uint8_t *seed, uint64_t stream, uint64_t error_scale, int with_c1,
                                          uint64_t *d_ct) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli, seed, d_sk, d_ct);
    HP_ALIGNED(ctx, d_sk, d_pt, d_ct);
    if (with_c1 != 0 && with_c1 != 1) return fail(ctx, HP_EINVAL, "rlwe_encrypt_seeded: with_c1 is 0 or 1");
    HpSampleRows rows;
    int rc = enc_seeded_ok(ctx, "rlwe_encrypt_seeded", logn, L, moduli, batch, batch, error_scale, rows);
    if (rc) return rc;
    const size_t n = (size_t)1 << logn, ct_rows = (with_c1 ? 2 : 1) * L, ct_bytes = batch * ct_rows * n * 8;
    if ((rc = no_overlap(ctx, "rlwe_encrypt_seeded", d_sk, L * n * 8, d_ct, ct_bytes)) ||
        (d_pt && (rc = no_overlap(ctx, "rlwe_encrypt_seeded", d_pt, batch * L * n * 8, d_ct, ct_bytes))))
        return rc;
    const Plan *plan;
    if ((rc = get_plan(ctx, logn, moduli, L, true, &plan))) return rc;
    // NTT(pt): into the c1 rows where the ciphertext has them (k_enc_seeded reads a word before it stores a over it), else workspace
    u64 *ptn = nullptr;
    size_t pt_rows = 0;
    if (d_pt && with_c1) {
        ptn = d_ct + L * n;
        pt_rows = 2 * L;
    } else if (d_pt) {
        if ((rc = ws_reserve(ctx, padded(batch * L * n)))) return rc;
        ptn = Carver(ctx->ws).take(batch * L * n);
        pt_rows = L;
    }
    if ((rc = small_ntt_rows(ctx, plan, rows, HP_SAMPLE_CBD, logn, L, batch, seed, stream, 1, error_scale, ct_rows, d_ct))) return rc;
    if (d_pt && (rc = run_ntt(ctx, batch_job(plan, logn, L, batch, d_pt, ptn, L, pt_rows, 0, 0)))) return rc;
    ProfScope ps(ctx, "enc_seeded");
    return chk(ctx, hp_launch_enc_seeded(hp_sample_seed(seed), rows, plan->d_limbs, (u32)L, (u32)logn, batch, stream, d_sk, ptn, pt_rows * n,
                                         with_c1 != 0, d_ct, ctx->stream), "enc_seeded");
}

extern "C" int hp_dev_rlwe_encrypt_pk_seeded(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch, const uint64_t *d_pk,
                                             const uint64_t *d_pt, const uint8_t *seed, uint64_t stream, uint64_t error_scale, uint64_t *d_ct) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli, seed, d_pk, d_ct);
    HP_ALIGNED(ctx, d_pk, d_pt, d_ct);
    HpSampleRows rows;
    int rc = enc_seeded_ok(ctx, "rlwe_encrypt_pk_seeded", logn, L, moduli, batch, 2 * batch, error_scale, rows);
    if (rc) return rc;
    const size_t n = (size_t)1 << logn, ct_bytes = batch * 2 * L * n * 8;
    if ((rc = no_overlap(ctx, "rlwe_encrypt_pk_seeded", d_pk, 2 * L * n * 8, d_ct, ct_bytes)) ||
        (d_pt && (rc = no_overlap(ctx, "rlwe_encrypt_pk_seeded", d_pt, batch * L * n * 8, d_ct, ct_bytes))))
        return rc;
    const Plan *plan;
    if ((rc = get_plan(ctx, logn, moduli, L, true, &plan))) return rc;
    if ((rc = ws_reserve(ctx, (d_pt ? 2 : 1) * padded(batch * L * n)))) return rc;
    Carver cv(ctx->ws);
    u64 *u = cv.take(batch * L * n), *ptn = d_pt ? cv.take(batch * L * n) : nullptr;
    // e0_b, e1_b: the ids stream + 2b, stream + 2b + 1 -- the 2 * batch polynomials of d_ct in order; u_b: the ternary sample of stream + 2b
    if ((rc = small_ntt_rows(ctx, plan, rows, HP_SAMPLE_CBD, logn, L, 2 * batch, seed, stream, 1, error_scale, L, d_ct)) ||
        (rc = small_ntt_rows(ctx, plan, rows, HP_SAMPLE_TERNARY, logn, L, batch, seed, stream, 2, 1, L, u)))
        return rc;
    if (d_pt && (rc = run_ntt(ctx, batch_job(plan, logn, L, batch, d_pt, ptn, L, L, 0, 0)))) return rc;
    ProfScope ps(ctx, "enc_pk_fin");
    return chk(ctx, hp_launch_enc_pk_fin(plan->d_limbs, (u32)L, (u32)n, (u32)batch, d_pk, u, ptn, d_ct, ctx->stream), "enc_pk_fin");
}
