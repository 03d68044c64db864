// hp_api_hks.cpp -- C ABI, part 3 (extension): hybrid key switch -- digits of several moduli, several special primes;
// kernels in hp_hks.hip.  Exact integer arithmetic throughout (ModUp / ModDown by mixed-radix composition); keys have
// their own format, so results are pinned by an exact integer model and by decryption, not by hehub's words.
#include "hp_ctx.h"

#include <algorithm>
#include <cstring>
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

static size_t hks_ws_words(size_t n, size_t L, size_t k, size_t nd, size_t P) {
    const size_t E = L + k;
    return padded(P * L * n) / 8 + padded(P * nd * E * n) / 8 + padded(P * 2 * E * n) / 8 + padded(2 * P * k * n) / 8 +
           padded(2 * P * L * n) / 8;
}

// key switch of P polynomials pt (NTT form, L limbs, row stride pt_pstride) with a hybrid key u64[nd][2][L+k][N]:
// out [P][2][L][N] = ModDown( sum_d D_d * key_d ) [+ addend rows (p2>>1)*add_ct_stride + (p2&1)*add_poly_stride + i]
// The digit stage: lifted [P][nd][E][N] = every digit's exact integer, in NTT form, in every modulus outside the digit (the slots
// inside a digit stay unwritten: there D_d is the input limb itself).  All that depends on the input alone -- a rotation that
// is applied to these rows afterwards (hp_dev_ckks_rotate_hoisted_hks) shares them with every other rotation.
static int hks_digits(hp_ctx *ctx, const Plan *plan, const HpHksConsts *hc, size_t logn, size_t L, size_t k, size_t alpha, size_t P,
                      const u64 *pt, size_t pt_pstride, u64 **lifted_out, Carver &cv) {
    const size_t n = (size_t)1 << logn, E = L + k, nd = (L + alpha - 1) / alpha;
    u64 *coef = cv.take(P * L * n), *lifted = cv.take(P * nd * E * n);
    *lifted_out = lifted;
    int rc;
    // coefficients of the input, strictly reduced (as rgsw.cpp:103-105)
    if ((rc = ks_coef(ctx, plan, logn, L, P, 0, L, pt, pt_pstride, coef))) return rc;
    {   // ModUp: every digit's exact integer into every modulus outside the digit
        ProfScope ps(ctx, "hks_modup");
        if ((rc = chk(ctx, hp_launch_hks_modup(plan->d_limbs, hc, (u32)alpha, (u32)nd, (u32)n, (u32)P, coef, lifted, ctx->stream), "hks_modup")))
            return rc;
    }
    // transforms of the lifted limbs, in place
    HpNttJob j;
    memset(&j, 0, sizeof(j));
    j.limbs = plan->d_limbs; j.src = lifted; j.dst = lifted; j.logn = (u32)logn; j.L = (u32)L; j.P = (u32)P;
    j.hks_nd = (u32)nd; j.hks_E = (u32)E; j.hks_alpha = (u32)alpha; j.mode = HP_NTT_HKS;
    j.W = (u32)(L * (nd - 1) * P + k * nd * P);
    // parity level A: the lifted rows are canonical residues (ModUp's exact conversion), the inner product takes any
    // representative, and hybrid results have no word-level contract with hehub (other keys): the FP64 transform where allowed
    if (ctx->cur_a) j.limbs_a = plan->d_limbs_a;
    return run_ntt(ctx, j);
}

// The rest, after the inner product ks [P][2][E][N] = sum_d D_d * key_d (NTT form): rem [2P][L][N] = the centred exact conversion
// of its P-part into every q_i (coefficient form); yp [2P][k][N] is scratch
static int hks_pdown(hp_ctx *ctx, const Plan *plan, const HpHksConsts *hc, size_t logn, size_t L, size_t k, size_t P, const u64 *ks,
                     const uint64_t *mext, u64 *yp, u64 *rem) {
    const size_t n = (size_t)1 << logn, E = L + k;
    int rc;
    // ModDown: coefficients of the P-part (strict), centred exact conversion into every q_i, transform, subtract, * P^-1
    {
        HpNttJob j = batch_job(plan, logn, k, 2 * P, ks + L * n, yp, E, k, 1, 1);
        j.limbs = plan->d_limbs + L;
        if (ctx->cur_a) j.limbs_a = plan->d_limbs_a + L;   // (strict either way: the same words)
        if ((rc = run_ntt(ctx, j))) return rc;
    }
    if (k <= HP_HKS_MAX_ALPHA) {
        ProfScope ps(ctx, "hks_moddown");
        if ((rc = chk(ctx, hp_launch_hks_moddown(plan->d_limbs, hc, (u32)k, (u32)n, (u32)(2 * P), yp, rem, ctx->stream), "hks_moddown")))
            return rc;
    } else {   // many special primes: one composition per target modulus (hp_edge.hip)
        const Plan *pplan;
        if ((rc = get_plan(ctx, 0, mext + L, k, false, &pplan))) return rc;
        for (size_t i = 0; i < L; i++) {
            const HpCrtConsts *cc;
            if ((rc = get_crt_consts(ctx, mext + L, k, mext[i], &cc))) return rc;
            ProfScope ps(ctx, "hks_moddown");
            if ((rc = chk(ctx, hp_launch_base_to_single_crt(pplan->d_limbs, cc, (u32)k, (u32)n, (u32)(2 * P), yp, rem + i * n, (u32)L,
                                                            nullptr, ctx->stream), "hks_moddown")))
                return rc;
        }
    }
    return HP_OK;
}

// the two halves around the plain inner product: ks [P][2][E][N] and rem [2P][L][N] of one key
static int hks_front(hp_ctx *ctx, const Plan *plan, const HpHksConsts *hc, size_t logn, size_t L, size_t k, size_t alpha, size_t P,
                     const u64 *pt, size_t pt_pstride, const u64 *key, const uint64_t *mext, u64 **ks_out, u64 **rem_out, Carver &cv) {
    const size_t n = (size_t)1 << logn, E = L + k, nd = (L + alpha - 1) / alpha;
    u64 *lifted;
    int rc;
    if ((rc = hks_digits(ctx, plan, hc, logn, L, k, alpha, P, pt, pt_pstride, &lifted, cv))) return rc;
    u64 *ks = cv.take(P * 2 * E * n), *yp = cv.take(2 * P * k * n), *rem = cv.take(2 * P * L * n);
    *ks_out = ks; *rem_out = rem;
    {
        ProfScope ps(ctx, "ks_inner");
        if ((rc = chk(ctx, hp_launch_hks_inner(plan->d_limbs, (u32)L, (u32)E, (u32)nd, (u32)alpha, (u32)n, (u32)P, lifted, pt, (u32)pt_pstride,
                                               key, ks, ctx->stream), "hks_inner")))
            return rc;
    }
    return hks_pdown(ctx, plan, hc, logn, L, k, P, ks, mext, yp, rem);
}

// Parity level A for the drops that end a hybrid key switch (round 6; DESIGN section 7 item 1 of round 5): the FP64 drop kernels of
// hp_ntt_a.hip take them as they are -- their compile-time flavours 1 / 2 / 5 (no addend / addend on both polynomials / on polynomial 0)
// for ModDown, flavour 6 (two drops in one transform) for ModDown merged with the rescale.  What differs from hehub's drops is only
// that the transform's input rows already ARE the per-limb remainders (hp_drop.h: a_raw_rows).
static bool a_drop_shape(const Addend &add) { return add.mask == 0 || add.mask == 3u || add.mask == 1u; }

// ModDown of the limbs [i0, i0 + cnt) with the transform of the remainders fused in: out = (ks - NTT(rem)) * P^-1 [+ addend]
// (level A: the canonical residues of that)
static int hks_down_fused(hp_ctx *ctx, const Plan *plan, const HksEntry *he, size_t logn, size_t L, size_t i0, size_t cnt, size_t P2,
                          const u64 *rem, HpDropArgs &da, bool level_a, const uint64_t *mext, const char *what, const char *what_a) {
    HpNttJob fj = batch_job(plan, logn, cnt, P2, rem + i0 * ((size_t)1 << logn), nullptr, L, 0, 0, 0);
    fj.limbs = plan->d_limbs + i0;
    hks_down_consts(he->host, i0, cnt, da);
    ProfScope ps(ctx, "ntt_drop");
    if (!level_a) return chk(ctx, hp_launch_ntt_fast_drop(fj, da, ctx->stream), what);
    fj.limbs_a = plan->d_limbs_a + i0;
    hks_down_consts_a(mext, i0, cnt, da);
    return chk(ctx, hp_launch_ntt_a_drop(fj, da, ctx->stream), what_a);
}

// the end of a switch: out [P][2][L][N] = (ks - NTT(rem)) * P^-1 [+ addend]
static int hks_down(hp_ctx *ctx, const Plan *plan, const HksEntry *he, size_t logn, size_t L, size_t k, size_t P, const u64 *ks, u64 *rem,
                    const Addend &add, const uint64_t *mext, u64 *out) {
    const size_t n = (size_t)1 << logn, E = L + k;
    int rc;
    if (fused_drop_ok(ctx, logn)) {
        HpDropArgs da = drop_args(ks, E, add, out, L);
        return hks_down_fused(ctx, plan, he, logn, L, 0, L, 2 * P, rem, da, ctx->cur_a && a_drop_shape(add), mext, "hks fused ModDown",
                              "hks fused ModDown (level A)");
    }
    if ((rc = run_ntt(ctx, batch_job(plan, logn, L, 2 * P, rem, rem, L, L, 0, 0)))) return rc;
    ProfScope ps(ctx, "hks_down_fin");
    return chk(ctx, hp_launch_hks_down_fin(plan->d_limbs, he->dev, (u32)L, (u32)n, (u32)(2 * P), ks, rem, add.rows, add.poly_stride,
                                           add.ct_stride, add.mask, out, ctx->stream), "hks_down_fin");
}

static int hks_switch(hp_ctx *ctx, const Plan *plan, const HksEntry *he, size_t logn, size_t L, size_t k, size_t alpha, size_t P,
                      const u64 *pt, size_t pt_pstride, const u64 *key, const Addend &add, const uint64_t *mext, u64 *out, Carver &cv) {
    u64 *ks, *rem;
    int rc;
    if ((rc = hks_front(ctx, plan, he->dev, logn, L, k, alpha, P, pt, pt_pstride, key, mext, &ks, &rem, cv))) return rc;
    return hks_down(ctx, plan, he, logn, L, k, P, ks, rem, add, mext, out);
}

static int hks_args_ok(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, size_t batch) {
    if (!logn_ok(logn)) return fail(ctx, HP_EUNSUPPORTED, HP_LOGN_MSG);
    if (L < 1 || k < 1 || k > HP_CRT_MAX_LIMBS || L + k > HP_MAX_LIMBS) return fail(ctx, HP_EINVAL, "unsupported number of moduli");
    if (alpha < 1 || alpha > HP_HKS_MAX_ALPHA || (L + alpha - 1) / alpha > HP_HKS_MAX_DIGITS)
        return fail(ctx, HP_EINVAL, "unsupported digit size");
    if (batch == 0) return fail(ctx, HP_EINVAL, "empty batch");
    return HP_OK;
}

extern "C" int hp_dev_hks_switch(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t batch,
                      const uint64_t *pt, const uint64_t *key, uint64_t *out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, pt, key, out);
    HP_ALIGNED(ctx, pt, key, out);
    int rc = hks_args_ok(ctx, logn, L, k, alpha, batch);
    if (rc) return rc;
    const Plan *plan;
    if ((rc = get_plan(ctx, logn, moduli_ext, L + k, true, &plan))) return rc;
    const HksEntry *he;
    if ((rc = get_hks_consts(ctx, moduli_ext, L, k, alpha, &he))) return rc;
    LevelScope lvl(ctx, plan);   // level A: the transforms of the lifted digits and the coefficient rows on the FP64 kernels
    if (lvl.rc) return lvl.rc;
    const size_t n = (size_t)1 << logn, nd = (L + alpha - 1) / alpha;
    if ((rc = ws_reserve(ctx, hks_ws_words(n, L, k, nd, batch) * 8))) return rc;
    Carver cv(ctx->ws);
    return hks_switch(ctx, plan, he, logn, L, k, alpha, batch, pt, L, key, Addend(), moduli_ext, out, cv);
}

// ckks rotate / conjugate with a hybrid key: moved = gather(ct); out = hks_switch(moved[1]); out[0] += moved[0]
static int dev_hks_automorphism(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *mext, size_t batch,
                                bool conj, size_t step, const uint64_t *ct, const uint64_t *key, uint64_t *out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, mext, ct, key, out);
    HP_ALIGNED(ctx, ct, key, out);
    int rc = hks_args_ok(ctx, logn, L, k, alpha, batch);
    if (rc) return rc;
    if (!conj && step >= ((size_t)1 << 17)) return fail(ctx, HP_EINVAL, "rotation step out of range");
    const Plan *plan;
    if ((rc = get_plan(ctx, logn, mext, L + k, true, &plan))) return rc;
    const HksEntry *he;
    if ((rc = get_hks_consts(ctx, mext, L, k, alpha, &he))) return rc;
    LevelScope lvl(ctx, plan);
    if (lvl.rc) return lvl.rc;
    const size_t n = (size_t)1 << logn, nd = (L + alpha - 1) / alpha;
    if ((rc = ws_reserve(ctx, (padded(batch * 2 * L * n) / 8 + hks_ws_words(n, L, k, nd, batch)) * 8))) return rc;
    Carver cv(ctx->ws);
    u64 *moved = cv.take(batch * 2 * L * n);
    if ((rc = move_rows(ctx, logn, batch * 2 * L, conj, step, ct, moved))) return rc;
    return hks_switch(ctx, plan, he, logn, L, k, alpha, batch, moved + L * n, 2 * L, key, Addend(moved, L, 2 * L, 1), mext, out, cv);
}
extern "C" int hp_dev_ckks_rotate_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t batch,
                           size_t step, const uint64_t *ct, const uint64_t *rot_key, uint64_t *out) {
    return dev_hks_automorphism(ctx, logn, L, k, alpha, moduli_ext, batch, false, step, ct, rot_key, out);
}
extern "C" int hp_dev_ckks_conjugate_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t batch,
                              const uint64_t *ct, const uint64_t *conj_key, uint64_t *out) {
    return dev_hks_automorphism(ctx, logn, L, k, alpha, moduli_ext, batch, true, 0, ct, conj_key, out);
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
extern "C" int hp_dev_ckks_rotate_hoisted_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                              size_t batch, size_t rotations, const size_t *steps, const unsigned char *conj,
                                              const uint64_t *ct, const uint64_t *const *keys, uint64_t *out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, steps, ct, keys, out);
    HP_ALIGNED(ctx, ct, out);
    int rc = hks_args_ok(ctx, logn, L, k, alpha, batch);
    if (rc) return rc;
    if (rotations == 0) return fail(ctx, HP_EINVAL, "rotate_hoisted: no rotations");
    for (size_t r = 0; r < rotations; r++) {
        if (!keys[r] || ((uintptr_t)keys[r] & 15u)) return fail(ctx, HP_EINVAL, "rotate_hoisted: NULL or misaligned key");
        if (!(conj && conj[r]) && steps[r] >= ((size_t)1 << 17)) return fail(ctx, HP_EINVAL, "rotation step out of range");
    }
    const size_t n = (size_t)1 << logn, E = L + k, nd = (L + alpha - 1) / alpha;
    {   // the output is written while later rotations still read the input
        const uintptr_t c0 = (uintptr_t)ct, c1 = c0 + batch * 2 * L * n * 8, o0 = (uintptr_t)out, o1 = o0 + batch * rotations * 2 * L * n * 8;
        if (o0 < c1 && c0 < o1) return fail(ctx, HP_EINVAL, "rotate_hoisted: the output overlaps the input");
    }
    const Plan *plan;
    if ((rc = get_plan(ctx, logn, moduli_ext, E, true, &plan))) return rc;
    const HksEntry *he;
    if ((rc = get_hks_consts(ctx, moduli_ext, L, k, alpha, &he))) return rc;
    LevelScope lvl(ctx, plan);   // level A: the digit stage and the drops on the FP64 kernels, as in hp_dev_hks_switch
    if (lvl.rc) return lvl.rc;
    size_t pass = std::max<size_t>(1, HOIST_POLYS / batch);   // rotations per pass
    pass = std::min(std::min(pass, rotations), (size_t)HP_HOIST_TABLE_MAX);
    const size_t PP = batch * pass;                            // switched polynomials per pass
    const size_t words = padded(batch * L * n) / 8 + padded(batch * nd * E * n) / 8 + padded(PP * L * n) / 8 + padded(PP * 2 * E * n) / 8 +
                         padded(2 * PP * k * n) / 8 + padded(2 * PP * L * n) / 8;
    if ((rc = ws_reserve(ctx, words * 8))) return rc;
    Carver cv(ctx->ws);
    u64 *lifted;
    if ((rc = hks_digits(ctx, plan, he->dev, logn, L, k, alpha, batch, ct + L * n, 2 * L, &lifted, cv))) return rc;
    u64 *moved0 = cv.take(PP * L * n), *ks = cv.take(PP * 2 * E * n), *yp = cv.take(2 * PP * k * n), *rem = cv.take(2 * PP * L * n);
    for (size_t r0 = 0; r0 < rotations; r0 += pass) {
        const size_t cnt = std::min(pass, rotations - r0), P = batch * cnt;   // this pass: polynomial b * cnt + r
        HpHoistTable ht;
        memset(&ht, 0, sizeof(ht));
        if ((rc = reserve_cycle_perms(ctx, cnt))) return rc;   // (a miss in a full map cache empties it: not between these)
        for (size_t r = 0; r < cnt; r++) {
            ht.key[r] = keys[r0 + r];
            if (!(conj && conj[r0 + r]) && (rc = get_cycle_perm(ctx, logn, steps[r0 + r], &ht.map[r]))) return rc;
        }
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
            if ((rc = chk(ctx, hp_launch_hks_inner_hoisted(plan->d_limbs, (u32)L, (u32)E, (u32)nd, (u32)alpha, (u32)n, (u32)batch, (u32)cnt,
                                                           lifted, ct + L * n, (u32)(2 * L), ht, ks, ctx->stream), "hks_inner_hoisted")))
                return rc;
        }
        if ((rc = hks_pdown(ctx, plan, he->dev, logn, L, k, P, ks, moduli_ext, yp, rem))) return rc;
        // out[b][r0 + r]: one launch when the pass holds every rotation, else one per ciphertext (its rotations are adjacent in out)
        const size_t launches = cnt == rotations ? 1 : batch, per = P / launches;
        for (size_t b = 0; b < launches; b++) {
            const Addend add(moved0 + b * per * L * n, L, L, 1);
            if ((rc = hks_down(ctx, plan, he, logn, L, k, per, ks + b * per * 2 * E * n, rem + b * per * 2 * L * n, add, moduli_ext,
                               out + (b * rotations + r0) * 2 * L * n)))
                return rc;
        }
    }
    return HP_OK;
}

// Diagonal linear transform, double hoisted: out = sum_r diag_r * rot_r(ct) with one key per rotation, the weighted sum formed in the
// extended basis Q P BEFORE ModDown.  Everything after the inner product of a switch is linear in its accumulator, so
//   sum_r diag_r * ModDown(acc_r)  ~  ModDown( sum_r diag_r * acc_r )
// up to the roundings: R of them, each scaled by its diagonal, on the left; ONE on the right.  The flow is that of a single switch of
// `batch` polynomials -- hks_digits, the accumulate launches (k_hks_inner_lintrans, at most one argument table of rotations each, the
// later ones adding to the reduced words of the earlier), hks_pdown, hks_down -- and so is the workspace, whatever `rotations` is:
// no [b][r] row set, no yp / rem per rotation, no moved c0 (the kernel folds (P mod q_i) diag_r move_r(c0) into polynomial 0 of the
// accumulator, which ModDown divides by P exactly: hks_down runs without an addend).
extern "C" int hp_dev_ckks_lintrans_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                        size_t batch, size_t rotations, const size_t *steps, const unsigned char *conj, const uint64_t *ct,
                                        const uint64_t *const *keys, const uint64_t *const *diags, uint64_t *out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, steps, ct, keys, diags, out);
    HP_ALIGNED(ctx, ct, out);
    int rc = hks_args_ok(ctx, logn, L, k, alpha, batch);
    if (rc) return rc;
    if (rotations == 0) return fail(ctx, HP_EINVAL, "lintrans: no rotations");
    for (size_t r = 0; r < rotations; r++) {
        if (!keys[r] || ((uintptr_t)keys[r] & 15u)) return fail(ctx, HP_EINVAL, "lintrans: NULL or misaligned key");
        if ((uintptr_t)diags[r] & 15u) return fail(ctx, HP_EINVAL, "lintrans: misaligned diagonal");
        if (!(conj && conj[r]) && steps[r] >= ((size_t)1 << 17)) return fail(ctx, HP_EINVAL, "rotation step out of range");
    }
    const size_t n = (size_t)1 << logn, E = L + k, nd = (L + alpha - 1) / alpha;
    {
        const uintptr_t c0 = (uintptr_t)ct, o0 = (uintptr_t)out, bytes = batch * 2 * L * n * 8;
        if (o0 < c0 + bytes && c0 < o0 + bytes) return fail(ctx, HP_EINVAL, "lintrans: the output overlaps the input");
    }
    const size_t pass = hks_lintrans_max_rotations(moduli_ext, E, nd, HP_HOIST_TABLE_MAX);   // rotations per launch
    if (pass == 0) return fail(ctx, HP_EUNSUPPORTED, "lintrans: moduli too large for the 128-bit accumulators");
    const Plan *plan;
    if ((rc = get_plan(ctx, logn, moduli_ext, E, true, &plan))) return rc;
    const HksEntry *he;
    if ((rc = get_hks_consts(ctx, moduli_ext, L, k, alpha, &he))) return rc;
    LevelScope lvl(ctx, plan);   // level A: the digit stage and the drops on the FP64 kernels, as in hp_dev_hks_switch
    if (lvl.rc) return lvl.rc;
    if ((rc = ws_reserve(ctx, hks_ws_words(n, L, k, nd, batch) * 8))) return rc;
    Carver cv(ctx->ws);
    u64 *lifted;
    if ((rc = hks_digits(ctx, plan, he->dev, logn, L, k, alpha, batch, ct + L * n, 2 * L, &lifted, cv))) return rc;
    u64 *ks = cv.take(batch * 2 * E * n), *yp = cv.take(2 * batch * k * n), *rem = cv.take(2 * batch * L * n);
    for (size_t r0 = 0; r0 < rotations; r0 += pass) {
        const size_t cnt = std::min(pass, rotations - r0);
        HpLinTable ht;
        memset(&ht, 0, sizeof(ht));
        if ((rc = reserve_cycle_perms(ctx, cnt))) return rc;   // (a miss in a full map cache empties it: not between these)
        for (size_t r = 0; r < cnt; r++) {
            ht.key[r] = keys[r0 + r];
            ht.diag[r] = diags[r0 + r];
            if (!(conj && conj[r0 + r]) && (rc = get_cycle_perm(ctx, logn, steps[r0 + r], &ht.map[r]))) return rc;
        }
        ProfScope ps(ctx, "ks_inner");
        if ((rc = chk(ctx, hp_launch_hks_inner_lintrans(plan->d_limbs, he->dev, (u32)E, (u32)n, (u32)batch, (u32)cnt, lifted, ct, ht, r0 != 0,
                                                        ks, ctx->stream), "hks_inner_lintrans")))
            return rc;
    }
    if ((rc = hks_pdown(ctx, plan, he->dev, logn, L, k, batch, ks, moduli_ext, yp, rem))) return rc;
    return hks_down(ctx, plan, he, logn, L, k, batch, ks, rem, Addend(), moduli_ext, out);
}

// Baby-step giant-step form of the diagonal transform: out = sum_g rot_g( sum_i diag_{g,i} * rot_i(ct) ), babies + giants keys for
// babies * giants diagonals.  The linearity argument above, twice: the baby results stay in the extended basis (no ModDown), every
// giant's weighted sum is formed there and pays ONE ModDown, and the giants' switches are summed in the extended basis again before
// the last ModDown.  All giants go through each stage together, as P = batch * (giants that are not the identity) polynomials:
//   1. hks_digits of c1                                      (batch polynomials)
//   2. baby rows [b][i][2][E][N], c0 folded in               (k_hks_inner_lintrans<BABY>, one launch per argument table)
//   3. pre[b][g'][2][E][N] = sum_i diag_{g,i} * baby_i       (k_hks_bsgs_presum; an identity giant's row goes straight into acc)
//   4. hks_pdown + hks_down of pre -> u[b][g'][2][L][N]      (P polynomials)
//   5. hks_digits of the u1 rows                             (P polynomials)
//   6. acc[b][2][E][N] (+)= sum_g' switch_g'(u)              (k_hks_inner_lintrans<GIANT>, one launch per argument table)
//   7. hks_pdown + hks_down of acc -> out                    (batch polynomials)
// The workspace and the pass plan are hpi::hks_bsgs_plan's (hp_drop.h): a function of the shape alone.  The first digit rows and the
// baby rows are dead after stage 3; the digit rows of stage 5 take their place.
extern "C" int hp_dev_ckks_lintrans_bsgs_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                             size_t batch, size_t babies, const size_t *baby_steps, const unsigned char *baby_conj,
                                             const uint64_t *const *baby_keys, size_t giants, const size_t *giant_steps,
                                             const unsigned char *giant_conj, const uint64_t *const *giant_keys,
                                             const uint64_t *const *diags, const uint64_t *ct, uint64_t *out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, baby_steps, baby_keys, giant_steps, giant_keys, diags, ct, out);
    HP_ALIGNED(ctx, ct, out);
    int rc = hks_args_ok(ctx, logn, L, k, alpha, batch);
    if (rc) return rc;
    if (babies == 0 || giants == 0) return fail(ctx, HP_EINVAL, "lintrans_bsgs: no baby steps or no giant steps");
    const auto entries_ok = [&](size_t cnt, const size_t *steps, const unsigned char *conj, const uint64_t *const *keys) {
        for (size_t r = 0; r < cnt; r++) {
            const bool cj = conj && conj[r];
            if (!cj && steps[r] >= ((size_t)1 << 17)) return fail(ctx, HP_EINVAL, "rotation step out of range");
            if (!keys[r] && (cj || steps[r] != 0)) return fail(ctx, HP_EINVAL, "lintrans_bsgs: a NULL key on an entry that is not the identity");
            if ((uintptr_t)keys[r] & 15u) return fail(ctx, HP_EINVAL, "lintrans_bsgs: misaligned key");
        }
        return (int)HP_OK;
    };
    if ((rc = entries_ok(babies, baby_steps, baby_conj, baby_keys)) || (rc = entries_ok(giants, giant_steps, giant_conj, giant_keys))) return rc;
    for (size_t g = 0; g < giants; g++) {
        bool any = false;
        for (size_t i = 0; i < babies; i++) {
            if ((uintptr_t)diags[g * babies + i] & 15u) return fail(ctx, HP_EINVAL, "lintrans_bsgs: misaligned diagonal");
            any = any || diags[g * babies + i];
        }
        if (!any) return fail(ctx, HP_EINVAL, "lintrans_bsgs: a giant step without a diagonal");
    }
    const size_t n = (size_t)1 << logn, E = L + k, nd = (L + alpha - 1) / alpha;
    {
        const uintptr_t c0 = (uintptr_t)ct, o0 = (uintptr_t)out, bytes = batch * 2 * L * n * 8;
        if (o0 < c0 + bytes && c0 < o0 + bytes) return fail(ctx, HP_EINVAL, "lintrans_bsgs: the output overlaps the input");
    }
    HksBsgsPlan bp;
    if (!hks_bsgs_plan(moduli_ext, n, L, k, alpha, batch, babies, giants, bp))
        return fail(ctx, HP_EUNSUPPORTED, "lintrans_bsgs: moduli too large for the 128-bit accumulators");
    const Plan *plan;
    if ((rc = get_plan(ctx, logn, moduli_ext, E, true, &plan))) return rc;
    const HksEntry *he;
    if ((rc = get_hks_consts(ctx, moduli_ext, L, k, alpha, &he))) return rc;
    LevelScope lvl(ctx, plan);   // level A: the digit stages and the drops on the FP64 kernels, as in hp_dev_hks_switch
    if (lvl.rc) return lvl.rc;
    if ((rc = ws_reserve(ctx, bp.words * 8))) return rc;
    std::vector<size_t> keyed;   // the giants that switch, in order: polynomial b * GK + (index here) from stage 3 to stage 6
    for (size_t g = 0; g < giants; g++)
        if (giant_keys[g]) keyed.push_back(g);
    const size_t GK = keyed.size(), rows = 2 * E * n;
    Carver cv(ctx->ws), late(ctx->ws);   // `late`: stage 5's digit rows, over the first digit rows and the baby rows
    u64 *lifted;
    if ((rc = hks_digits(ctx, plan, he->dev, logn, L, k, alpha, batch, ct + L * n, 2 * L, &lifted, cv))) return rc;
    u64 *baby = cv.take(batch * babies * rows);
    cv.off = bp.overlay_words * 8;
    u64 *acc = cv.take(batch * rows), *pre = cv.take(batch * giants * rows), *yp = cv.take(2 * batch * giants * k * n),
        *rem = cv.take(2 * batch * giants * L * n), *u = cv.take(batch * giants * 2 * L * n);
    // a table of rotations [r0, r0 + cnt) of a list; a NULL key with a NULL map is the identity (babies only: keyed giants come here)
    const auto fill = [&](HpLinTable &ht, const size_t *steps, const unsigned char *conj, const uint64_t *const *keys, const size_t *idx,
                          size_t r0, size_t cnt) {
        memset(&ht, 0, sizeof(ht));
        int e = reserve_cycle_perms(ctx, cnt);   // (a miss in a full map cache empties it: not between these)
        for (size_t r = 0; r < cnt && !e; r++) {
            const size_t at = idx ? idx[r0 + r] : r0 + r;
            ht.key[r] = keys[at];
            if (keys[at] && !(conj && conj[at])) e = get_cycle_perm(ctx, logn, steps[at], &ht.map[r]);
        }
        return e;
    };
    for (size_t i0 = 0; i0 < babies; i0 += HP_HOIST_TABLE_MAX) {   // stage 2
        const size_t cnt = std::min<size_t>(HP_HOIST_TABLE_MAX, babies - i0);
        HpLinTable ht;
        if ((rc = fill(ht, baby_steps, baby_conj, baby_keys, nullptr, i0, cnt))) return rc;
        ProfScope ps(ctx, "ks_inner");
        if ((rc = chk(ctx, hp_launch_hks_bsgs_babies(plan->d_limbs, he->dev, (u32)E, (u32)n, (u32)batch, (u32)cnt, (u32)babies, lifted, ct, ht,
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
            for (size_t c = 0; c < gcnt; c++) {
                const size_t g = gs[c];
                for (size_t i = 0; i < cnt; i++) pt.diag[c * cnt + i] = diags[g * babies + i0 + i];
                pt.dst[c] = to_acc ? acc : pre + (size_t)(gs + c - keyed.data()) * rows;
            }
            const bool add = to_acc ? acc_written : i0 != 0;
            ProfScope ps(ctx, "ks_inner");
            int e = chk(ctx, hp_launch_hks_bsgs_presum(plan->d_limbs, (u32)E, (u32)n, (u32)batch, (u32)gcnt, (u32)cnt, baby + i0 * rows,
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
        if ((rc = hks_pdown(ctx, plan, he->dev, logn, L, k, P, pre, moduli_ext, yp, rem))) return rc;           // stage 4
        if ((rc = hks_down(ctx, plan, he, logn, L, k, P, pre, rem, Addend(), moduli_ext, u))) return rc;
        u64 *lifted2;
        if ((rc = hks_digits(ctx, plan, he->dev, logn, L, k, alpha, P, u + L * n, 2 * L, &lifted2, late))) return rc;   // stage 5
        for (size_t c0 = 0; c0 < GK; c0 += bp.giant_pass) {                                                     // stage 6
            const size_t cnt = std::min(bp.giant_pass, GK - c0);
            HpLinTable ht;
            if ((rc = fill(ht, giant_steps, giant_conj, giant_keys, keyed.data(), c0, cnt))) return rc;
            ProfScope ps(ctx, "ks_inner");
            if ((rc = chk(ctx, hp_launch_hks_bsgs_giants(plan->d_limbs, he->dev, (u32)E, (u32)n, (u32)batch, (u32)cnt, (u32)GK,
                                                         lifted2 + c0 * nd * E * n, u + c0 * 2 * L * n, ht, acc_written, acc, ctx->stream),
                          "hks_bsgs_giants")))
                return rc;
            acc_written = true;
        }
    }
    if ((rc = hks_pdown(ctx, plan, he->dev, logn, L, k, batch, acc, moduli_ext, yp, rem))) return rc;           // stage 7
    return hks_down(ctx, plan, he, logn, L, k, batch, acc, rem, Addend(), moduli_ext, out);
}

// ckks::mult_low_level + relinearisation with a hybrid key + rescale by the last ciphertext modulus
extern "C" int hp_dev_ckks_mult_relin_rescale_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                       size_t batch, const uint64_t *ct1, const uint64_t *ct2, const uint64_t *key,
                                       uint64_t *out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_ext, ct1, ct2, key, out);
    HP_ALIGNED(ctx, ct1, ct2, key, out);
    int rc = hks_args_ok(ctx, logn, L, k, alpha, batch);
    if (rc) return rc;
    if (L < 2) return fail(ctx, HP_EINVAL, "Unable to drop the only one prime.");
    const Plan *plan;
    if ((rc = get_plan(ctx, logn, moduli_ext, L + k, true, &plan))) return rc;
    const HksEntry *he;
    if ((rc = get_hks_consts(ctx, moduli_ext, L, k, alpha, &he))) return rc;
    LevelScope lvl(ctx, plan);
    if (lvl.rc) return lvl.rc;
    const size_t n = (size_t)1 << logn, nd = (L + alpha - 1) / alpha;
    const size_t words = padded(batch * 3 * L * n) / 8 + padded(batch * 2 * L * n) / 8 + hks_ws_words(n, L, k, nd, batch) +
                         drop_ws_words(n, L, 2 * batch) + 2 * (padded(2 * batch * n) / 8);
    if ((rc = ws_reserve(ctx, words * 8))) return rc;
    Carver cv(ctx->ws);
    u64 *quad = cv.take(batch * 3 * L * n), *lin = cv.take(batch * 2 * L * n);
    {
        ProfScope ps(ctx, "tensor");
        if ((rc = chk(ctx, hp_launch_tensor(plan->d_limbs, (u32)L, 0, (u32)L, (u32)n, (u32)batch, ct1, ct2, quad, ctx->stream), "tensor")))
            return rc;
    }
    if (fused_drop_ok(ctx, logn) && !ctx->hks_two_step) {
        // ModDown and the rescale in ONE transform per remaining limb.  With c = the coefficients of the relinearised limb L-1,
        //   ((ks_i - NTT(rem_i)) P^-1 + quad_i - NTT(centre_i(c))) q_last^-1 = ((ks_i - NTT(rem_i + P centre_i(c))) P^-1 + quad_i) q_last^-1
        // so: ModDown of limb L-1 alone -> its coefficients -> rem_i += P centre_i(c) -> one fused transform over limbs 0..L-2.
        // The same residues as the two-step composition below (another lazy representative of them).
        const size_t P2 = 2 * batch, E = L + k;
        const Addend add(quad, L, 3 * L, 3);
        u64 *ks, *rem;
        if ((rc = hks_front(ctx, plan, he->dev, logn, L, k, alpha, batch, quad + 2 * L * n, 3 * L, key, moduli_ext, &ks, &rem, cv))) return rc;
        u64 *r_last = cv.take(P2 * n), *c_last = cv.take(P2 * n);
        {
            HpDropArgs da = drop_args(ks + (L - 1) * n, E, add.from((L - 1) * n), r_last, 1);
            if ((rc = hks_down_fused(ctx, plan, he, logn, L, L - 1, 1, P2, rem, da, ctx->cur_a, moduli_ext, "hks ModDown of the last limb",
                                     "hks ModDown of the last limb (level A)")))
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
            if ((rc = chk(ctx, hp_launch_hks_combine(plan->d_limbs, he->dev, (u32)L, (u32)n, (u32)P2, c_last, rem, ctx->stream), "hks_combine")))
                return rc;
        }
        HpNttJob fj = batch_job(plan, logn, L - 1, P2, rem, nullptr, L, 0, 0, 0);
        HpDropArgs da = drop_args(ks, E, add, out, L - 1);
        hks_down_rescale_consts(he->host, moduli_ext, L, in_loads ? c_last : nullptr, da);
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
    if ((rc = hks_switch(ctx, plan, he, logn, L, k, alpha, batch, quad + 2 * L * n, 3 * L, key, Addend(quad, L, 3 * L, 3), moduli_ext, lin, cv)))
        return rc;
    return drop_last(ctx, plan, logn, L, 2 * batch, false, 0, lin, Addend(), out, cv);
}

