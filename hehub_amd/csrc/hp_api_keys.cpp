// hp_api_keys.cpp -- C ABI, part 3 (extension): what makes fresh keys and ciphertexts on the device -- the hybrid key generators
// (kernels in hp_hks.hip, over the call object of hp_hks_call.h), the ChaCha20 samplers and seeded RLWE encryption (hp_sample.hip).
#include "hp_hks_call.h"

#include <algorithm>

using namespace hpi;

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
        if (!(rot->conj && rot->conj[r]) && !rot_step_ok(rot->steps[r])) return fail(ctx, HP_EINVAL, "rotation step out of range");
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
extern "C" int hp_dev_sample_gauss(hp_ctx *ctx, size_t logn, size_t batch, const uint8_t *seed, uint64_t stream, int64_t *d_out) {
    return dev_sample_signed(ctx, HP_SAMPLE_GAUSS, "sample_gauss", logn, batch, seed, stream, d_out);
}
// the profile scope of an error row drawn with the context's sampler (hp_ctx_set_error_sampler)
static const char *error_scope(const hp_ctx *ctx) { return ctx->error_sampler == HP_SAMPLE_GAUSS ? "sample_gauss" : "sample_cbd"; }

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
// the draw of a seeded generator: a into the [1] halves, error_scale * e (the context's error sampler) into workspace (i64[keys][dnum][N]: a function of
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
        ProfScope ps(c.ctx, error_scope(c.ctx));
        return chk(c.ctx, hp_launch_sample_signed(c.ctx->error_sampler, hp_sample_seed(seed), (u32)c.logn, keys * c.nd, stream,
                                                  (long long)error_scale, e, c.ctx->stream), error_scope(c.ctx));
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
// The small polynomials (errors by the context's error sampler, the public-key form's ternary u) go from the keystream straight to
// the residues of every modulus (k_sample_spread) and through the batched forward transform where the ciphertext will lie; one
// fused kernel then finishes the rows.  The transforms are the level-B launches at either parity level and the last kernel reduces to the canonical residue, so
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
    if ((rc = small_ntt_rows(ctx, plan, rows, ctx->error_sampler, logn, L, batch, seed, stream, 1, error_scale, ct_rows, d_ct))) return rc;
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
    if ((rc = small_ntt_rows(ctx, plan, rows, ctx->error_sampler, logn, L, 2 * batch, seed, stream, 1, error_scale, L, d_ct)) ||
        (rc = small_ntt_rows(ctx, plan, rows, HP_SAMPLE_TERNARY, logn, L, batch, seed, stream, 2, 1, L, u)))
        return rc;
    if (d_pt && (rc = run_ntt(ctx, batch_job(plan, logn, L, batch, d_pt, ptn, L, L, 0, 0)))) return rc;
    ProfScope ps(ctx, "enc_pk_fin");
    return chk(ctx, hp_launch_enc_pk_fin(plan->d_limbs, (u32)L, (u32)n, (u32)batch, d_pk, u, ptn, d_ct, ctx->stream), "enc_pk_fin");
}
