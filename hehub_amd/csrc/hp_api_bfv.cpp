// hp_api_bfv.cpp -- C ABI, part 4 (extension): BFV's scale-invariant multiplication and decryption rounding; kernels in hp_bfv.hip,
// constants in hp_bfv.h.  Exact integer arithmetic throughout (both base conversions by mixed-radix composition), pinned by a
// Python-integer model and by decryption (tests/bfv_model.py).  The relinearising calls live with the other multiplication tails of
// the hybrid key switch (hp_api_hks_mult.cpp) and use bfv_mult from here.
// Every transform in this file is the level-B launch at either parity level, and one reduction to the canonical residue follows the
// last one: the words do not depend on the level (the contract of the seeded calls).
#include "hp_ctx.h"

#include <algorithm>

namespace hpi {

int bfv_check(hp_ctx *ctx, size_t logn, size_t L, size_t M, const uint64_t *q, const uint64_t *b, bool with_t, u64 t, size_t count) {
    if (logn < 3 || logn > 16) return fail(ctx, HP_EINVAL, "bfv: ring degrees 2^3 .. 2^16 are supported");
    if (L == 0 || M == 0) return fail(ctx, HP_EINVAL, "bfv: an empty base");
    if (count == 0) return fail(ctx, HP_EINVAL, "empty batch");
    if (L > HP_BFV_MAX || M > HP_BFV_MAX || L + M > HP_MAX_LIMBS) return fail(ctx, HP_EUNSUPPORTED, "bfv: at most 16 moduli per base and 32 in all");
    if (count > ((size_t)1 << 30) / (3 * (L + M) * (((size_t)1 << logn) / 2048 + 1)))   // (every launch below 2^30 workgroups, every u32 row count with it)
        return fail(ctx, HP_EUNSUPPORTED, "bfv: too many polynomials for one call");
    if (with_t) {
        if (t < 2) return fail(ctx, HP_EINVAL, "bfv: the plain modulus must be at least 2");
        for (size_t i = 0; i < L; i++)
            if (t >= q[i]) return fail(ctx, HP_EINVAL, "bfv: the plain modulus must be below every modulus");
        for (size_t j = 0; j < M; j++)
            if (t >= b[j]) return fail(ctx, HP_EINVAL, "bfv: the plain modulus must be below every modulus");
    }
    for (size_t i = 0; i < L; i++)
        if (!(q[i] & 1) || q[i] < 3) return fail(ctx, HP_EINVAL, "bfv: the moduli must be odd");
    for (size_t j = 0; j < M; j++) {
        if (!(b[j] & 1) || b[j] < 3) return fail(ctx, HP_EINVAL, "bfv: the moduli must be odd");
        for (size_t i = 0; i < L; i++)
            if (b[j] == q[i]) return fail(ctx, HP_EINVAL, "bfv: the auxiliary base shares a modulus with the ciphertext modulus");
    }
    if (with_t) {
        std::vector<u64> qb(q, q + L);
        qb.insert(qb.end(), b, b + M);
        if (!bfv_base_ok(qb.data(), L, M, t, (u64)1 << logn)) return fail(ctx, HP_EINVAL, "bfv: the auxiliary base is too small (B >= 4 t N Q)");
    }
    return HP_OK;
}

int bfv_open(hp_ctx *ctx, size_t logn, size_t L, size_t M, const uint64_t *q, const uint64_t *b, bool with_t, u64 t, BfvShape &s) {
    return contained(ctx, [&] {
        s.logn = logn; s.L = L; s.M = M; s.n = (size_t)1 << logn; s.t = t;
        s.qb.assign(q, q + L);
        s.qb.insert(s.qb.end(), b, b + M);
        int rc;
        if ((rc = get_plan(ctx, logn, s.qb.data(), L + M, true, &s.plan)) || (rc = get_bfv_consts(ctx, s.qb.data(), L, M, &s.consts))) return rc;
        if (with_t) bfv_plain(s.qb.data(), L + M, t, s.plain);
        return (int)HP_OK;
    });
}

// lift of P polynomials: in [P][in_ps rows][N] (NTT form, words below 2q, L rows used) -> out [P][L + M][N], canonical residues:
// the Q rows carried over, the B rows = NTT(centre_Q(x) mod b_j)
static size_t bfv_lift_bytes(const BfvShape &s, size_t P) { return padded(P * s.L * s.n); }
static int bfv_lift(hp_ctx *ctx, const BfvShape &s, size_t P, const u64 *in, size_t in_ps, u64 *out, Carver &cv) {
    const size_t L = s.L, M = s.M, n = s.n, E = L + M;
    const HpLimb *ql = s.plan->d_limbs, *bl = s.plan->d_limbs + L;
    u64 *coef = cv.take(P * L * n);
    int rc;
    if ((rc = run_ntt(ctx, batch_job(s.plan, s.logn, L, P, in, coef, in_ps, L, 1, 1)))) return rc;   // strict coefficients over Q
    {
        ProfScope ps(ctx, "bfv_lift");
        if ((rc = chk(ctx, hp_launch_bfv_lift(ql, bl, &s.consts->q2b, (u32)L, (u32)M, (u32)n, (u32)P, coef, (u32)L, out + L * n, (u32)E, ctx->stream),
                      "bfv_lift")))
            return rc;
    }
    {
        HpNttJob j = batch_job(s.plan, s.logn, M, P, out + L * n, out + L * n, E, E, 0, 0);
        j.limbs = bl;
        if ((rc = run_ntt(ctx, j))) return rc;
    }
    ProfScope ps(ctx, "elem");
    if ((rc = chk(ctx, hp_launch_bfv_canonical(bl, (u32)M, (u32)n, (u32)P, out + L * n, (u32)E, out + L * n, (u32)E, ctx->stream), "bfv_canonical"))) return rc;
    return chk(ctx, hp_launch_bfv_canonical(ql, (u32)L, (u32)n, (u32)P, in, (u32)in_ps, out, (u32)E, ctx->stream), "bfv_canonical");
}

// scaling of P polynomials: in [P][L + M][N] (NTT form, words below 2q) -> out [P][L][N], canonical residues of floor((t x + h) / Q)
static size_t bfv_scale_bytes(const BfvShape &s, size_t P) { return padded(P * (s.L + s.M) * s.n) + padded(P * s.M * s.n); }
static int bfv_scale(hp_ctx *ctx, const BfvShape &s, size_t P, const u64 *in, u64 *out, Carver &cv) {
    const size_t L = s.L, M = s.M, n = s.n, E = L + M;
    const HpLimb *ql = s.plan->d_limbs, *bl = s.plan->d_limbs + L;
    u64 *coef = cv.take(P * E * n), *y = cv.take(P * M * n);
    int rc;
    if ((rc = run_ntt(ctx, batch_job(s.plan, s.logn, E, P, in, coef, E, E, 1, 1)))) return rc;   // strict coefficients over Q B
    {
        ProfScope ps(ctx, "bfv_scale");
        if ((rc = chk(ctx, hp_launch_bfv_scale(ql, s.consts, s.plain, (u32)L, (u32)n, (u32)P, coef, y, ctx->stream), "bfv_scale"))) return rc;
    }
    {
        ProfScope ps(ctx, "bfv_lift");   // centre_B(y) into every q_i
        if ((rc = chk(ctx, hp_launch_bfv_lift(bl, ql, &s.consts->b2q, (u32)M, (u32)L, (u32)n, (u32)P, y, (u32)M, out, (u32)L, ctx->stream), "bfv_lift")))
            return rc;
    }
    if ((rc = run_ntt(ctx, batch_job(s.plan, s.logn, L, P, out, out, L, L, 0, 0)))) return rc;
    ProfScope ps(ctx, "elem");
    return chk(ctx, hp_launch_bfv_canonical(ql, (u32)L, (u32)n, (u32)P, out, (u32)L, out, (u32)L, ctx->stream), "bfv_canonical");
}

// the multiplication: lift of the four polynomials, the tensor product over L + M limbs, scaling of the three
size_t bfv_mult_bytes(const BfvShape &s, size_t batch) {
    const size_t E = s.L + s.M;
    return 2 * padded(batch * 2 * E * s.n) + padded(batch * 3 * E * s.n) + std::max(bfv_lift_bytes(s, 2 * batch), bfv_scale_bytes(s, 3 * batch));
}
int bfv_mult(hp_ctx *ctx, const BfvShape &s, size_t batch, const u64 *ct1, const u64 *ct2, u64 *quad, Carver &cv) {
    const size_t L = s.L, n = s.n, E = s.L + s.M;
    u64 *a = cv.take(batch * 2 * E * n), *b = cv.take(batch * 2 * E * n), *wide = cv.take(batch * 3 * E * n);
    Carver c1 = cv, c2 = cv, c3 = cv;   // the stages' scratch rows share one block (stream order)
    cv.off += std::max(bfv_lift_bytes(s, 2 * batch), bfv_scale_bytes(s, 3 * batch));
    int rc;
    if ((rc = bfv_lift(ctx, s, 2 * batch, ct1, L, a, c1)) || (rc = bfv_lift(ctx, s, 2 * batch, ct2, L, b, c2))) return rc;
    {
        ProfScope ps(ctx, "tensor");
        if ((rc = chk(ctx, hp_launch_tensor(s.plan->d_limbs, (u32)E, 0, (u32)E, (u32)n, (u32)batch, a, b, wide, ctx->stream), "tensor"))) return rc;
    }
    return bfv_scale(ctx, s, 3 * batch, wide, quad, c3);
}

} // namespace hpi

using namespace hpi;

extern "C" {

int hp_dev_bfv_lift(hp_ctx *ctx, size_t logn, size_t L, size_t M, const uint64_t *moduli_qb, size_t polys, const uint64_t *d_in,
                    uint64_t *d_out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_qb, d_in, d_out);
    HP_ALIGNED(ctx, d_in, d_out);
    int rc = bfv_check(ctx, logn, L, M, moduli_qb, moduli_qb + L, false, 0, polys);
    if (rc) return rc;
    const size_t n = (size_t)1 << logn;
    if (ranges_overlap(d_in, polys * L * n * 8, d_out, polys * (L + M) * n * 8)) return fail(ctx, HP_EINVAL, "bfv_lift: the output overlaps an input");
    BfvShape s;
    if ((rc = bfv_open(ctx, logn, L, M, moduli_qb, moduli_qb + L, false, 0, s)) || (rc = ws_reserve(ctx, bfv_lift_bytes(s, polys)))) return rc;
    Carver cv(ctx->ws);
    return bfv_lift(ctx, s, polys, d_in, L, d_out, cv);
}

int hp_dev_bfv_scale_round(hp_ctx *ctx, size_t logn, size_t L, size_t M, const uint64_t *moduli_qb, uint64_t t, size_t polys,
                           const uint64_t *d_in, uint64_t *d_out) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_qb, d_in, d_out);
    HP_ALIGNED(ctx, d_in, d_out);
    int rc = bfv_check(ctx, logn, L, M, moduli_qb, moduli_qb + L, true, t, polys);
    if (rc) return rc;
    const size_t n = (size_t)1 << logn;
    if (ranges_overlap(d_in, polys * (L + M) * n * 8, d_out, polys * L * n * 8)) return fail(ctx, HP_EINVAL, "bfv_scale_round: the output overlaps an input");
    BfvShape s;
    if ((rc = bfv_open(ctx, logn, L, M, moduli_qb, moduli_qb + L, true, t, s)) || (rc = ws_reserve(ctx, bfv_scale_bytes(s, polys)))) return rc;
    Carver cv(ctx->ws);
    return bfv_scale(ctx, s, polys, d_in, d_out, cv);
}

int hp_dev_bfv_mult_low_level(hp_ctx *ctx, size_t logn, size_t L, size_t M, const uint64_t *moduli_qb, uint64_t t, size_t batch,
                              const uint64_t *d_ct1, const uint64_t *d_ct2, uint64_t *d_quad) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli_qb, d_ct1, d_ct2, d_quad);
    HP_ALIGNED(ctx, d_ct1, d_ct2, d_quad);
    int rc = bfv_check(ctx, logn, L, M, moduli_qb, moduli_qb + L, true, t, batch);
    if (rc) return rc;
    const size_t n = (size_t)1 << logn;
    if (ranges_overlap(d_ct1, batch * 2 * L * n * 8, d_quad, batch * 3 * L * n * 8) ||
        ranges_overlap(d_ct2, batch * 2 * L * n * 8, d_quad, batch * 3 * L * n * 8))
        return fail(ctx, HP_EINVAL, "bfv_mult_low_level: the output overlaps an input");
    BfvShape s;
    if ((rc = bfv_open(ctx, logn, L, M, moduli_qb, moduli_qb + L, true, t, s)) || (rc = ws_reserve(ctx, bfv_mult_bytes(s, batch)))) return rc;
    Carver cv(ctx->ws);
    return bfv_mult(ctx, s, batch, d_ct1, d_ct2, d_quad, cv);
}

int hp_dev_bfv_decrypt_round(hp_ctx *ctx, size_t n, size_t L, const uint64_t *moduli, uint64_t t, size_t polys, const uint64_t *d_x,
                             uint64_t *d_m) {
    HP_ENTER(ctx);
    HP_REQUIRE(ctx, moduli, d_x, d_m);
    HP_ALIGNED(ctx, d_x, d_m);
    if (n < 8 || n > ((size_t)1 << 16) || (n & (n - 1))) return fail(ctx, HP_EINVAL, "bfv: ring degrees 2^3 .. 2^16 are supported");
    if (L == 0) return fail(ctx, HP_EINVAL, "bfv: an empty base");
    if (polys == 0) return fail(ctx, HP_EINVAL, "empty batch");
    if (L > HP_BFV_MAX) return fail(ctx, HP_EUNSUPPORTED, "bfv: at most 16 moduli per base and 32 in all");
    if (polys > ((size_t)1 << 30) / (n / 2048 + 1)) return fail(ctx, HP_EUNSUPPORTED, "bfv: too many polynomials for one call");
    if (t < 2) return fail(ctx, HP_EINVAL, "bfv: the plain modulus must be at least 2");
    for (size_t i = 0; i < L; i++)
        if (t >= moduli[i]) return fail(ctx, HP_EINVAL, "bfv: the plain modulus must be below every modulus");
    for (size_t i = 0; i < L; i++)
        if (!(moduli[i] & 1) || moduli[i] < 3) return fail(ctx, HP_EINVAL, "bfv: the moduli must be odd");
    HpBfvDecPlain pc;
    if (!bfv_dec_plain(moduli, L, t, pc)) return fail(ctx, HP_EINVAL, "bfv: the plain modulus must be coprime to the ciphertext modulus");
    if (ranges_overlap(d_x, polys * L * n * 8, d_m, polys * n * 8)) return fail(ctx, HP_EINVAL, "bfv_decrypt_round: the output overlaps an input");
    const Plan *plan;
    const HpBfvConsts *bc;
    int rc;
    if ((rc = get_plan(ctx, 0, moduli, L, false, &plan)) || (rc = get_bfv_consts(ctx, moduli, L, 0, &bc))) return rc;
    ProfScope ps(ctx, "bfv_decrypt_round");
    return chk(ctx, hp_launch_bfv_decrypt_round(plan->d_limbs, bc, pc, (u32)L, (u32)n, (u32)polys, d_x, d_m, ctx->stream), "bfv_decrypt_round");
}

} // extern "C"
