// hp_drop.cpp -- the constants of the fused drop launches (hp_drop.h has the field-by-field description).  Host only, no HIP, no
// context: modular algebra on a chain of moduli, checked against a big-integer model by tests/test_host_drop_consts.py.
#include "hp_drop.h"

#include "hp_tables.h"

#include <algorithm>
#include <cstring>

int hp_drop_flavour_b(const HpDropArgs &da, bool *small) {
    int flav = 0;
    if (!da.fin_on && !da.raw_input && !da.comb) {
        if (!da.addend || da.add_mask == 0) flav = 1;
        else if (da.add_mask == 3u) flav = 2;
        else if (da.add_mask == 1u && !da.dc.bgv) flav = 5;   // rotation / conjugation: += moved[0]
        if (flav && flav != 5 && da.dc.bgv) flav += 2;
    }
    *small = flav != 0 && da.small_rem != 0;
    return flav;
}

int hp_drop_flavour_a(const HpDropArgs &da) {
    if (da.fin_on || da.raw_input) return -1;
    int flav = 0;
    if (da.comb) flav = (da.addend && da.add_mask == 3u) ? (da.dc.bgv ? 7 : 6) : 0;   // two drops at once
    else if (!da.addend || da.add_mask == 0) flav = 1;
    else if (da.add_mask == 3u) flav = 2;
    else if (da.add_mask == 1u && !da.dc.bgv) flav = 5;
    if (flav && flav < 5 && da.dc.bgv) flav += 2;
    return flav ? flav : -1;
}

namespace hpi {

namespace {
u64 inv_mod(u64 v, u64 q) { return hp::inverse_mod_prime(v, q) % q; }
void harvey_pair(u64 v, u64 q, u64 &w, u64 &w_h) { w = v; w_h = hp::harvey_quotient(v, q); }
u64 f64_of(u64 v) { return hp::f64_bits((double)v); }
} // namespace

void a_pair(u64 v, u64 q, u64 &bits, u64 &bits_h) {
    bits = hp::f64_bits((double)v);
    bits_h = hp::f64_bits((double)v / (double)q);
}

HpDropArgs drop_args(const u64 *x, size_t L, const Addend &add, u64 *out, size_t out_stride) {
    HpDropArgs da;
    memset(&da, 0, sizeof(da));
    da.x = x; da.L = (u32)L; da.out = out; da.out_stride = (u32)out_stride;
    da.addend = add.rows; da.add_poly_stride = add.poly_stride; da.add_ct_stride = add.ct_stride; da.add_mask = add.mask;
    return da;
}

void drop_consts(const hp::ModConsts *chain, size_t L, size_t k0, size_t k1, bool bgv, u64 t, HpDropConsts &dc) {
    const u64 q_last = chain[L - 1].q;
    memset(&dc, 0, sizeof(dc));
    dc.q_last = q_last;
    dc.half_q_last = q_last / 2;
    dc.bgv = bgv ? 1 : 0;
    for (size_t k = k0; k < k1; k++) {
        const u64 q = chain[k].q;
        const size_t i = k - k0;
        dc.r[i] = q_last % q;
        harvey_pair(inv_mod(q_last, q), q, dc.inv[i], dc.inv_h[i]);
        if (bgv) {
            harvey_pair(t % q, q, dc.t[i], dc.t_h[i]);
            harvey_pair((q_last % t) % q, q, dc.qlt[i], dc.qlt_h[i]);
        }
    }
}

int drop_small_rem(const hp::ModConsts *chain, size_t L, size_t k0, size_t k1) {
    for (size_t k = k0; k < k1; k++)
        if (chain[L - 1].q > 2 * chain[k].q) return 0;
    return 1;
}

void drop_consts_to_a(const hp::ModConsts *chain, size_t k0, size_t k1, HpDropConsts &dc) {
    dc.q_last = f64_of(dc.q_last);
    dc.half_q_last = f64_of(dc.half_q_last);
    for (size_t k = k0; k < k1; k++) {
        const u64 q = chain[k].q;
        const size_t i = k - k0;
        a_pair(dc.inv[i], q, dc.inv[i], dc.inv_h[i]);
        a_pair(dc.t[i], q, dc.t[i], dc.t_h[i]);
        a_pair(dc.qlt[i], q, dc.qlt[i], dc.qlt_h[i]);
    }
}

void drop_post_scalar(u64 t, u64 q_last, bool level_a, u64 &s, u64 &s_h) {
    const u64 v = inv_mod(t, q_last);
    if (level_a) a_pair(v, q_last, s, s_h);
    else harvey_pair(v, q_last, s, s_h);
}

void two_drop_consts(const hp::ModConsts *chain, size_t L, bool bgv, u64 t1, u64 t2, HpDropArgs &da, HpInvMixArgs &mx) {
    HpDropConsts dc1, dc2;
    drop_consts(chain, L + 1, 0, L, bgv, t1, dc1);
    drop_consts(chain, L, 0, L - 1, bgv, t2, dc2);
    // A = p^-1 [(p mod t1)], m = A [t1], m2 = 1 [t2], B = q'^-1 [(q' mod t2)]     (bracketed factors: BGV)
    auto first_drop = [&](size_t k, u64 &A, u64 &m) {
        const u64 q = chain[k].q;
        A = m = dc1.inv[k];
        if (bgv) {
            A = hp::mul_mod(A, dc1.qlt[k], q);
            m = hp::mul_mod(A, dc1.t[k], q);
        }
    };
    da.dc.bgv = bgv ? 1 : 0;
    da.dc.q_last = f64_of(dc1.q_last);
    da.dc.half_q_last = f64_of(dc1.half_q_last);
    da.q2_last = f64_of(dc2.q_last);
    da.half_q2_last = f64_of(dc2.half_q_last);
    for (size_t k = 0; k + 1 < L; k++) {
        const u64 q = chain[k].q;
        u64 A, m;
        first_drop(k, A, m);
        const u64 m2 = bgv ? dc2.t[k] : 1 % q;
        const u64 B = bgv ? hp::mul_mod(dc2.inv[k], dc2.qlt[k], q) : dc2.inv[k];
        a_pair(A, q, da.dc.inv[k], da.dc.inv_h[k]);
        a_pair(m, q, da.dc.t[k], da.dc.t_h[k]);
        a_pair(m2, q, da.comb_mul[k], da.comb_mul_h[k]);
        a_pair(B, q, da.dc.qlt[k], da.dc.qlt_h[k]);
    }
    u64 A, K;
    first_drop(L - 1, A, K);
    a_pair(A, chain[L - 1].q, mx.A, mx.A_h);
    a_pair(K, chain[L - 1].q, mx.K, mx.K_h);
    mx.prev_q = da.dc.q_last;
    mx.prev_half = da.dc.half_q_last;
}

bool hks_limb_consts(const u64 *mext, size_t L, size_t k, HksLimbConsts &out) {
    out.pinv.assign(L, 0); out.pinv_h.assign(L, 0); out.p_mod_q.assign(L, 0); out.p_mod_q_h.assign(L, 0);
    for (size_t i = 0; i < L; i++) {
        const u64 q = mext[i];
        u64 pm = 1 % q;
        for (size_t j = 0; j < k; j++) pm = hp::mul_mod(pm, mext[L + j] % q, q);
        if (pm == 0) return false;
        harvey_pair(pm, q, out.p_mod_q[i], out.p_mod_q_h[i]);
        harvey_pair(inv_mod(pm, q), q, out.pinv[i], out.pinv_h[i]);
    }
    return true;
}

size_t hks_lintrans_max_rotations(const u64 *mext, size_t E, size_t nd, size_t table_max) {
    typedef unsigned __int128 u128;
    u64 q = 0;
    for (size_t m = 0; m < E; m++) q = std::max(q, mext[m]);
    if (q == 0 || q >> 62) return 0;   // (2q must leave room in a word; keeps everything below inside 128 bits)
    const u128 t = (((u128)q * q) >> 64) + 1, w = 4 * (u128)nd * t + 3 * (u128)q;
    if (w >> 64) return 0;
    const u128 r = ~(u128)0 / (w * (2 * (u128)q));
    return r < table_max ? (size_t)r : table_max;
}

size_t tensor_sum_max_terms(const u64 *moduli, size_t L, size_t table_max) {
    typedef unsigned __int128 u128;
    u64 q = 0;
    for (size_t m = 0; m < L; m++) q = std::max(q, moduli[m]);
    if (q == 0 || q >> 62) return 0;   // (2q must leave room in a word; (2q - 1)^2 then stays below 2^126)
    const u128 w = 2 * (u128)q - 1, top = ((((u128)1 << 64) - q) << 64) - 1;
    const u128 r = top / (2 * w * w);
    return r < table_max ? (size_t)r : table_max;
}

size_t lincomb_max_terms(const u64 *moduli, size_t L, size_t table_max) {
    typedef unsigned __int128 u128;
    u64 q = 0;
    for (size_t m = 0; m < L; m++) q = std::max(q, moduli[m]);
    if (q < 2 || q >> 62) return 0;   // ((q - 1)(2q - 1) then stays below 2^125)
    const u128 top = ((((u128)1 << 64) - q) << 64) - 1 - 3 * (u128)q;
    const u128 r = top / (((u128)q - 1) * (2 * (u128)q - 1));
    return r < table_max ? (size_t)r : table_max;
}

bool hks_bsgs_plan(const u64 *mext, size_t n, size_t L, size_t k, size_t alpha, size_t batch, size_t babies, size_t giants,
                   HksBsgsPlan &out) {
    out = HksBsgsPlan();
    if (babies == 0 || giants == 0 || alpha == 0) return false;
    const size_t E = L + k, nd = (L + alpha - 1) / alpha, B = batch, G = giants;
    const size_t cap = hks_lintrans_max_rotations(mext, E, nd, HP_BSGS_TABLE_MAX);
    if (cap == 0) return false;
    const auto pad = [](size_t words) { return ((words * 8 + 255) & ~(size_t)255) / 8; };   // (hp_ctx.h: padded, in words)
    out.baby_pass = std::min(cap, babies);
    out.giant_pass = std::min<size_t>(G, HP_BSGS_TABLE_MAX);
    out.presum_giants = std::min(std::min<size_t>(G, HP_BSGS_GIANT_MAX), (size_t)HP_BSGS_DIAG_MAX / out.baby_pass);
    const size_t first = pad(B * L * n) + pad(B * nd * E * n) + pad(B * babies * 2 * E * n);
    const size_t second = pad(B * G * L * n) + pad(B * G * nd * E * n);
    out.overlay_words = std::max(first, second);
    out.words = out.overlay_words + pad(B * 2 * E * n) + pad(B * G * 2 * E * n) + pad(2 * B * G * k * n) + pad(2 * B * G * L * n) +
                pad(B * G * 2 * L * n);
    return true;
}

void a_raw_rows(HpDropArgs &da) {
    da.raw_input = 0;
    da.dc.bgv = 0;
    da.dc.q_last = hp::f64_bits(0.0);
    da.dc.half_q_last = hp::f64_bits(4611686018427387904.0);   // 2^62: no word is ever "above half"
}

void hks_down_consts(const HksLimbConsts &hc, size_t i0, size_t cnt, HpDropArgs &da) {
    da.raw_input = 1;
    for (size_t i = 0; i < cnt; i++) { da.dc.inv[i] = hc.pinv[i0 + i]; da.dc.inv_h[i] = hc.pinv_h[i0 + i]; }
}

void hks_down_consts_a(const u64 *mext, size_t i0, size_t cnt, HpDropArgs &da) {
    a_raw_rows(da);
    for (size_t i = 0; i < cnt; i++) a_pair(da.dc.inv[i], mext[i0 + i], da.dc.inv[i], da.dc.inv_h[i]);
}

void hks_down_rescale_consts(const HksLimbConsts &hc, const u64 *mext, size_t L, const u64 *comb, HpDropArgs &da) {
    const u64 q_last = mext[L - 1];
    hks_down_consts(hc, 0, L - 1, da);
    da.fin_on = 1;
    if (comb) { da.comb = comb; da.comb_half = q_last / 2; }
    for (size_t i = 0; i + 1 < L; i++) {
        const u64 q = mext[i];
        da.comb_mul[i] = hc.p_mod_q[i]; da.comb_mul_h[i] = hc.p_mod_q_h[i];
        da.comb_r[i] = q_last % q;
        harvey_pair(inv_mod(q_last % q, q), q, da.fin[i], da.fin_h[i]);
    }
}

void hks_down_rescale_consts_a(const u64 *mext, size_t L, HpDropArgs &da) {
    const u64 q_last = mext[L - 1];
    a_raw_rows(da);
    da.fin_on = 0;
    da.q2_last = f64_of(q_last);
    da.half_q2_last = f64_of(q_last / 2);
    for (size_t i = 0; i + 1 < L; i++) {
        const u64 q = mext[i], A = da.dc.inv[i], B = da.fin[i];
        a_pair(A, q, da.dc.inv[i], da.dc.inv_h[i]);
        a_pair(A, q, da.dc.t[i], da.dc.t_h[i]);
        a_pair(1 % q, q, da.comb_mul[i], da.comb_mul_h[i]);
        a_pair(B, q, da.dc.qlt[i], da.dc.qlt_h[i]);
    }
}

} // namespace hpi
