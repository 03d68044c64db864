// hp_bfv.h -- BFV's exact scale-invariant multiplication and decryption rounding (EXTENSION; include/hehub_amd.h has the convention) as
// the host describes them to the kernels of hp_bfv.hip: the constant blocks, and the pure builders of every word in them.
// No HIP here: the builders take plain moduli and are checked word for word on the CPU (tests/test_bfv_host.py, tests/cpp/bfv_shim.cpp).
// hp_kernels.h includes this header; the kernels read the structs as they are laid out here.
//
//   Q = q_0 ... q_{L-1} the ciphertext modulus (odd), h = (Q - 1) / 2 = floor(Q / 2); B = b_0 ... b_{M-1} the auxiliary base; t the
//   plain modulus.  moduli_qb = q_0 .. q_{L-1}, b_0 .. b_{M-1}.
//   HpBfvBase   one exact centred conversion X -> Y (X = Q, Y = B for the lift; X = B, Y = Q after the scaling): Garner inverses and the
//               digits of floor(X/2) for the composition, the prefix products and X itself modulo every target for the reduction
//   HpBfvConsts both directions of one (moduli_qb, L, M), Q^-1 mod b_j and h modulo every modulus -- a function of the chain alone
//   HpBfvPlain, HpBfvDecPlain   what depends on t: by value, built per call
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

typedef uint64_t u64;
typedef uint32_t u32;

#define HP_BFV_MAX 16   // moduli per base (HP_CRT_MAX_LIMBS); L + M <= HP_MAX_LIMBS

struct HpBfvBase {
    u64 inv[HP_BFV_MAX][HP_BFV_MAX], inv_h[HP_BFV_MAX][HP_BFV_MAX];     // [b][a], b < a: x_b^-1 mod x_a (+ Harvey word)
    u64 half[HP_BFV_MAX];                                               // mixed-radix digits of floor(X/2)
    u64 pref[HP_BFV_MAX][HP_BFV_MAX], pref_h[HP_BFV_MAX][HP_BFV_MAX];   // [target][a]: x_0 ... x_{a-1} mod y_target (+ Harvey word)
    u64 prod[HP_BFV_MAX];                                               // X mod y_target
};
struct HpBfvConsts {
    u32 L, M;
    HpBfvBase q2b, b2q;
    u64 qinv_b[HP_BFV_MAX], qinv_b_h[HP_BFV_MAX];   // Q^-1 mod b_j (+ Harvey word)
    u64 h_mod[2 * HP_BFV_MAX];                      // h mod moduli_qb[m]
};
struct HpBfvPlain {   // k_bfv_scale
    u64 t_mod[2 * HP_BFV_MAX], t_mod_h[2 * HP_BFV_MAX];   // t mod moduli_qb[m] (+ Harvey word)
};
struct HpBfvDecPlain {   // k_bfv_decrypt_round
    u64 t, barrett_t;                               // floor((2^64 - 1) / t)
    u64 t_mod_q[HP_BFV_MAX], t_mod_q_h[HP_BFV_MAX];   // t mod q_a (+ Harvey word modulo q_a)
    u64 pref_t[HP_BFV_MAX], pref_t_h[HP_BFV_MAX];   // q_0 ... q_{a-1} mod t (+ Harvey word modulo t)
    u64 h_t, qinv_t, qinv_t_h;                      // h mod t, Q^-1 mod t (+ Harvey word modulo t)
};

namespace hpi {

// ---- multiword unsigned integers, little-endian 64-bit limbs (the base-size decision is exact, never floating point) -----
typedef std::vector<u64> BfvWide;
inline void bfv_wide_mul(BfvWide &x, u64 m) {
    unsigned __int128 carry = 0;
    for (u64 &w : x) {
        const unsigned __int128 p = (unsigned __int128)w * m + carry;
        w = (u64)p;
        carry = p >> 64;
    }
    if (carry) x.push_back((u64)carry);
}
inline int bfv_wide_cmp(const BfvWide &a, const BfvWide &b) {
    size_t na = a.size(), nb = b.size();
    while (na && !a[na - 1]) na--;
    while (nb && !b[nb - 1]) nb--;
    if (na != nb) return na < nb ? -1 : 1;
    for (size_t i = na; i-- > 0;)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
inline u64 bfv_wide_mod(const BfvWide &x, u64 m) {
    unsigned __int128 r = 0;
    for (size_t i = x.size(); i-- > 0;) r = ((r << 64) | x[i]) % m;
    return (u64)r;
}
inline void bfv_wide_half(BfvWide &x) {
    for (size_t i = 0; i < x.size(); i++) x[i] = (x[i] >> 1) | (i + 1 < x.size() ? x[i + 1] << 63 : 0);
}
inline BfvWide bfv_wide_product(const u64 *m, size_t cnt) {
    BfvWide x(1, 1);
    for (size_t i = 0; i < cnt; i++) bfv_wide_mul(x, m[i]);
    return x;
}

// B >= 4 t N Q: then t |x| + h < Q B / 2 for every tensor coefficient |x| <= N (Q + 1)^2 / 2 and |y| < B / 2 -- both centrings
// of the scaling are unambiguous
inline bool bfv_base_ok(const u64 *moduli_qb, size_t L, size_t M, u64 t, u64 n) {
    BfvWide need = bfv_wide_product(moduli_qb, L);
    bfv_wide_mul(need, t);
    bfv_wide_mul(need, n);
    bfv_wide_mul(need, 4);
    return bfv_wide_cmp(bfv_wide_product(moduli_qb + L, M), need) >= 0;
}

inline u64 bfv_harvey(u64 v, u64 q) { return (u64)(((unsigned __int128)v << 64) / q); }
inline u64 bfv_mul_mod(u64 a, u64 b, u64 q) { return (u64)((unsigned __int128)a * b % q); }
// a^-1 mod m by the extended Euclidean algorithm (m need not be prime: the plain modulus is only coprime to Q); 0 = not invertible
inline u64 bfv_inverse(u64 a, u64 m) {
    __int128 r0 = m, r1 = a % m, s0 = 0, s1 = 1;
    while (r1) {
        const __int128 q = r0 / r1, r2 = r0 - q * r1, s2 = s0 - q * s1;
        r0 = r1; r1 = r2; s0 = s1; s1 = s2;
    }
    if (r0 != 1) return 0;
    return (u64)(s0 < 0 ? s0 + m : s0);
}

// one direction: the K moduli x -> the T moduli y; false: two moduli of x share a factor
inline bool bfv_build_base(const u64 *x, size_t K, const u64 *y, size_t T, HpBfvBase &b) {
    memset(&b, 0, sizeof(b));
    for (size_t a = 0; a < K; a++)
        for (size_t c = 0; c < a; c++) {
            b.inv[c][a] = bfv_inverse(x[c] % x[a], x[a]);
            if (!b.inv[c][a]) return false;
            b.inv_h[c][a] = bfv_harvey(b.inv[c][a], x[a]);
        }
    BfvWide half = bfv_wide_product(x, K);
    bfv_wide_half(half);
    for (size_t a = 0; a < K; a++) {   // the digits of floor(X/2), by the recurrence the kernels run
        u64 u = bfv_wide_mod(half, x[a]);
        for (size_t c = 0; c < a; c++) u = bfv_mul_mod((u + x[a] - b.half[c] % x[a]) % x[a], b.inv[c][a], x[a]);
        b.half[a] = u;
    }
    for (size_t m = 0; m < T; m++) {
        u64 prod = 1 % y[m];
        for (size_t a = 0; a < K; a++) {
            b.pref[m][a] = prod;
            b.pref_h[m][a] = bfv_harvey(prod, y[m]);
            prod = bfv_mul_mod(prod, x[a] % y[m], y[m]);
        }
        b.prod[m] = prod;
    }
    return true;
}

// false: the moduli are not pairwise coprime (inside a base, or Q against a b_j)
inline bool bfv_build_consts(const u64 *moduli_qb, size_t L, size_t M, HpBfvConsts &c) {
    memset(&c, 0, sizeof(c));
    if (L < 1 || L > HP_BFV_MAX || M > HP_BFV_MAX) return false;
    c.L = (u32)L; c.M = (u32)M;
    const u64 *q = moduli_qb, *b = moduli_qb + L;
    if (!bfv_build_base(q, L, b, M, c.q2b) || !bfv_build_base(b, M, q, L, c.b2q)) return false;
    for (size_t j = 0; j < M; j++) {
        c.qinv_b[j] = bfv_inverse(c.q2b.prod[j], b[j]);
        if (!c.qinv_b[j]) return false;
        c.qinv_b_h[j] = bfv_harvey(c.qinv_b[j], b[j]);
    }
    BfvWide h = bfv_wide_product(q, L);
    bfv_wide_half(h);
    for (size_t m = 0; m < L + M; m++) c.h_mod[m] = bfv_wide_mod(h, moduli_qb[m]);
    return true;
}

inline void bfv_plain(const u64 *moduli_qb, size_t cnt, u64 t, HpBfvPlain &p) {
    memset(&p, 0, sizeof(p));
    for (size_t m = 0; m < cnt; m++) {
        p.t_mod[m] = t % moduli_qb[m];
        p.t_mod_h[m] = bfv_harvey(p.t_mod[m], moduli_qb[m]);
    }
}

// false: t shares a factor with Q
inline bool bfv_dec_plain(const u64 *q, size_t L, u64 t, HpBfvDecPlain &p) {
    memset(&p, 0, sizeof(p));
    p.t = t;
    p.barrett_t = ~(u64)0 / t;
    u64 prod = 1 % t;
    for (size_t a = 0; a < L; a++) {
        p.t_mod_q[a] = t % q[a];
        p.t_mod_q_h[a] = bfv_harvey(p.t_mod_q[a], q[a]);
        p.pref_t[a] = prod;
        p.pref_t_h[a] = bfv_harvey(prod, t);
        prod = bfv_mul_mod(prod, q[a] % t, t);
    }
    BfvWide h = bfv_wide_product(q, L);
    bfv_wide_half(h);
    p.h_t = bfv_wide_mod(h, t);
    p.qinv_t = bfv_inverse(prod, t);
    if (!p.qinv_t) return false;
    p.qinv_t_h = bfv_harvey(p.qinv_t, t);
    return true;
}

} // namespace hpi
