// hp_edge.hip -- coefficient-wise kernels at the edges of the headline path: the drop-last-prime helpers, the encrypt /
// decrypt cores and the RNS base transforms.  Simple one-word-per-lane streaming kernels over the tile skeleton of hp_elem.h.
#include "hp_elem.h"

// ---- drop-last-prime helpers: rescaling.cpp:54-74 / mod_switch.cpp:52-76 --------------------
// rem[p2][k][i] = strict_barrett_{q_k}(c[i]) (+ q_k - r_k if c[i] >= q_last/2) (BGV: then * t)
__global__ void __launch_bounds__(ELEM_THREADS) k_drop_rem(const HpLimb *__restrict__ limbs, HpDropConsts dc, u32 Lm1,
                                                          u32 n, u32 chunks, const u64 *__restrict__ clast,
                                                          u64 *__restrict__ rem) {
    const ElemTile tile(n, chunks);   // row = p2*Lm1 + k
    const u32 p2 = tile.row / Lm1, k = tile.row % Lm1;
    const u64 q = limbs[k].q, bc = limbs[k].barrett_c;
    const u64 bump = q - dc.r[k];
    for (const u32 i : tile.words()) {
        const u64 c = clast[(size_t)p2 * n + i];
        u64 v = hp_strict(hp_barrett_lazy(c, q, bc), q);
        if (c >= dc.half_q_last) v += bump;
        if (dc.bgv) v = hp_harvey_lazy(v, dc.t[k], dc.t_h[k], q);
        rem[(size_t)tile.row * n + i] = v;
    }
}

hipError_t hp_launch_drop_rem(const HpLimb *limbs, const HpDropConsts &dc, u32 Lm1, u32 n, u32 P2, const u64 *clast,
                              u64 *rem, hipStream_t stream) {
    return elem_launch(k_drop_rem, P2 * Lm1, n, stream, limbs, dc, Lm1, n, ElemChunks{}, clast, rem);
}

// out = ((x - rem) * inv) [* (q_last mod t)] [+ addend]     (rns.cpp:89-118, :155-171, :58-87)
__global__ void __launch_bounds__(ELEM_THREADS) k_drop_fin(const HpLimb *__restrict__ limbs, HpDropConsts dc, u32 L,
                                                          u32 kc, u32 n, u32 chunks, const u64 *__restrict__ x,
                                                          const u64 *__restrict__ rem, const u64 *__restrict__ addend,
                                                          u32 add_poly_stride, u32 add_ct_stride, u32 add_mask,
                                                          u64 *__restrict__ out) {
    // kc limbs per polynomial are processed (all L-1, or a limb range whose first limb the pointers/constants
    // have been shifted to); x rows have stride L, out rows stride L-1, rem rows are compact [P2][kc]
    const ElemTile tile(n, chunks);   // row = p2*kc + k
    const u32 p2 = tile.row / kc, k = tile.row % kc;
    const u64 q = limbs[k].q, two_q = limbs[k].two_q;
    const u64 *xs = x + ((size_t)p2 * L + k) * n;
    const u64 *as = drop_addend_row(addend, add_poly_stride, add_ct_stride, add_mask, p2, k, n);
    for (const u32 i : tile.words()) {
        u64 v = hp_sub_lazy(xs[i], rem[(size_t)tile.row * n + i], two_q);
        v = hp_harvey_lazy(v, dc.inv[k], dc.inv_h[k], q);
        if (dc.bgv) v = hp_harvey_lazy(v, dc.qlt[k], dc.qlt_h[k], q);
        if (as) v = hp_add_lazy(v, as[i], two_q);
        out[((size_t)p2 * (L - 1) + k) * n + i] = v;
    }
}

hipError_t hp_launch_drop_fin(const HpLimb *limbs, const HpDropConsts &dc, u32 L, u32 kc, u32 n, u32 P2, const u64 *x,
                              const u64 *rem, const u64 *addend, u32 add_poly_stride, u32 add_ct_stride, u32 add_mask,
                              u64 *out, hipStream_t stream) {
    if (kc == 0) return hipSuccess;
    return elem_launch(k_drop_fin, P2 * kc, n, stream, limbs, dc, L, kc, n, ElemChunks{}, x, rem, addend, add_poly_stride,
                       add_ct_stride, add_mask, out);
}

// ---- either side of the path: encrypt / decrypt cores and RNS base transforms ------
// These run once per ciphertext, not once per multiplication.

// sampling.cpp:77-83: ex[p][k][i] = q_k + (u64)e[p][i], minus q_k if that reached q_k
__global__ void __launch_bounds__(ELEM_THREADS) k_lift_noise(const HpLimb *__restrict__ limbs, u32 L, u32 n, u32 chunks,
                                                            const long long *__restrict__ noise, u64 *__restrict__ out,
                                                            u32 out_pstride) {
    const ElemTile tile(n, chunks);   // row = p*L + k
    const u32 p = tile.row / L, k = tile.row % L;
    const u64 q = limbs[k].q;
    for (const u32 i : tile.words()) {
        u64 v = q + (u64)noise[(size_t)p * n + i];
        out[((size_t)p * out_pstride + k) * n + i] = v - ((v >= q) ? q : 0);
    }
}

// Small signed polynomials as residues (hp_dev_poly_from_signed, the error rows of hp_dev_hks_keygen): out row p*out_pstride + k =
// coeffs[p] mod q_k, strict.  Unlike k_lift_noise this takes ANY int64_t: plain integer arithmetic -- Barrett on the magnitude
// (|INT64_MIN| = 2^63 is a u64 like any other; hp_barrett_lazy is below 2q for every 64-bit word), then the conditional negation
// q - r, where r = 0 stays 0.  Two coefficients per lane and round (n is even for every supported ring).  The coefficient row is
// read by the L workgroups of its moduli and the residues by the transform that follows: ordinary loads and stores.
__global__ void __launch_bounds__(ELEM_THREADS) k_spread_signed(const HpLimb *__restrict__ limbs, u32 L, u32 n, u32 chunks,
                                                               const long long *__restrict__ coeffs, u64 *__restrict__ out,
                                                               u32 out_pstride) {
    const ElemTile tile(n, chunks);   // row = p*L + k
    const u32 p = tile.row / L, k = tile.row % L;
    const u64 q = limbs[k].q, bc = limbs[k].barrett_c;
    const u64 *src = reinterpret_cast<const u64 *>(coeffs) + (size_t)p * n;
    u64 *dst = out + ((size_t)p * out_pstride + k) * n;
    const auto residue = [&](u64 c) {
        const bool neg = (long long)c < 0;
        const u64 r = hp_strict(hp_barrett_lazy(neg ? 0 - c : c, q, bc), q);
        return (neg && r) ? q - r : r;
    };
    for (const u32 i : tile.pairs()) {
        const U2 c = *reinterpret_cast<const U2 *>(src + i);
        *reinterpret_cast<U2 *>(dst + i) = U2{residue(c.x), residue(c.y)};
    }
}

// rlwe.cpp:52 and :70: c0 = (ex - c1*sk) + NTT(pt); ct[p] = (c0, c1).  ex is read from ct[p][0] (in place).
__global__ void __launch_bounds__(ELEM_THREADS) k_enc_fin(const HpLimb *__restrict__ limbs, u32 L, u32 n, u32 chunks,
                                                         const u64 *__restrict__ c1, const u64 *__restrict__ sk,
                                                         const u64 *__restrict__ ptn, u64 *__restrict__ ct) {
    const ElemTile tile(n, chunks);   // row = p*L + k
    const u32 p = tile.row / L, k = tile.row % L;
    const HpLimb m = limbs[k];
    u64 *c0 = ct + ((size_t)p * 2 * L + k) * n, *o1 = c0 + (size_t)L * n;
    const u64 *a = c1 + (size_t)tile.row * n, *s = sk + (size_t)k * n, *t = ptn + (size_t)tile.row * n;
    for (const u32 i : tile.words()) {
        const u64 av = a[i];
        u64 v = hp_sub_lazy(c0[i], hp_mul_hybrid_lazy(av, s[i], m), m.two_q);
        c0[i] = hp_add_lazy(v, t[i], m.two_q);
        o1[i] = av;
    }
}

// rlwe.cpp:76: c0 + c1*sk (the INTT and the strict reduction follow as a transform launch)
__global__ void __launch_bounds__(ELEM_THREADS) k_dec_fma(const HpLimb *__restrict__ limbs, u32 L, u32 n, u32 chunks,
                                                         const u64 *__restrict__ ct, const u64 *__restrict__ sk,
                                                         u64 *__restrict__ out) {
    const ElemTile tile(n, chunks);   // row = p*L + k
    const u32 p = tile.row / L, k = tile.row % L;
    const HpLimb m = limbs[k];
    const u64 *c0 = ct + ((size_t)p * 2 * L + k) * n, *c1 = c0 + (size_t)L * n, *s = sk + (size_t)k * n;
    for (const u32 i : tile.words()) out[(size_t)tile.row * n + i] = hp_add_lazy(c0[i], hp_mul_hybrid_lazy(c1[i], s[i], m), m.two_q);
}

// rns_transform.cpp:113 + :11-37: strict(x) mod old -> centred lift into every new modulus (+ lazy Barrett when q < old)
__global__ void __launch_bounds__(ELEM_THREADS) k_base_from_single(const HpLimb *__restrict__ limbs, u64 old_q, u32 L, u32 n,
                                                                  u32 chunks, const u64 *__restrict__ in,
                                                                  u64 *__restrict__ out) {
    const ElemTile tile(n, chunks);   // row = p*L + k
    const u32 p = tile.row / L, k = tile.row % L;
    const u64 q = limbs[k].q, bc = limbs[k].barrett_c;
    const u64 half = old_q / 2, multiple = (old_q / q + 1) * q;
    const bool reduce = q < old_q;
    for (const u32 i : tile.words()) {
        const u64 x = hp_strict(in[(size_t)p * n + i], old_q);
        u64 v = (x < half) ? x : multiple - old_q + x;
        if (reduce) v = hp_barrett_lazy(v, q, bc);
        out[(size_t)tile.row * n + i] = v;
    }
}

// rns_transform.cpp:113 + :39-84 (small-coefficient branch): consistency check over the limbs (any violation sets
// not_small[p]) and the centred lift of limb 0 into the new modulus, strictly Barrett-reduced
__global__ void __launch_bounds__(ELEM_THREADS) k_base_to_single(const HpLimb *__restrict__ limbs, u32 L, u32 n, u32 chunks,
                                                                u64 new_q, u64 new_bc, const u64 *__restrict__ in,
                                                                u64 *__restrict__ out, u32 *__restrict__ not_small) {
    const ElemTile tile(n, chunks);   // row = p
    const u32 p = tile.row;
    const u64 q0 = limbs[0].q, half = q0 / 2, multiple = (q0 / new_q + 1) * new_q;
    const u64 *x = in + (size_t)p * L * n;
    bool bad = false;
    for (const u32 i : tile.words()) {
        const u64 x0 = hp_strict(x[i], q0);
        for (u32 k = 1; k < L; k++) {
            const u64 qk = limbs[k].q, xk = hp_strict(x[(size_t)k * n + i], qk);
            bad |= (x0 < half) ? (xk != x0) : (qk - xk != q0 - x0);
        }
        const u64 v = (x0 < half) ? x0 : multiple - q0 + x0;
        out[(size_t)p * n + i] = hp_strict(hp_barrett_lazy(v, new_q, new_bc), new_q);
    }
    if (bad) atomicOr(not_small + p, 1u);
}

hipError_t hp_launch_lift_noise(const HpLimb *limbs, u32 L, u32 n, u32 P, const long long *noise, u64 *out, u32 out_pstride,
                                hipStream_t stream) {
    return elem_launch(k_lift_noise, P * L, n, stream, limbs, L, n, ElemChunks{}, noise, out, out_pstride);
}
hipError_t hp_launch_spread_signed(const HpLimb *limbs, u32 L, u32 n, u32 P, const long long *coeffs, u64 *out, u32 out_pstride,
                                   hipStream_t stream) {
    return elem_launch(k_spread_signed, P * L, n, stream, limbs, L, n, ElemChunks{}, coeffs, out, out_pstride);
}
hipError_t hp_launch_enc_fin(const HpLimb *limbs, u32 L, u32 n, u32 P, const u64 *c1, const u64 *sk, const u64 *ptn, u64 *ct,
                             hipStream_t stream) {
    return elem_launch(k_enc_fin, P * L, n, stream, limbs, L, n, ElemChunks{}, c1, sk, ptn, ct);
}
hipError_t hp_launch_dec_fma(const HpLimb *limbs, u32 L, u32 n, u32 P, const u64 *ct, const u64 *sk, u64 *out,
                             hipStream_t stream) {
    return elem_launch(k_dec_fma, P * L, n, stream, limbs, L, n, ElemChunks{}, ct, sk, out);
}
hipError_t hp_launch_base_from_single(const HpLimb *limbs, u64 old_q, u32 L, u32 n, u32 P, const u64 *in, u64 *out,
                                      hipStream_t stream) {
    return elem_launch(k_base_from_single, P * L, n, stream, limbs, old_q, L, n, ElemChunks{}, in, out);
}
hipError_t hp_launch_base_to_single(const HpLimb *limbs, u32 L, u32 n, u32 P, u64 new_q, const u64 *in, u64 *out,
                                    u32 *not_small, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(not_small, 0, (size_t)P * sizeof(u32), stream);
    if (e != hipSuccess) return e;
    return elem_launch(k_base_to_single, P, n, stream, limbs, L, n, ElemChunks{}, new_q, (~(u64)0) / new_q, in, out, not_small);
}

// rns_transform.cpp:86-104 on the device, without big integers: the mixed-radix (Garner) digits of the CRT value (hp_elem.h)
// are computed with word arithmetic, x < floor(Q/2) is a lexicographic comparison with the digits of floor(Q/2), and x mod t
// is sum v_i (q_0...q_{i-1} mod t).  The result is the reference's: x mod t below the half, t - ((Q - x) mod t) from the half
// on (which is t itself, not 0, when t | Q - x).
// Only polynomials flagged not_small are touched; the others keep the small-coefficient result.
__global__ void __launch_bounds__(ELEM_THREADS) k_base_to_single_crt(const HpLimb *__restrict__ limbs,
                                                                    const HpCrtConsts *__restrict__ cc,
                                                                    u32 L, u32 n, u32 chunks, const u64 *__restrict__ in,
                                                                    u64 *__restrict__ out, u32 out_pstride,
                                                                    const u32 *__restrict__ not_small) {
    const ElemTile tile(n, chunks);   // row = p
    const u32 p = tile.row;
    if (not_small && !not_small[p]) return;   // NULL: every polynomial takes the CRT composition
    const u64 t = cc->t;
    const u64 *x = in + (size_t)p * L * n;
    for (const u32 i : tile.words()) {
        u64 v[HP_CRT_MAX_LIMBS][1];
        for (u32 a = 0; a < L; a++) {
            const u64 qa = limbs[a].q;
            v[a][0] = hp_strict(x[(size_t)a * n + i], qa);
            garner_digit<1>(v[a], v, a, qa, limbs[a].barrett_c, cc->inv, cc->inv_h);
        }
        u64 r = 0;   // x mod t
        for (u32 a = 0; a < L; a++) {
            r += hp_strict(hp_harvey_lazy(v[a][0], cc->pref[a], cc->pref_h[a], t), t);
            r -= (r >= t) ? t : 0;
        }
        if (!garner_below<1>(v, 0, L, cc->half)) {
            u64 abs = cc->q_mod_t + t - r;   // (Q - x) mod t
            abs -= (abs >= t) ? t : 0;
            r = t - abs;
        }
        out[(size_t)p * out_pstride * n + i] = r;
    }
}

hipError_t hp_launch_base_to_single_crt(const HpLimb *limbs, const HpCrtConsts *cc, u32 L, u32 n, u32 P, const u64 *in, u64 *out,
                                        u32 out_pstride, const u32 *not_small, hipStream_t stream) {
    return elem_launch(k_base_to_single_crt, P, n, stream, limbs, cc, L, n, ElemChunks{}, in, out, out_pstride, not_small);
}
