// hp_bfv.hip -- kernels of BFV's scale-invariant multiplication and of its decryption rounding (EXTENSION, not part of hehub: see
// include/hehub_amd.h for the convention, hp_bfv.h for the constants).
//
// BFV multiplies over an enlarged basis Q B and then scales every coefficient by t / Q, rounded.  Both base conversions are EXACT
// (mixed-radix / Garner digits, word arithmetic, as ModUp / ModDown of hp_hks.hip):
//   lift     the integer centre_Q(x) behind the strict residues over Q, reduced into every b_j               k_bfv_lift (Q -> B)
//   scale    v = t x + h over Q B; r = [v]_Q in [0, Q) by Garner over Q, reduced into every b_j;
//            y = (v - r) Q^-1 mod b_j  -- the residues over B of floor((t x + h) / Q)                        k_bfv_scale
//            then centre_B(y) reduced into every q_i: the same conversion the other way round               k_bfv_lift (B -> Q)
//   decrypt  m = (h - r) Q^-1 mod t, r = [t x + h]_Q by Garner over Q, reduced mod t                         k_bfv_decrypt_round
// The scaling is two kernels, not one: the digits of Q and of B never live in registers together, so no width needs scratch
// (tests/test_bfv_resources.py prints the counts; DESIGN has them).  K is the Garner width: 1..8 exactly, 16 for the widths 9..16
// (the loops are unrolled over 16 and guarded by the run-time count).  Two coefficients per lane, 16-byte accesses, ordinary
// stores: every row written here is read again by the next launch of its call.
// Tile skeleton, launch helpers and the Garner comparison (garner_below): hp_elem.h.
#include "hp_elem.h"

// the exact width for 1..8, the guarded width 16 above
template <class F> static inline hipError_t bfv_with_width(u32 v, F f) {
    if (v >= 1 && v <= 8) return elem_with_1to8(v, f);
    if (v <= HP_BFV_MAX) return f(std::integral_constant<int, HP_BFV_MAX>{});
    return hipErrorInvalidValue;
}

// The digit loop with the digit's index as a template integer: f(std::integral_constant<int, a>) for a = 0 .. K-1.  garner_digit's
// inner loop runs to a; at the guarded width 16 the compiler leaves a loop of run-time length there, which indexes the digits in
// scratch -- with a compile-time a every index is a register's (tests/test_bfv_resources.py).
// Every digit's body starts with an empty asm that redefines the constants' base pointers, as k_hks_moddown_t does from K = 4 on: the
// scalar loads of digit a's inverses are then issued for that digit, not all K (K - 1) / 2 pairs up front, where from K = 5 on they spilled
// SGPRs (no kernel of this file may: tests/test_kernel_resources.py).
template <int A, int K, class F> HP_DEV void bfv_each_digit(F &&f) {
    if constexpr (A < K) {
        f(std::integral_constant<int, A>{});
        bfv_each_digit<A + 1, K>(f);
    }
}
// garner_digit (hp_elem.h) for digit A of two coefficients: v[A] = the residues modulo x_A on entry, the digit on return
template <int A, int K, int R, int C>
HP_DEV void bfv_digit(u64 (&v)[K][2], u64 qa, u64 bc, const u64 (&inv)[R][C], const u64 (&inv_h)[R][C]) {
    const u64 *pi = &inv[0][0], *ph = &inv_h[0][0];   // (column A, fetched four inverses at a time: see bfv_each_digit)
#pragma unroll
    for (int b = 0; b < A; b++) {
        if (b % 4 == 0 && b) asm volatile("" : "+s"(pi), "+s"(ph));
        const u64 w = pi[b * C + A], wh = ph[b * C + A];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const u64 vb = hp_strict(hp_barrett_lazy(v[b][e], qa, bc), qa);         // v_b mod x_A
            v[A][e] = hp_strict(hp_harvey_lazy(v[A][e] + qa - vb, w, wh, qa), qa);   // (u - v_b) / x_b mod x_A
        }
    }
}

// Up to this width nothing spills without the fences, and they cost time (k_bfv_scale<4>: 0.083 ms without, 0.118 ms with):
// the widths 1..4 are compiled without them.
#define BFV_PLAIN_WIDTHS 4

// a zero the compiler cannot see through: an index a + bfv_zero<K>() into the by-value constants is a load from the argument segment where
// it is used, not one of 2 K scalars fetched at the kernel's start
template <int K> HP_DEV u32 bfv_zero() {
    u32 z = 0;
    if constexpr (K > BFV_PLAIN_WIDTHS) asm volatile("" : "+s"(z));
    return z;
}

// r = sum_a v[a] * pref[a] mod qm for two coefficients, canonical (the prefix products fetched four digits at a time)
template <int K>
HP_DEV void bfv_compose(const u64 (&v)[K][2], u32 cnt, const u64 *pref, const u64 *pref_h, u64 qm, u64 (&r)[2]) {
    r[0] = r[1] = 0;
    if constexpr (K > BFV_PLAIN_WIDTHS) asm volatile("" : "+s"(cnt));   // (the K guards below are compared here, not once per kernel and kept in K scalar pairs)
#pragma unroll
    for (int a = 0; a < K; a++) {
        if constexpr (K > BFV_PLAIN_WIDTHS)
            if (a % 4 == 0) asm volatile("" : "+s"(pref), "+s"(pref_h));
        if ((u32)a < cnt) {
            const u64 w = pref[a], wh = pref_h[a];
#pragma unroll
            for (int e = 0; e < 2; e++) {
                r[e] += hp_strict(hp_harvey_lazy(v[a][e], w, wh, qm), qm);
                r[e] -= (r[e] >= qm) ? qm : 0;
            }
        }
    }
}

// Exact centred conversion of P polynomials from the base X (cnt moduli, plan xs) into the base Y (T moduli, plan ys):
// src [p][src_ps rows][n] strict coefficient rows modulo x_a in its first cnt rows -> dst [p][dst_ps rows][n], row m = the canonical
// residue modulo y_m of x if x < floor(X/2), of x - X otherwise.  Garner digits once per coefficient, then T compositions.
template <int K>
__global__ void __launch_bounds__(ELEM_THREADS) k_bfv_lift(const HpLimb *__restrict__ xs, const HpLimb *__restrict__ ys,
                                                         const HpBfvBase *__restrict__ bc, u32 cnt, u32 T, u32 n, u32 chunks,
                                                         const u64 *__restrict__ src, u32 src_ps, u64 *__restrict__ dst, u32 dst_ps) {
    const ElemTile tile(n, chunks);   // row = p
    const u64 *s = src + (size_t)tile.row * src_ps * n;
    u64 *d = dst + (size_t)tile.row * dst_ps * n;
    for (const u32 i : tile.pairs()) {
        u64 v[K][2];
        bfv_each_digit<0, K>([&](auto ac) {
            constexpr int a = decltype(ac)::value;
            if constexpr (K > BFV_PLAIN_WIDTHS) asm volatile("" : "+s"(bc), "+s"(xs));   // (bfv_each_digit: one digit's constants at a time)
            if ((u32)a < cnt) {
                const U2 in = *reinterpret_cast<const U2 *>(s + (size_t)a * n + i);
                v[a][0] = in.x;
                v[a][1] = in.y;
                bfv_digit<a>(v, xs[a].q, xs[a].barrett_c, bc->inv, bc->inv_h);
            } else {
                v[a][0] = v[a][1] = 0;
            }
        });
        // (over all K slots: the digits and the half's are both zero from cnt on, so the comparison never indexes by cnt)
        const bool below[2] = {garner_below<K>(v, 0, K, bc->half), garner_below<K>(v, 1, K, bc->half)};
        for (u32 m = 0; m < T; m++) {
            const u64 qm = ys[m].q, xm = bc->prod[m];
            u64 r[2];
            bfv_compose<K>(v, cnt, bc->pref[m], bc->pref_h[m], qm, r);
#pragma unroll
            for (int e = 0; e < 2; e++) {
                if (!below[e]) {   // x - X
                    r[e] += qm - xm;
                    r[e] -= (r[e] >= qm) ? qm : 0;
                }
            }
            *reinterpret_cast<U2 *>(d + (size_t)m * n + i) = U2{r[0], r[1]};
        }
    }
}

hipError_t hp_launch_bfv_lift(const HpLimb *xs, const HpLimb *ys, const HpBfvBase *bc, u32 cnt, u32 T, u32 n, u32 P, const u64 *src,
                              u32 src_ps, u64 *dst, u32 dst_ps, hipStream_t stream) {
    if (P == 0 || T == 0) return hipSuccess;
    return bfv_with_width(cnt, [&](auto k) {
        return elem_launch(k_bfv_lift<decltype(k)::value>, P, n, stream, xs, ys, bc, cnt, T, n, ElemChunks{}, src, src_ps, dst, dst_ps);
    });
}

// The Q-part of the scaling: src [p][L + M][n] strict coefficient rows of x over Q B -> y [p][M][n], the canonical residues modulo
// b_j of floor((t x + h) / Q):  v = t x + h residue-wise, r = [v]_Q in [0, Q) (NOT centred) by Garner over Q, y = (v - r) Q^-1.
// limbs: the plan of moduli_qb.  The t-dependent words travel by value (pc); HpBfvConsts belongs to the chain alone.
template <int K>
__global__ void __launch_bounds__(ELEM_THREADS) k_bfv_scale(const HpLimb *__restrict__ limbs, const HpBfvConsts *__restrict__ bc, HpBfvPlain pc,
                                                          u32 n, u32 chunks, const u64 *__restrict__ src, u64 *__restrict__ y) {
    const u32 L = bc->L, M = bc->M;
    const ElemTile tile(n, chunks);   // row = p
    const u64 *s = src + (size_t)tile.row * (L + M) * n;
    u64 *d = y + (size_t)tile.row * M * n;
    // t x + h modulo the modulus of row m, canonical
    const auto scaled = [&](U2 in, u32 m, u64 qm, u64 (&o)[2]) {
        const u64 tm = pc.t_mod[m], tmh = pc.t_mod_h[m], hm = bc->h_mod[m];
        o[0] = hp_strict(hp_harvey_lazy(in.x, tm, tmh, qm), qm) + hm;
        o[1] = hp_strict(hp_harvey_lazy(in.y, tm, tmh, qm), qm) + hm;
        o[0] -= (o[0] >= qm) ? qm : 0;
        o[1] -= (o[1] >= qm) ? qm : 0;
    };
    for (const u32 i : tile.pairs()) {
        u64 v[K][2];
        bfv_each_digit<0, K>([&](auto ac) {
            constexpr int a = decltype(ac)::value;
            if constexpr (K > BFV_PLAIN_WIDTHS) asm volatile("" : "+s"(bc), "+s"(limbs));   // (bfv_each_digit: one digit's constants at a time)
            if ((u32)a < L) {
                scaled(*reinterpret_cast<const U2 *>(s + (size_t)a * n + i), a + bfv_zero<K>(), limbs[a].q, v[a]);
                bfv_digit<a>(v, limbs[a].q, limbs[a].barrett_c, bc->q2b.inv, bc->q2b.inv_h);
            } else {
                v[a][0] = v[a][1] = 0;
            }
        });
        for (u32 j = 0; j < M; j++) {
            const u64 bj = limbs[L + j].q, qi = bc->qinv_b[j], qih = bc->qinv_b_h[j];
            u64 r[2], w[2];
            bfv_compose<K>(v, L, bc->q2b.pref[j], bc->q2b.pref_h[j], bj, r);
            scaled(*reinterpret_cast<const U2 *>(s + (size_t)(L + j) * n + i), L + j, bj, w);
#pragma unroll
            for (int e = 0; e < 2; e++) {
                w[e] += bj - r[e];
                w[e] -= (w[e] >= bj) ? bj : 0;
                w[e] = hp_strict(hp_harvey_lazy(w[e], qi, qih, bj), bj);
            }
            *reinterpret_cast<U2 *>(d + (size_t)j * n + i) = U2{w[0], w[1]};
        }
    }
}

hipError_t hp_launch_bfv_scale(const HpLimb *limbs, const HpBfvConsts *bc, const HpBfvPlain &pc, u32 L, u32 n, u32 P, const u64 *src, u64 *y,
                               hipStream_t stream) {
    if (P == 0) return hipSuccess;
    return bfv_with_width(L, [&](auto k) {
        return elem_launch(k_bfv_scale<decltype(k)::value>, P, n, stream, limbs, bc, pc, n, ElemChunks{}, src, y);
    });
}

// Decryption rounding: x [p][L][n] strict coefficient rows of x in [0, Q) -> m [p][n] = floor((t x + h) / Q) mod t, words below t:
// r = [t x + h]_Q by Garner over Q, reduced modulo t digit by digit, then (h - r) Q^-1 mod t.  t is any modulus of two or more
// coprime to Q (even ones too): Barrett and Harvey words modulo t are exact for every 64-bit operand.
template <int K>
__global__ void __launch_bounds__(ELEM_THREADS) k_bfv_decrypt_round(const HpLimb *__restrict__ limbs, const HpBfvConsts *__restrict__ bc,
                                                                  HpBfvDecPlain pc, u32 n, u32 chunks, const u64 *__restrict__ x,
                                                                  u64 *__restrict__ out) {
    const u32 L = bc->L;
    const ElemTile tile(n, chunks);   // row = p
    const u64 *s = x + (size_t)tile.row * L * n;
    u64 *d = out + (size_t)tile.row * n;
    const u64 t = pc.t;
    for (const u32 i : tile.pairs()) {
        u64 v[K][2];
        bfv_each_digit<0, K>([&](auto ac) {
            constexpr int a = decltype(ac)::value;
            if constexpr (K > BFV_PLAIN_WIDTHS) asm volatile("" : "+s"(bc), "+s"(limbs));   // (bfv_each_digit: one digit's constants at a time)
            if ((u32)a < L) {
                const u32 az = a + bfv_zero<K>();
                const u64 qa = limbs[a].q, tm = pc.t_mod_q[az], tmh = pc.t_mod_q_h[az], hm = bc->h_mod[a];
                const U2 in = *reinterpret_cast<const U2 *>(s + (size_t)a * n + i);
                v[a][0] = hp_strict(hp_harvey_lazy(in.x, tm, tmh, qa), qa) + hm;
                v[a][1] = hp_strict(hp_harvey_lazy(in.y, tm, tmh, qa), qa) + hm;
                v[a][0] -= (v[a][0] >= qa) ? qa : 0;
                v[a][1] -= (v[a][1] >= qa) ? qa : 0;
                bfv_digit<a>(v, qa, limbs[a].barrett_c, bc->q2b.inv, bc->q2b.inv_h);
            } else {
                v[a][0] = v[a][1] = 0;
            }
        });
        u64 r[2] = {0, 0};
        u32 cnt = L;
        if constexpr (K > BFV_PLAIN_WIDTHS) asm volatile("" : "+s"(cnt));   // (as in bfv_compose)
#pragma unroll
        for (int a = 0; a < K; a++) {
            if ((u32)a < cnt) {
                const u32 az = a + bfv_zero<K>();
                const u64 w = pc.pref_t[az], wh = pc.pref_t_h[az];
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const u64 va = hp_strict(hp_barrett_lazy(v[a][e], t, pc.barrett_t), t);
                    r[e] += hp_strict(hp_harvey_lazy(va, w, wh, t), t);
                    r[e] -= (r[e] >= t) ? t : 0;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 2; e++) {
            r[e] = pc.h_t + t - r[e];
            r[e] -= (r[e] >= t) ? t : 0;
            r[e] = hp_strict(hp_harvey_lazy(r[e], pc.qinv_t, pc.qinv_t_h, t), t);
        }
        *reinterpret_cast<U2 *>(d + i) = U2{r[0], r[1]};
    }
}

hipError_t hp_launch_bfv_decrypt_round(const HpLimb *limbs, const HpBfvConsts *bc, const HpBfvDecPlain &pc, u32 L, u32 n, u32 P, const u64 *x,
                                       u64 *out, hipStream_t stream) {
    if (P == 0) return hipSuccess;
    return bfv_with_width(L, [&](auto k) {
        return elem_launch(k_bfv_decrypt_round<decltype(k)::value>, P, n, stream, limbs, bc, pc, n, ElemChunks{}, x, out);
    });
}

// The output contract of the BFV calls: rows of any u64 words (lazy transform words, a caller's words below 2q) -> the canonical
// residue, one reduction after the last transform.  R rows per polynomial, row k of modulus limbs[k]; src == dst: in place.
__global__ void __launch_bounds__(ELEM_THREADS) k_bfv_canonical(const HpLimb *__restrict__ limbs, u32 R, u32 n, u32 chunks,
                                                              const u64 *src, u32 src_ps, u64 *dst, u32 dst_ps) {
    const ElemTile tile(n, chunks);   // row = p * R + k
    const u32 p = tile.row / R, k = tile.row % R;
    const u64 q = limbs[k].q, c = limbs[k].barrett_c;
    const u64 *s = src + ((size_t)p * src_ps + k) * n;
    u64 *d = dst + ((size_t)p * dst_ps + k) * n;
    for (const u32 i : tile.pairs()) {
        const U2 v = *reinterpret_cast<const U2 *>(s + i);
        *reinterpret_cast<U2 *>(d + i) = U2{hp_strict(hp_barrett_lazy(v.x, q, c), q), hp_strict(hp_barrett_lazy(v.y, q, c), q)};
    }
}

hipError_t hp_launch_bfv_canonical(const HpLimb *limbs, u32 R, u32 n, u32 P, const u64 *src, u32 src_ps, u64 *dst, u32 dst_ps,
                                   hipStream_t stream) {
    if (P == 0 || R == 0) return hipSuccess;
    return elem_launch(k_bfv_canonical, P * R, n, stream, limbs, R, n, ElemChunks{}, src, src_ps, dst, dst_ps);
}
