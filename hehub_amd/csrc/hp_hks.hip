// hp_hks.hip -- kernels of the hybrid key switch (EXTENSION, not part of hehub: see include/hehub_amd.h).
//
// hehub switches keys with one digit per RNS limb and one special prime: L digits, L*(L+1) digit transforms per
// switch (rgsw.cpp:57-156).  The hybrid variant groups alpha consecutive limbs into one digit (dnum = ceil(L/alpha)
// digits) and uses k special primes P = p_0...p_{k-1} >= the largest digit: dnum*(L+k) - L transforms instead of L*L.
// It needs keys in its own format (one row per digit), so it can never be bit-compatible with hehub's keys; it is
// pinned by an exact integer model and by decryption (tests/test_hks.py).
//
//   ModUp    digit d = limbs [d*alpha, ...): the EXACT integer x_d in [0, Q_d) behind its residues (mixed-radix / Garner
//            digits, word arithmetic) reduced into every other modulus of q_0..q_{L-1}, p_0..p_{k-1}
//   inner    out[half][m] = montgomery( sum_d D[d][m] * key[d][half][m] ), D[d][m] = NTT_m(lift) or the input limb itself
//            when m belongs to digit d -- the same 128-bit accumulation as hehub's inner product
//   ModDown  the P-part of the result, centred exactly (hp_edge.hip: k_base_to_single_crt), is subtracted and the rest
//            multiplied by P^-1:  out = (x - NTT(rem)) * P^-1 [+ addend]
//            BGV (a plain modulus t): the remainder is t * centre([x]_P t^-1 mod P), so that the quotient keeps x's value mod t
//   keygen   the keys themselves from the caller's samples: key_d = ((NTT(e) - a s_to + [digit d] (P mod q) s_from) 2^64, a 2^64)
// Tile skeleton, launch helpers and the Garner digits shared with hp_edge.hip: hp_elem.h.
#include "hp_elem.h"

// lifted[p][d][m][i] = x_d mod modulus_m for every modulus m outside digit d (slots inside the digit are not written).
// Two coefficients per lane and iteration: 16-byte accesses (n is even for every supported ring).
template <int ALPHA>
__global__ void __launch_bounds__(ELEM_THREADS) k_hks_modup(const HpLimb *__restrict__ limbs, const HpHksConsts *__restrict__ hc,
                                                          u32 n, u32 chunks, const u64 *__restrict__ coef,
                                                          u64 *__restrict__ lifted) {
    const u32 L = hc->L, E = hc->E, nd = hc->nd;
    const ElemTile tile(n, chunks);   // row = p*nd + d
    const u32 p = tile.row / nd, d = tile.row % nd;
    const u32 first = d * hc->alpha, cnt = min(hc->alpha, L - first);   // limbs of this digit
    const u64 *src = coef + ((size_t)p * L + first) * n;
    u64 *dst = lifted + (size_t)tile.row * E * n;
    for (const u32 i : tile.pairs()) {
        u64 v[ALPHA][2];
#pragma unroll
        for (int a = 0; a < ALPHA; a++) {
            if ((u32)a < cnt) {
                const U2 in = *reinterpret_cast<const U2 *>(src + (size_t)a * n + i);   // strict residues
                v[a][0] = in.x;
                v[a][1] = in.y;
                garner_digit<ALPHA>(v[a], v, a, limbs[first + a].q, limbs[first + a].barrett_c, hc->inv[d], hc->inv_h[d]);
            } else {
                v[a][0] = v[a][1] = 0;
            }
        }
        for (u32 m = 0; m < E; m++) {
            if (m >= first && m < first + cnt) continue;
            const u64 qm = limbs[m].q;
            u64 r[2] = {0, 0};
#pragma unroll
            for (int a = 0; a < ALPHA; a++) {
                if ((u32)a < cnt) {
                    const u64 w = hc->pref[d][m][a], wh = hc->pref_h[d][m][a];
#pragma unroll
                    for (int e = 0; e < 2; e++) {
                        r[e] += hp_strict(hp_harvey_lazy(v[a][e], w, wh, qm), qm);
                        r[e] -= (r[e] >= qm) ? qm : 0;
                    }
                }
            }
            U2 o{r[0], r[1]};
            *reinterpret_cast<U2 *>(dst + (size_t)m * n + i) = o;
        }
    }
}

hipError_t hp_launch_hks_modup(const HpLimb *limbs, const HpHksConsts *hc, u32 alpha, u32 nd, u32 n, u32 P, const u64 *coef,
                               u64 *lifted, hipStream_t stream) {
    return elem_with_1to8(alpha, [&](auto a) {
        return elem_launch(k_hks_modup<decltype(a)::value>, P * nd, n, stream, limbs, hc, n, ElemChunks{}, coef, lifted);
    });
}

// out[p][half][m][i] = montgomery_128( sum_d D[p][d][m][i] * key[d][half][m][i] ); PT ciphertexts share each key word.
// The key may have been generated for a longer chain (the _at entry points): its digits have KE >= E rows, of which row
// km = m + (m >= L ? KE - E : 0) belongs to modulus m of this level -- the ciphertext moduli first, the special primes last.  m is the
// workgroup's, so km is one scalar; every internal row (digits, accumulators) stays indexed by m over E.  (hks_key_row: all inner kernels)
__device__ __forceinline__ u32 hks_key_row(u32 m, u32 L, u32 E, u32 KE) { return m + (m >= L ? KE - E : 0u); }

// The digit sum every inner product of this file is built on: acc[c][half][word] = sum_d D_c[d][m] * key[d][half][m] at the thread's
// pair of words, for the PT polynomials c of the thread.  D_c[d][m] is the caller's own row own_row[c] where m belongs to digit d
// (own: that digit; nd for a special prime, which belongs to none), else row (poly[c], d, m) of the lifted digits.
// LD says how the words come in (its i: the thread's pair):
//   HksStreamedPair  the digit pair at i, read once per launch: non-temporal; the key is shared by the whole batch: cached
//   HksMovedPair     the digit pair moved by a rotation (MovedPair, hp_elem.h); the rotation's key is read once per launch: non-temporal
// A kernel supplies its workgroup numbering (m, the polynomials, the chunk), the rows, and the tail: what becomes of acc.
struct HksStreamedPair {
    u32 i;
    HP_DEV U2 key(const u64 *row) const { return *reinterpret_cast<const U2 *>(row + i); }
    HP_DEV U2 digit(const u64 *row) const { return ld_nt(row + i); }
};
struct HksMovedPair {
    u32 i;
    MovedPair moved;
    HP_DEV HksMovedPair(const u32 *map, u32 n, u32 i) : i(i), moved(map, n, i) {}
    HP_DEV U2 key(const u64 *row) const { return ld_nt(row + i); }
    HP_DEV U2 digit(const u64 *row) const { return moved(row); }
};
template <int PT, class LD>
HP_DEV void hks_digit_sum(HpAcc (&acc)[PT][2][2], const LD &ld, const u64 *__restrict__ key, u32 KE, u32 km, u32 nd, u32 own,
                          const u64 *const (&own_row)[PT], const u64 *__restrict__ lifted, const size_t (&poly)[PT], u32 E, u32 m, u32 n) {
    acc_zero(acc);
    for (u32 d = 0; d < nd; d++) {
        const U2 g0 = ld.key(key + (((size_t)d * 2 + 0) * KE + km) * n);
        const U2 g1 = ld.key(key + (((size_t)d * 2 + 1) * KE + km) * n);
#pragma unroll
        for (int c = 0; c < PT; c++)
            key_mac(g0, g1, ld.digit((d == own) ? own_row[c] : lifted + ((poly[c] * nd + d) * E + m) * n), acc[c]);
    }
}

template <int PT>
__global__ void __launch_bounds__(ELEM_THREADS) k_hks_inner(const HpLimb *__restrict__ limbs, u32 L, u32 E, u32 KE, u32 nd, u32 alpha, u32 P,
                                                          u32 n, u32 chunks, const u64 *__restrict__ lifted,
                                                          const u64 *__restrict__ pt, u32 pt_pstride,
                                                          const u64 *__restrict__ key, u64 *__restrict__ out) {
    const u32 PG = (P + PT - 1) / PT;
    const ElemTile tile(n, chunks);
    const u32 m = tile.row / PG, p0 = (tile.row % PG) * PT, km = hks_key_row(m, L, E, KE);
    const u64 q = limbs[m].q, mqinv = limbs[m].mqinv;
    const u32 own = (m < L) ? m / alpha : nd;
    const u64 *own_row[PT];
    size_t poly[PT];
#pragma unroll
    for (int c = 0; c < PT; c++) {
        poly[c] = min(p0 + c, P - 1);   // a ragged last group re-reads its last ciphertext and skips the store
        own_row[c] = pt + (poly[c] * pt_pstride + m) * n;
    }
    for (const u32 i : tile.pairs()) {
        HpAcc acc[PT][2][2];
        hks_digit_sum(acc, HksStreamedPair{i}, key, KE, km, nd, own, own_row, lifted, poly, E, m, n);
        acc_store_montgomery(acc, p0, P, q, mqinv, out + ((size_t)p0 * 2 * E + m) * n + i, (size_t)2 * E * n, (size_t)E * n);
    }
}

hipError_t hp_launch_hks_inner(const HpLimb *limbs, u32 L, u32 E, u32 KE, u32 nd, u32 alpha, u32 n, u32 P, const u64 *lifted, const u64 *pt,
                               u32 pt_pstride, const u64 *key, u64 *out, hipStream_t stream) {
    if (KE < E) return hipErrorInvalidValue;
    // two ciphertexts per thread (four: the column accumulators halve the occupancy, measured -5 %)
    const u32 PT = P >= 2 ? 2 : 1;
    return elem_launch(PT == 2 ? k_hks_inner<2> : k_hks_inner<1>, ((P + PT - 1) / PT) * E, n, stream, limbs, L, E, KE, nd, alpha, P, n,
                       ElemChunks{}, lifted, pt, pt_pstride, key, out);
}

// Hoisted rotations (hp_dev_ckks_rotate_hoisted_hks): the digit rows of the UNROTATED c1 are built once and every rotation r reads
// them through its own map -- k_hks_inner with the digit operand gathered:
//   out[b][r][half][m][i] = montgomery_128( sum_d D[b][d][m][map_r(i)] * key_r[d][half][m][i] )
// (the same accumulation order and tail as k_hks_inner: the words follow the model).  Keys and maps are kernel arguments.
// Key words are read once per launch: streamed, non-temporal.  The digit rows -- nd rows of 8N bytes per (b, m) -- are read again
// by every rotation, scattered over the whole row: ordinary cached loads, and a numbering of the workgroups that keeps the rows
// in ONE XCD's L2 while they are needed.  A unit = one modulus m and one group of PT ciphertexts, R * chunks workgroups.
// Workgroups are dealt round-robin over the 8 XCDs, so of eight consecutive ids each goes to its own unit: an XCD works through
// all rotations and chunks of one unit (at N = 32768: 1 MiB of digit rows per ciphertext, 4 MiB of L2) before it takes the next.
// The units that do not fill a group of eight are numbered plainly -- their rows get fetched by every XCD (from the Infinity
// Cache after the first) -- so that no XCD idles.  A speed matter only: any placement computes the same words.
template <int PT>
__global__ void __launch_bounds__(ELEM_THREADS) k_hks_inner_hoisted(const HpLimb *__restrict__ limbs, u32 L, u32 E, u32 KE, u32 nd, u32 alpha,
                                                                  u32 P, u32 R, u32 n, u32 chunks, const u64 *__restrict__ lifted,
                                                                  const u64 *__restrict__ pt, u32 pt_pstride, HpHoistTable tab,
                                                                  u64 *__restrict__ out) {
    const u32 PG = (P + PT - 1) / PT, units = E * PG, W = R * chunks;
    u32 unit, w;
    hp_xcd_unit(blockIdx.x, units, W, unit, w);
    const u32 m = unit / PG, p0 = (unit % PG) * PT, r = w / chunks, km = hks_key_row(m, L, E, KE);
    const ElemTile tile(ElemTile::At{unit, w % chunks}, n);
    const u64 q = limbs[m].q, mqinv = limbs[m].mqinv;
    const u32 own = (m < L) ? m / alpha : nd;
    const u64 *__restrict__ key = tab.key[r];
    const u32 *__restrict__ map = tab.map[r];   // NULL: the involution
    const u64 *own_row[PT];
    size_t poly[PT];
#pragma unroll
    for (int c = 0; c < PT; c++) {
        poly[c] = min(p0 + c, P - 1);
        own_row[c] = pt + (poly[c] * pt_pstride + m) * n;
    }
    for (const u32 i : tile.pairs()) {
        HpAcc acc[PT][2][2];
        hks_digit_sum(acc, HksMovedPair(map, n, i), key, KE, km, nd, own, own_row, lifted, poly, E, m, n);
        acc_store_montgomery(acc, p0, P, q, mqinv, out + ((((size_t)p0 * R + r) * 2) * E + m) * n + i, (size_t)R * 2 * E * n, (size_t)E * n);
    }
}

hipError_t hp_launch_hks_inner_hoisted(const HpLimb *limbs, u32 L, u32 E, u32 KE, u32 nd, u32 alpha, u32 n, u32 P, u32 R, const u64 *lifted,
                                       const u64 *pt, u32 pt_pstride, const HpHoistTable &tab, u64 *out, hipStream_t stream) {
    if (P == 0 || R == 0) return hipSuccess;
    if (R > HP_HOIST_TABLE_MAX || KE < E) return hipErrorInvalidValue;
    // two ciphertexts per thread share the key words and the map's pair, as in k_hks_inner
    const u32 PT = P >= 2 ? 2 : 1, chunks = (n + ELEM_CHUNK - 1) / ELEM_CHUNK;
    const auto k = PT == 2 ? k_hks_inner_hoisted<2> : k_hks_inner_hoisted<1>;
    k<<<dim3(((P + PT - 1) / PT) * E * R * chunks, 1, 1), ELEM_THREADS, 0, stream>>>(limbs, L, E, KE, nd, alpha, P, R, n, chunks, lifted, pt,
                                                                                 pt_pstride, tab, out);
    return hipGetLastError();
}

// Diagonal linear transform in the extended basis (hp_dev_ckks_lintrans_hks): k_hks_inner_hoisted with the rotation loop INSIDE the
// thread.  A thread owns one pair of words of acc[b][.][m] and, for every rotation r of the table, runs the digit sum of the hoisted
// kernel (hks_digit_sum over HksMovedPair), reduces it to a word w_r (Montgomery: the keys carry the 2^64) and multiplies it by the
// diagonal's word into a SECOND set of carry-save columns:
//   acc[b][h][m][i] = sum_r diag_r[m][i] * w_r,      w_r = montgomery_128( sum_d D[b][d][m][map_r(i)] * key_r[d][h][m][i] )
// The diagonals are plain words: the outer sum ends in the tail of a sum of plain products (acc_store_plain, hp_elem.h), below 2q.
// The c0 term of the rotation is folded in rather than kept as a third accumulator and an addend row: on polynomial 0 and the
// ciphertext moduli the word (P mod q) * map_r(c0) is added to w_r before the diagonal multiplies it -- ModDown divides P out exactly
// and the special-prime limbs see a multiple of P, i.e. nothing.  One gathered load and one Harvey product per rotation on 1/(2(1+k/L))
// of the rows, against 8 more VGPRs per word and an addend row written and read.
// Ranges: w_r + the folded word < 4 nd ceil(q^2 / 2^64) + 3q, times a diagonal word < 2q, summed over R: the host keeps that below
// 2^128 (hpi::hks_lintrans_max_rotations, hp_drop.h: 32 rotations for every modulus below 2^59).  A diagonal word of 2q or more can
// make the sum wrap unnoticed: the residues are then undefined.
// That bound for w_r takes every digit word below 2q.  The caller's own rows are; the lifted rows at level B are hehub's lazy
// transform words, which exceed 2q where the modulus sits far below its power of two (kb = round(log2 q), fix = 0, large
// 2^kb - q: hp::lazy_fold_bound's word_end).  Measured on a chain of 58- and 59-bit moduli with 16 digits and 32 rotations
// (tests/test_hks_edges.py): digit words up to 4.24 q at the 58-bit moduli near 1.6 * 2^58 (N = 1024), the digit sum up to 2^123.97,
// w_r + the folded word up to 2^60.85 -- still under the bound, 2^61.32 there, which is taken at the LARGEST modulus of the chain
// while only moduli a good way below a power of two have such rows -- and the outer sum up to 2^125.50.  With lazy_fold_bound's
// largest word for any modulus the transforms accept (log_modulus <= 59, N <= 65536: under 11 q at q = 2^58.5) the same arithmetic
// gives 2^125.4, 2^61.9 and 2^126.4: both sums fit 128 bits and the word fits 64 at every supported modulus, so the host formula
// stands although its premise does not.
// Workgroups: one pair per thread (chunks of 2 * ELEM_THREADS words -- the rotations no longer widen the grid), units = (modulus,
// ciphertext) numbered by XCD as in the hoisted kernel: the digit rows of a unit are now read R times by the SAME workgroups.
// Unmeasured for this kernel.  One ciphertext per thread at every batch: two sets of accumulators already leave 4 waves per SIMD.
// Flavours (hp_dev_ckks_lintrans_bsgs_hks; FLAV is a compile-time branch, the flat flavour's code is what it was):
//   HKS_LT_GIANT  rotation r reads ITS OWN polynomial p * Rtot + r -- digit rows and the rows (u0, u1) where the flat call has (c0, c1) --
//                 and there is no diagonal: the sum over the giants of one ciphertext, the words w_r summed with weight 1
//   HKS_LT_BABY   nothing is summed: the rotations widen the grid as in the hoisted kernel and the word w_r + the folded word goes
//                 to row set p * Rtot + r as it is (a 64-bit word under the bound above, which is what the pre-sum's range argument
//                 takes).  A NULL key is the identity: (P mod q) * c_h on the ciphertext moduli, zero on the special primes.
//                 The rows are read again by the pre-sum: ordinary stores.
#define HKS_LT_CHUNK (2u * ELEM_THREADS)
enum { HKS_LT_FLAT = 0, HKS_LT_GIANT = 1, HKS_LT_BABY = 2 };
template <int FLAV>
__global__ void __launch_bounds__(ELEM_THREADS) k_hks_inner_lintrans(const HpLimb *__restrict__ limbs, const HpHksConsts *__restrict__ hc,
                                                                   u32 KE, u32 P, u32 R, u32 Rtot, u32 n, u32 chunks,
                                                                   const u64 *__restrict__ lifted, const u64 *__restrict__ ct,
                                                                   HpLinTable tab, u32 add_prev, u64 *__restrict__ out) {
    const u32 L = hc->L, E = hc->E, nd = hc->nd, alpha = hc->alpha;
    const u32 units = E * P, W = FLAV == HKS_LT_BABY ? R * chunks : chunks;
    u32 unit, w;
    HP_XCD_UNIT(blockIdx.x, units, W, unit, w)   // (hp_device.h: why not the function here)
    const u32 m = unit / P, p = unit % P, km = hks_key_row(m, L, E, KE);   // (keys and diagonals: rows of the chain they were made for)
    const ElemTile tile(ElemTile::At{unit, w % chunks}, n, HKS_LT_CHUNK);
    const u32 r_first = FLAV == HKS_LT_BABY ? w / chunks : 0, r_end = FLAV == HKS_LT_BABY ? r_first + 1 : R;
    const u64 q = limbs[m].q, mqinv = limbs[m].mqinv, two_q = limbs[m].two_q, r64 = limbs[m].r64, r64h = limbs[m].r64h;
    const u32 own = (m < L) ? m / alpha : nd;
    const bool fold = m < L;                    // polynomial 0 of these rows takes the c0 term
    const u64 pm = fold ? hc->p_mod_q[m] : 0, pmh = fold ? hc->p_mod_q_h[m] : 0;
    for (const u32 i : tile.pairs()) {
        HpAcc sum[2][2];   // the outer sum over the rotations
        acc_zero(sum);
        for (u32 r = r_first; r < r_end; r++) {
            const u64 *__restrict__ key = tab.key[r];
            const u32 *__restrict__ map = tab.map[r];   // NULL: the involution
            const u64 *__restrict__ dg = FLAV == HKS_LT_FLAT ? tab.diag[r] : nullptr;   // NULL: the constant 1
            const size_t pr[1] = {FLAV == HKS_LT_GIANT ? (size_t)p * Rtot + r : p};           // the polynomial rotation r reads
            const u64 *__restrict__ c0row = ct + (pr[0] * 2 * L + m) * n;   // a ciphertext is 2 L rows: c0, then c1
            const u64 *const c1row[1] = {c0row + (size_t)L * n};
            if (FLAV == HKS_LT_BABY && !key) {   // the identity baby
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    U2 v{0, 0};
                    if (fold) {
                        v = *reinterpret_cast<const U2 *>((h ? c1row[0] : c0row) + i);
                        v.x = hp_harvey_lazy(v.x, pm, pmh, q);
                        v.y = hp_harvey_lazy(v.y, pm, pmh, q);
                    }
                    *reinterpret_cast<U2 *>(out + ((((size_t)p * Rtot + r) * 2 + h) * E + m) * n + i) = v;
                }
                continue;
            }
            const HksMovedPair ld(map, n, i);
            U2 dw{1, 1};
            if (dg) dw = *reinterpret_cast<const U2 *>(dg + (size_t)km * n + i);
            U2 c0{0, 0};
            if (fold) c0 = ld.moved(c0row);
            HpAcc acc[1][2][2];
            hks_digit_sum(acc, ld, key, KE, km, nd, own, c1row, lifted, pr, E, m, n);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                U2 v = acc2_montgomery(acc[0][h][0], acc[0][h][1], q, mqinv);
                if (h == 0 && fold) {
                    v.x += hp_harvey_lazy(c0.x, pm, pmh, q);
                    v.y += hp_harvey_lazy(c0.y, pm, pmh, q);
                }
                if (FLAV == HKS_LT_BABY) *reinterpret_cast<U2 *>(out + ((((size_t)p * Rtot + r) * 2 + h) * E + m) * n + i) = v;
                else hp_mac2(sum[h][0], v.x, dw.x, sum[h][1], v.y, dw.y);
            }
        }
        if (FLAV == HKS_LT_BABY) continue;
#pragma unroll
        for (int h = 0; h < 2; h++)
            acc_store_plain(sum[h][0], sum[h][1], q, mqinv, two_q, r64, r64h, add_prev, out + (((size_t)p * 2 + h) * E + m) * n + i);
    }
}

template <int FLAV>
static hipError_t hks_lintrans_launch(const HpLimb *limbs, const HpHksConsts *hc, u32 E, u32 KE, u32 n, u32 P, u32 R, u32 Rtot,
                                      const u64 *lifted, const u64 *ct, const HpLinTable &tab, bool add_prev, u64 *out, hipStream_t stream) {
    if (P == 0 || R == 0) return hipSuccess;
    if (R > HP_HOIST_TABLE_MAX || KE < E) return hipErrorInvalidValue;
    const u32 chunks = (n + HKS_LT_CHUNK - 1) / HKS_LT_CHUNK, W = FLAV == HKS_LT_BABY ? R * chunks : chunks;
    k_hks_inner_lintrans<FLAV><<<dim3(P * E * W, 1, 1), ELEM_THREADS, 0, stream>>>(limbs, hc, KE, P, R, Rtot, n, chunks, lifted, ct, tab,
                                                                                 add_prev ? 1u : 0u, out);
    return hipGetLastError();
}
hipError_t hp_launch_hks_inner_lintrans(const HpLimb *limbs, const HpHksConsts *hc, u32 E, u32 KE, u32 n, u32 P, u32 R, const u64 *lifted,
                                        const u64 *ct, const HpLinTable &tab, bool add_prev, u64 *acc, hipStream_t stream) {
    return hks_lintrans_launch<HKS_LT_FLAT>(limbs, hc, E, KE, n, P, R, R, lifted, ct, tab, add_prev, acc, stream);
}
hipError_t hp_launch_hks_bsgs_babies(const HpLimb *limbs, const HpHksConsts *hc, u32 E, u32 KE, u32 n, u32 P, u32 R, u32 Rtot,
                                     const u64 *lifted, const u64 *ct, const HpLinTable &tab, u64 *baby, hipStream_t stream) {
    return hks_lintrans_launch<HKS_LT_BABY>(limbs, hc, E, KE, n, P, R, Rtot, lifted, ct, tab, false, baby, stream);
}
hipError_t hp_launch_hks_bsgs_giants(const HpLimb *limbs, const HpHksConsts *hc, u32 E, u32 KE, u32 n, u32 P, u32 R, u32 Rtot,
                                     const u64 *lifted, const u64 *u, const HpLinTable &tab, bool add_prev, u64 *acc, hipStream_t stream) {
    return hks_lintrans_launch<HKS_LT_GIANT>(limbs, hc, E, KE, n, P, R, Rtot, lifted, u, tab, add_prev, acc, stream);
}

// Pre-sum of the baby-step giant-step transform: pre_g = sum_i diag_{g,i} * baby_i in the extended basis, the outer sum of the flat
// kernel with the inner product already done (the baby rows).  A thread owns one pair of words of (b, m) for BOTH halves -- one
// diagonal load serves h = 0 and h = 1 -- and a tile of GT giants: a baby pair is loaded once per tile, so a baby row is read
// ceil(giants / GT) times per launch (ordinary cached loads), a diagonal word once per call (non-temporal).  The table is a kernel
// argument: an absent diagonal is a NULL that the whole wave sees, and costs no load.  The tail is the flat kernel's
// (acc_store_plain).  Ranges: a baby word is below the flat
// kernel's bound for w_r plus the folded word, a diagonal word below 2q, `babies` of them per launch (hpi::hks_bsgs_plan).
// GT = 4: 16 accumulators of 8 VGPRs; the counts are in DESIGN 4.7b (tests/test_bsgs_resources.py prints them).
// Workgroups: row = ((b * E + m) * tiles + tile), plain numbering -- the tiles of one (b, m) read the same baby rows and are
// `chunks` workgroups apart.  Unmeasured.
#define HKS_PRE_GT 4
template <int GT>
__global__ void __launch_bounds__(ELEM_THREADS) k_hks_bsgs_presum(const HpLimb *__restrict__ limbs, u32 L, u32 E, u32 KE, u32 G, u32 Bn, u32 n, u32 chunks,
                                                                const u64 *__restrict__ baby, size_t baby_pstride, HpPreTable tab,
                                                                size_t dst_pstride, u32 add_prev) {
    const u32 tiles = (G + GT - 1) / GT;
    const ElemTile tile(n, chunks, HKS_LT_CHUNK);
    const u32 g0 = (tile.row % tiles) * GT, m = (tile.row / tiles) % E, b = tile.row / (tiles * E);
    const u32 km = hks_key_row(m, L, E, KE);   // the diagonal's row of modulus m (a diagonal has KE rows)
    const u64 q = limbs[m].q, mqinv = limbs[m].mqinv, two_q = limbs[m].two_q, r64 = limbs[m].r64, r64h = limbs[m].r64h;
    const u64 *__restrict__ brow = baby + (size_t)b * baby_pstride + (size_t)m * n;   // baby i, half h: + (i * 2 + h) * E * n
    for (const u32 i : tile.pairs()) {
        HpAcc sum[GT][2][2];
        acc_zero(sum);
        for (u32 j = 0; j < Bn; j++) {
            const U2 v0 = *reinterpret_cast<const U2 *>(brow + ((size_t)j * 2 + 0) * E * n + i);
            const U2 v1 = *reinterpret_cast<const U2 *>(brow + ((size_t)j * 2 + 1) * E * n + i);
#pragma unroll
            for (int c = 0; c < GT; c++) {
                const u64 *__restrict__ dg = g0 + c < G ? tab.diag[(g0 + c) * Bn + j] : nullptr;
                if (dg) {
                    const U2 dw = ld_nt(dg + (size_t)km * n + i);
                    hp_mac2(sum[c][0][0], v0.x, dw.x, sum[c][0][1], v0.y, dw.y);
                    hp_mac2(sum[c][1][0], v1.x, dw.x, sum[c][1][1], v1.y, dw.y);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < GT; c++) {
            if (g0 + c < G) {
#pragma unroll
                for (int h = 0; h < 2; h++)
                    acc_store_plain(sum[c][h][0], sum[c][h][1], q, mqinv, two_q, r64, r64h, add_prev,
                                    tab.dst[g0 + c] + (size_t)b * dst_pstride + ((size_t)h * E + m) * n + i);
            }
        }
    }
}

hipError_t hp_launch_hks_bsgs_presum(const HpLimb *limbs, u32 L, u32 E, u32 KE, u32 n, u32 P, u32 giants, u32 babies, const u64 *baby,
                                     size_t baby_pstride, const HpPreTable &tab, size_t dst_pstride, bool add_prev, hipStream_t stream) {
    if (P == 0 || giants == 0 || babies == 0) return hipSuccess;
    if (giants > HP_BSGS_GIANT_MAX || giants * babies > HP_BSGS_DIAG_MAX || KE < E || L > E) return hipErrorInvalidValue;
    const u32 tiles = (giants + HKS_PRE_GT - 1) / HKS_PRE_GT;
    return elem_launch_cw(k_hks_bsgs_presum<HKS_PRE_GT>, HKS_LT_CHUNK, P * E * tiles, n, stream, limbs, L, E, KE, giants, babies, n, ElemChunks{},
                          baby, baby_pstride, tab, dst_pstride, add_prev ? 1u : 0u);
}

// Key generation (hp_dev_hks_keygen, hp_dev_hks_keygen_rot): one streaming multiply-add per word of a key.  Row = (r * nd + d) * E + m;
// the workgroup reads its chunk of NTT(e[r][d]) -- which the transform left in key[r][d][0][m], where the result goes -- of a[r][d][m]
// (its own rows, or the words already in key[r][d][1][m]), of s_to[m] and, on the limbs of digit d only, of the source secret, and
// writes both key rows:
//   key[r][d][0][m] = (NTT(e) - a * s_to + (m in digit d) * (P mod q_m) * from_r[m]) * 2^64 mod q_m,   key[r][d][1][m] = a * 2^64 mod q_m
// as CANONICAL residues, whatever representatives come in.  The transformed error word is any u64 (hehub's fold leaves up to 16 q at a
// modulus far below its power of two): Barrett, below 2q for every 64-bit word.  a, s_to and from_r are below 2q: hp_mul_hybrid_lazy
// (a product below 4q^2, q < 2^60) and the Harvey products by P mod q_m and by 2^64 mod q_m (the limb's own pair r64 / r64h) are below
// 2q for any 64-bit operand, the lazy sums stay there, and one conditional subtraction ends each row.
// A thread reads every word of key[..][0] and key[..][1] before it writes it: no scratch copy of the error rows, a may be in place.
// Traffic: e, a and the two key rows are streamed (non-temporal, 16 bytes per lane); s_to[m] is shared by the R * nd rows of its
// modulus and is left to the caches.  ROT: from_r = move_r(s_to), read as k_hks_inner_hoisted reads its digit rows (MovedPair,
// hp_elem.h) -- the row is s_to[m] again, so the scattered reads hit what the whole launch keeps in cache; otherwise s_from[r][m],
// read once per call: streamed.
template <bool ROT>
__global__ void __launch_bounds__(ELEM_THREADS) k_hks_keygen(const HpLimb *__restrict__ limbs, const HpHksConsts *__restrict__ hc, u32 n,
                                                           u32 chunks, const u64 *__restrict__ s_to, const u64 *__restrict__ s_from,
                                                           HpKeygenMaps maps, const u64 *a, u64 *keys) {   // a may be NULL: in place
    const u32 L = hc->L, E = hc->E, nd = hc->nd, alpha = hc->alpha;
    const ElemTile tile(n, chunks);   // row = (r * nd + d) * E + m
    const u32 m = tile.row % E, rd = tile.row / E, d = rd % nd, r = rd / nd;
    const HpLimb lm = limbs[m];
    const bool own = m < L && m / alpha == d;   // the message term: the limbs of digit d
    const u64 pm = own ? hc->p_mod_q[m] : 0, pmh = own ? hc->p_mod_q_h[m] : 0;
    u64 *k0 = keys + ((size_t)rd * 2 * E + m) * n, *k1 = k0 + (size_t)E * n;
    const u64 *ar = a ? a + (size_t)tile.row * n : k1;
    const u64 *st = s_to + (size_t)m * n;
    const u64 *sf = ROT ? st : s_from + ((size_t)r * E + m) * n;
    const u32 *__restrict__ map = ROT ? maps.map[r] : nullptr;   // ROT, NULL: the involution
    const auto from = [&](u32 i) {
        if (!own) return U2{0, 0};
        if (!ROT) return ld_nt(sf + i);
        // MovedPair's loads, written out: through the helper the kernel takes 104 VGPRs for 98, a wave per SIMD
        if (map) {
            const uint2 j = *reinterpret_cast<const uint2 *>(map + i);
            return U2{sf[j.x], sf[j.y]};
        }
        const U2 v = *reinterpret_cast<const U2 *>(sf + (n - 2 - i));
        return U2{v.y, v.x};
    };
    const auto word = [&](u64 e, u64 av, u64 sv, u64 fv, u64 &o0, u64 &o1) {
        u64 b = hp_sub_lazy(hp_barrett_lazy(e, lm.q, lm.barrett_c), hp_mul_hybrid_lazy(av, sv, lm), lm.two_q);
        if (own) b = hp_add_lazy(b, hp_harvey_lazy(fv, pm, pmh, lm.q), lm.two_q);
        o0 = hp_strict(hp_harvey_lazy(b, lm.r64, lm.r64h, lm.q), lm.q);
        o1 = hp_strict(hp_harvey_lazy(av, lm.r64, lm.r64h, lm.q), lm.q);
    };
    const auto pairs = tile.pairs();
    if (tile.full()) {   // all loads of a thread first, then the arithmetic and the stores (hp_elem.h)
        const size_t o = elem_full2(tile, 0);
        U2 ve[ELEM_IT2], va[ELEM_IT2], vs[ELEM_IT2], vf[ELEM_IT2];
#pragma unroll
        for (int t = 0; t < ELEM_IT2; ++t) {
            ve[t] = ld_nt(k0 + o + t * ELEM_STEP2);
            va[t] = ld_nt(ar + o + t * ELEM_STEP2);
            vs[t] = *reinterpret_cast<const U2 *>(st + o + t * ELEM_STEP2);
            vf[t] = from((u32)(o + t * ELEM_STEP2));
        }
#pragma unroll
        for (int t = 0; t < ELEM_IT2; ++t) {
            U2 o0, o1;
            word(ve[t].x, va[t].x, vs[t].x, vf[t].x, o0.x, o1.x);
            word(ve[t].y, va[t].y, vs[t].y, vf[t].y, o0.y, o1.y);
            st_nt(k0 + o + t * ELEM_STEP2, o0);
            st_nt(k1 + o + t * ELEM_STEP2, o1);
        }
        return;
    }
    for (const u32 i : pairs) {   // a row shorter than a chunk (n is even: always whole pairs)
        const U2 e = ld_nt(k0 + i), av = ld_nt(ar + i), sv = *reinterpret_cast<const U2 *>(st + i), fv = from(i);
        U2 o0, o1;
        word(e.x, av.x, sv.x, fv.x, o0.x, o1.x);
        word(e.y, av.y, sv.y, fv.y, o0.y, o1.y);
        st_nt(k0 + i, o0);
        st_nt(k1 + i, o1);
    }
}

hipError_t hp_launch_hks_keygen(const HpLimb *limbs, const HpHksConsts *hc, u32 E, u32 nd, u32 n, u32 R, const u64 *s_to, const u64 *s_from,
                                const HpKeygenMaps *maps, const u64 *a, u64 *keys, hipStream_t stream) {
    if (R == 0) return hipSuccess;
    if (maps && R > HP_HOIST_TABLE_MAX) return hipErrorInvalidValue;
    if (maps) return elem_launch(k_hks_keygen<true>, R * nd * E, n, stream, limbs, hc, n, ElemChunks{}, s_to, s_from, *maps, a, keys);
    return elem_launch(k_hks_keygen<false>, R * nd * E, n, stream, limbs, hc, n, ElemChunks{}, s_to, s_from, HpKeygenMaps{}, a, keys);
}

// ModDown conversion: Garner digits of the special-prime part once per coefficient, then its exact centred value
// (x below floor(P/2), x - P from there on; an exact multiple of q_i above the half comes out as q_i, a representative
// of 0) in every ciphertext modulus.
// PLAIN: with a plain modulus t (BGV; hehub_amd.h has the convention) the remainder is delta = t * c, c the centred value of
// u = [x]_P * t^-1 mod P -- delta = x mod P, delta = 0 mod t, |delta| <= t (P + 1) / 2 -- so that (x - delta) / P keeps x's value mod t.
// Two multiplications more: every special-prime residue by t^-1 mod p_a (strict) before the Garner digits, the centred residue by
// t mod q_m (Harvey, strict: the representative q_m of 0 becomes 0) before the store.  Words below q_m either way: what down() and
// the fused drops take.  The t-dependent constants are pc, a by-value kernel argument -- HpHksConsts belongs to the chain alone.
template <int K, bool PLAIN>
HP_DEV void hks_moddown_body(const HpLimb *__restrict__ limbs, const HpHksConsts *__restrict__ hc, const HpHksPlain *pc, u32 n, u32 chunks,
                             const u64 *__restrict__ yp, u64 *__restrict__ rem) {
    const u32 L = hc->L;
    const ElemTile tile(n, chunks);   // row = p2
    const u32 p2 = tile.row;
    const u64 *src = yp + (size_t)p2 * K * n;
    u64 *dst = rem + (size_t)p2 * L * n;
    for (const u32 i : tile.words()) {
        // PLAIN, K >= 4: the Garner tables are read anew for every word (scalar loads, the constant cache) rather than hoisted out of this
        // loop and spilled -- with pc's words on top of the rest that costs a wave per SIMD at K = 4 and scratch from K = 6 on
        if constexpr (PLAIN && K >= 4) asm volatile("" : "+s"(hc));
        u64 v[K][1];
#pragma unroll
        for (int a = 0; a < K; a++) {
            const u64 pa = limbs[L + a].q;
            v[a][0] = src[(size_t)a * n + i];
            if constexpr (PLAIN) v[a][0] = hp_strict(hp_harvey_lazy(v[a][0], pc->tinv_p[a], pc->tinv_p_h[a], pa), pa);
            garner_digit<K>(v[a], v, a, pa, limbs[L + a].barrett_c, hc->pg_inv, hc->pg_inv_h);
        }
        const bool below = garner_below<K>(v, 0, K, hc->p_half);
        for (u32 m = 0; m < L; m++) {
            const u64 qm = limbs[m].q;
            u64 r = 0;
#pragma unroll
            for (int a = 0; a < K; a++) {
                r += hp_strict(hp_harvey_lazy(v[a][0], hc->p_pref[m][a], hc->p_pref_h[m][a], qm), qm);
                r -= (r >= qm) ? qm : 0;
            }
            if (!below) {
                u64 abs = hc->p_mod_q[m] + qm - r;
                abs -= (abs >= qm) ? qm : 0;
                r = qm - abs;
            }
            if constexpr (PLAIN) r = hp_strict(hp_harvey_lazy(r, pc->t_mod_q[m], pc->t_mod_q_h[m], qm), qm);
            dst[(size_t)m * n + i] = r;
        }
    }
}
template <int K>
__global__ void __launch_bounds__(ELEM_THREADS) k_hks_moddown(const HpLimb *__restrict__ limbs, const HpHksConsts *__restrict__ hc,
                                                            u32 n, u32 chunks, const u64 *__restrict__ yp, u64 *__restrict__ rem) {
    hks_moddown_body<K, false>(limbs, hc, nullptr, n, chunks, yp, rem);
}

hipError_t hp_launch_hks_moddown(const HpLimb *limbs, const HpHksConsts *hc, u32 k, u32 n, u32 P2, const u64 *yp, u64 *rem,
                                 hipStream_t stream) {
    return elem_with_1to8(k, [&](auto kk) {
        return elem_launch(k_hks_moddown<decltype(kk)::value>, P2, n, stream, limbs, hc, n, ElemChunks{}, yp, rem);
    });
}

// ModDown with a plain modulus t: the PLAIN body.  Register budget (tests/test_hks_bgv_resources.py): no scratch, and the occupancy
// of k_hks_moddown<K>.
template <int K>
__global__ void __launch_bounds__(ELEM_THREADS) k_hks_moddown_t(const HpLimb *__restrict__ limbs, const HpHksConsts *__restrict__ hc,
                                                              HpHksPlain pc, u32 n, u32 chunks, const u64 *__restrict__ yp,
                                                              u64 *__restrict__ rem) {
    hks_moddown_body<K, true>(limbs, hc, &pc, n, chunks, yp, rem);
}

hipError_t hp_launch_hks_moddown_t(const HpLimb *limbs, const HpHksConsts *hc, const HpHksPlain &pc, u32 k, u32 n, u32 P2, const u64 *yp,
                                   u64 *rem, hipStream_t stream) {
    return elem_with_1to8(k, [&](auto kk) {
        return elem_launch(k_hks_moddown_t<decltype(kk)::value>, P2, n, stream, limbs, hc, pc, n, ElemChunks{}, yp, rem);
    });
}

// merged ModDown + rescale: the remainder of the division by q_{L-1} joins the ModDown remainder before the transform.
// In the coefficient domain, limb i < L-1:  rem_i <- rem_i + (P mod q_i) * centre_{q_i}(c), c the strict coefficient of the
// relinearised limb L-1 modulo q_last (centred like rescaling.cpp:54-69: c >= q_last/2 means c - q_last)
__global__ void __launch_bounds__(ELEM_THREADS) k_hks_combine(const HpLimb *__restrict__ limbs, const HpHksConsts *__restrict__ hc,
                                                            u32 n, u32 chunks, const u64 *__restrict__ clast,
                                                            u64 *__restrict__ rem) {
    const u32 L = hc->L, Lm1 = L - 1;
    const ElemTile tile(n, chunks);   // row = p2*(L-1) + i
    const u32 p2 = tile.row / Lm1, k = tile.row % Lm1;
    const u64 q = limbs[k].q, bc = limbs[k].barrett_c, two_q = limbs[k].two_q;
    const u64 q_last = limbs[Lm1].q, half = q_last / 2;
    const u64 bump = q - hp_strict(hp_barrett_lazy(q_last, q, bc), q);   // q_i - (q_last mod q_i)
    const u64 pm = hc->p_mod_q[k], pmh = hc->p_mod_q_h[k];
    const u64 *c = clast + (size_t)p2 * n;
    u64 *r = rem + ((size_t)p2 * L + k) * n;
    for (const u32 i : tile.words()) {
        const u64 cv = c[i];
        u64 v = hp_strict(hp_barrett_lazy(cv, q, bc), q);
        if (cv >= half) v += bump;                         // < 2 q_i
        v = hp_harvey_lazy(v, pm, pmh, q);                 // * (P mod q_i), lazy
        r[i] = hp_add_lazy(r[i], v, two_q);
    }
}

hipError_t hp_launch_hks_combine(const HpLimb *limbs, const HpHksConsts *hc, u32 L, u32 n, u32 P2, const u64 *clast, u64 *rem,
                                 hipStream_t stream) {
    if (L < 2) return hipSuccess;
    return elem_launch(k_hks_combine, P2 * (L - 1), n, stream, limbs, hc, n, ElemChunks{}, clast, rem);
}

// ModDown epilogue: out[p2][i] = ((x[p2][i] - rem[p2][i]) * P^-1 mod q_i) [+ addend]; x rows have E limbs, rem / out rows L
// (rem: the lazy transform of the remainders, brought below 2q first -- hp_lazy_below_2q, hp_device.h: exact at every modulus)
__global__ void __launch_bounds__(ELEM_THREADS) k_hks_down_fin(const HpLimb *__restrict__ limbs, const HpHksConsts *__restrict__ hc,
                                                             u32 n, u32 chunks, const u64 *__restrict__ x,
                                                             const u64 *__restrict__ rem, const u64 *__restrict__ addend,
                                                             u32 add_poly_stride, u32 add_ct_stride, u32 add_mask,
                                                             u64 *__restrict__ out) {
    const u32 L = hc->L, E = hc->E;
    const ElemTile tile(n, chunks);   // row = p2*L + i
    const u32 p2 = tile.row / L, k = tile.row % L;
    const u64 q = limbs[k].q, two_q = limbs[k].two_q;
    const u64 *xs = x + ((size_t)p2 * E + k) * n;
    const u64 *rs = rem + (size_t)tile.row * n;
    const u64 *as = drop_addend_row(addend, add_poly_stride, add_ct_stride, add_mask, p2, k, n);
    u64 *os = out + (size_t)tile.row * n;
    for (const u32 i : tile.words()) {
        u64 v = hp_sub_lazy(xs[i], hp_lazy_below_2q(rs[i], two_q), two_q);   // (rs: a lazy transform word, not always below 2q)
        v = hp_harvey_lazy(v, hc->pinv[k], hc->pinv_h[k], q);
        if (as) v = hp_add_lazy(v, as[i], two_q);
        os[i] = v;
    }
}

hipError_t hp_launch_hks_down_fin(const HpLimb *limbs, const HpHksConsts *hc, u32 L, u32 n, u32 P2, const u64 *x, const u64 *rem,
                                  const u64 *addend, u32 add_poly_stride, u32 add_ct_stride, u32 add_mask, u64 *out,
                                  hipStream_t stream) {
    return elem_launch(k_hks_down_fin, P2 * L, n, stream, limbs, hc, n, ElemChunks{}, x, rem, addend, add_poly_stride, add_ct_stride,
                       add_mask, out);
}
