// hp_lincomb.hip -- linear combinations of ciphertexts with per-limb integer coefficients (hp_dev_ckks_lincomb, and every linear
// form of hp_dev_ckks_eval_plan_hks): one HBM-streaming kernel over the tile skeleton of hp_elem.h.
//
//   out[b][h][m][i] = ( [accumulate] out + sum_{j < terms} coef_j[m] * E_j[b][h][m][i] + (h == 0) cst[m] )  mod q_m
//
// Every term is a ciphertext batch of its OWN limb count (tab.limbs[j] >= L rows per polynomial) read in its first L limb rows: the
// mod-drop of a polynomial evaluation costs no copy.  A thread owns pairs of adjacent words of a row (b, h, m) and keeps one
// carry-save accumulator per word for every term: per term one 16-byte non-temporal load per pair (the loads of a round are issued
// together, then its hp_mac2) and after the last term ONE Montgomery reduction per output word: the coefficients are plain residues,
// so the tail is that of a sum of plain products (acc2_plain, hp_elem.h, has the argument) with the constant and the accumulated
// word added BEFORE the reduction and one conditional subtraction after it, which makes the word canonical.  HBM traffic per output
// word: 8 (terms + 1) bytes (+ 8 with accumulate), against 16 + 24 = 40 bytes per term for a scalar multiplication and an addition.
// Range: operand words below 2q, coefficients and the constant below q, an accumulated word below 2q: a launch of T terms sums at
// most T (q - 1)(2q - 1) + 3q, which the host keeps within the tail's limit (hpi::lincomb_max_terms, hp_drop.h).  A longer list takes
// one launch per table, the later ones with accumulate.
// The coefficients of a launch live in device memory, u64[terms + 1][L] (row `terms`: the constant): wave-uniform scalar loads.
#include "hp_elem.h"

// R rounds of a lane (R == ELEM_IT2: a full ELEM_CHUNK, round t at + t * ELEM_STEP2; 1: one step of the pairs loop).  TWO: the lane's
// words i, i + 1 (16-byte accesses); else the single last word of an odd row
template <int R, bool TWO>
HP_DEV void lincomb_words(const HpLimb &m, const HpLincombTable &tab, const u64 *__restrict__ coef, u32 L, u32 k, u32 n, size_t p2,
                          size_t at, u64 cst, u32 accumulate, u64 *dst) {
    HpAcc s[R][2];
    acc_zero(s);
    for (u32 j = 0; j < tab.terms; j++) {
        const u64 c = coef[(size_t)j * L + k];
        const u64 *x = tab.src[j] + (p2 * tab.limbs[j] + k) * n + at;
        U2 v[R];
#pragma unroll
        for (int t = 0; t < R; t++) v[t] = TWO ? ld_nt(x + t * ELEM_STEP2) : U2{x[0], 0};
#pragma unroll
        for (int t = 0; t < R; t++) hp_mac2(s[t][0], v[t].x, c, s[t][1], v[t].y, c);
    }
    U2 old[R];
#pragma unroll
    for (int t = 0; t < R; t++) {
        old[t] = U2{0, 0};
        if (accumulate) old[t] = TWO ? *reinterpret_cast<const U2 *>(dst + t * ELEM_STEP2) : U2{dst[0], 0};
    }
#pragma unroll
    for (int t = 0; t < R; t++) {
        hp_mac2(s[t][0], old[t].x + cst, 1, s[t][1], old[t].y + cst, 1);   // (below 2q + q: a word)
        U2 v = acc2_montgomery(s[t][0], s[t][1], m.q, m.mqinv);           // the sum * 2^-64 ...
        v.x = hp_strict(hp_harvey_lazy(v.x, m.r64, m.r64h, m.q), m.q);    // ... * 2^64, below 2q, then canonical
        v.y = hp_strict(hp_harvey_lazy(v.y, m.r64, m.r64h, m.q), m.q);
        if (TWO) st_nt(dst + t * ELEM_STEP2, v);
        else dst[0] = v.x;
    }
}

__global__ void __launch_bounds__(ELEM_THREADS) k_ct_lincomb(const HpLimb *__restrict__ limbs, u32 L, u32 n, u32 chunks, u32 cw,
                                                            HpLincombTable tab, const u64 *__restrict__ coef, u32 accumulate,
                                                            u32 out_polys, u64 *out) {
    const ElemTile tile(n, chunks, cw);   // row = (p * 2 + h) * L + k; cw = words per workgroup
    const u32 p2 = tile.row / L, k = tile.row % L, p = p2 >> 1, h = p2 & 1;
    const HpLimb m = limbs[k];
    const u64 cst = h ? 0 : coef[(size_t)tab.terms * L + k];
    u64 *dst = out + (((size_t)p * out_polys + h) * L + k) * n;
    if (cw == ELEM_CHUNK && tile.full()) {
        const size_t at = elem_full2(tile, 0);
        lincomb_words<ELEM_IT2, true>(m, tab, coef, L, k, n, p2, at, cst, accumulate, dst + at);
        return;
    }
    for (const u32 i : tile.pairs()) {
        if (tile.pair(i)) lincomb_words<1, true>(m, tab, coef, L, k, n, p2, i, cst, accumulate, dst + i);
        else lincomb_words<1, false>(m, tab, coef, L, k, n, p2, i, cst, accumulate, dst + i);
    }
}

// out: [P][out_polys][L][n], polynomials 0 and 1 written (out_polys = 2: a ciphertext batch; 3: the (d0, d1) of a quad)
hipError_t hp_launch_ct_lincomb(const HpLimb *limbs, u32 L, u32 n, u32 P, const HpLincombTable &tab, const u64 *d_coef, bool accumulate,
                                u64 *out, u32 out_polys, hipStream_t stream) {
    if (P == 0 || L == 0) return hipSuccess;
    if (tab.terms > HP_LINCOMB_MAX || out_polys < 2 || out_polys > 3) return hipErrorInvalidValue;
    for (u32 j = 0; j < tab.terms; j++)
        if (tab.limbs[j] < L) return hipErrorInvalidValue;   // (a row past the operand's last limb)
    // a launch of few rows: 512 words per workgroup (one dependent step per thread), as k_tensor_sum
    const u32 rows = 2 * P * L;
    const u32 cw = ((size_t)rows * ((n + ELEM_CHUNK - 1) / ELEM_CHUNK) < 1024 && n >= ELEM_THREADS * 2) ? ELEM_THREADS * 2 : ELEM_CHUNK;
    if ((u64)rows * ((n + cw - 1) / cw) >= (1ull << 31)) return hipErrorInvalidValue;   // (workgroups of one launch)
    return elem_launch_cw(k_ct_lincomb, cw, rows, n, stream, limbs, L, n, ElemChunks{}, cw, tab, d_coef, accumulate ? 1u : 0u, out_polys,
                          out);
}
