// hp_hks_call.h -- the hybrid key switch as the host units see it: the call object every hybrid entry point is written against
// (bodies in hp_api_hks.cpp) and the pieces of the multiplication tails that more than one unit runs (hp_api_hks_mult.cpp).
#pragma once
#include "hp_ctx.h"

#include <cstring>
#include <optional>

namespace hpi {

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
            uint64_t plain_modulus);
    HksCall(const HksCall &) = delete;   // (one LevelScope per call)
    int limits(size_t batch) const;
    int open();
    // What a BGV entry point refuses on top of its CKKS sibling, after the shared limits: t must be invertible modulo every modulus
    // of the chain (they are primes: 0 < t < each of them is enough), and ModDown_t exists as the one-kernel conversion only.
    int plain_ok();
    void plain_consts();

    // The digit stage of P polynomials pt (NTT form, L limbs, row stride pt_pstride): lifted [P][nd][E][N] = every digit's exact
    // integer, in NTT form, in every modulus outside the digit (the slots inside a digit stay unwritten: there D_d is the input limb
    // itself).  All that depends on the input alone -- a rotation that is applied to these rows afterwards
    // (hp_dev_ckks_rotate_hoisted_hks) shares them with every other rotation.
    size_t digits_words(size_t P) const { return padded(P * L * n) / 8 + padded(P * nd * E * n) / 8; }
    int digits(size_t P, const u64 *pt, size_t pt_pstride, u64 **lifted_out, Carver &cv) const;

    size_t tail_words(size_t P) const { return padded(P * 2 * E * n) / 8 + padded(2 * P * k * n) / 8 + padded(2 * P * L * n) / 8; }
    HksTail tail(size_t P, Carver &cv) const { return {cv.take(P * 2 * E * n), cv.take(2 * P * k * n), cv.take(2 * P * L * n)}; }

    // a plain switch up to its inner product: t.ks [P][2][E][N] = sum_d D_d * key_d over the digit rows of pt
    int front(size_t P, const u64 *pt, size_t pt_pstride, const u64 *key, HksTail &t, Carver &cv) const;

    // The first half of ModDown: t.rem = the centred exact conversion of the P-part of t.ks into every q_i (coefficient form) --
    // coefficients of the P-part (strict), then the conversion; the transform, the subtraction and * P^-1 are down()'s
    int pdown(size_t P, const HksTail &t) const;

    // ModDown of the limbs [i0, i0 + cnt) with the transform of the remainders fused in: out = (ks - NTT(rem)) * P^-1 [+ addend]
    // (level A: the canonical residues of that)
    int down_fused(size_t i0, size_t cnt, size_t P2, const u64 *rem, HpDropArgs &da, bool level_a, const char *what, const char *what_a) const;

    // the end of a switch: out [P][2][L][N] = (ks - NTT(rem)) * P^-1 [+ addend rows (p2>>1)*add.ct_stride + (p2&1)*add.poly_stride + i]
    int down(size_t P, const u64 *ks, u64 *rem, const Addend &add, u64 *out) const;

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
int rotations_ok(hp_ctx *ctx, const char *call, const HksRotations &rot, const uint64_t *const *diags, bool identity_ok);

// the calls that write their output while they still read their input
int no_overlap(hp_ctx *ctx, const char *call, const void *in, size_t in_bytes, const void *out, size_t out_bytes);

// ---- the multiplication tails (hp_api_hks_mult.cpp) ----
// quad [batch][3][L][N] = the tensor product of ct1, ct2 [batch][2][L][N] (ckks:: / bgv::mult_low_level's words)
int tensor_quad(const HksCall &c, size_t batch, const u64 *ct1, const u64 *ct2, u64 *quad);

// What follows the tensor product of a hybrid multiplication, on an open call: hybrid relinearisation of d2, + (d0, d1), rescale by the
// last ciphertext modulus.  quad [batch][3][L][N], words below 2q: the workspace block of hp_dev_ckks_mult_relin_rescale_hks and
// hp_dev_ckks_dot_relin_rescale_hks, the caller's memory in hp_dev_ckks_relin_rescale_hks -> out [batch][2][L-1][N].  Everything here
// is linear in quad, which is why a sum of products pays it once.
size_t relin_rescale_words(const HksCall &c, size_t batch);
int relin_rescale(const HksCall &c, size_t batch, const u64 *quad, const u64 *key, u64 *out, Carver &cv);
// quad [batch][3][L][N], words below 2q -> out [batch][2][L-1][N] on an open BGV call; the workspace is relin_rescale_words'
int bgv_relin_modswitch(const HksCall &c, size_t batch, const u64 *quad, const u64 *key, u64 *out, Carver &cv);

// ---- sums of products: lazy relinearisation ----
// rescale(relin(sum_t a_t (x) b_t)) = rescale(sum_t (d0_t, d1_t) + switch(sum_t d2_t)), residue for residue: T products pay one switch
// and one rounding.  The quadratic sum is one streaming kernel (k_tensor_sum, hp_ks.hip), one launch per argument table.
struct TensorSumTerms {
    size_t terms;
    const uint64_t *const *a, *const *b;   // HOST arrays of device addresses, each u64[batch][2][L][N]
};
// before anything is enqueued: the list itself, and `out` (the call's output, out_bytes long) against every operand
int tensor_sum_ok(hp_ctx *ctx, const char *call, size_t n, size_t L, size_t batch, const TensorSumTerms &ts, const void *out, size_t out_bytes);
// quad [batch][3][L][N] = the sum over the list, `pass` terms per launch (tensor_sum_max_terms' answer)
int tensor_sum(hp_ctx *ctx, const HpLimb *limbs, size_t n, size_t L, size_t batch, size_t pass, const TensorSumTerms &ts, u64 *quad);

} // namespace hpi
