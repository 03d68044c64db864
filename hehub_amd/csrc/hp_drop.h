// hp_drop.h -- the fused drop launches (rescaling.cpp:46-75 / mod_switch.cpp:45-77, relinearize's mod-down, hybrid ModDown) as the
// host describes them to the kernels: the argument structs, and the pure builders (hp_drop.cpp) of every constant in them.
// No HIP here: the builders take a chain of hp::ModConsts or plain moduli and are checked word for word on the CPU
// (tests/test_host_drop_consts.py).  hp_kernels.h includes this header; the kernels read the structs as they are laid out here.
//
// What the fields of HpDropArgs hold, per flavour of the launch (k = limb of the launch, counted from its first limb):
//
//   level B, one drop (hp_ntt_fast.hip, hp_ntt_split.hip; drop_consts / hks_down_consts / hks_down_rescale_consts)
//     every word is an integer below its modulus, (v, v_h) = v with its Harvey word floor(v 2^64 / q_k)
//     dc.q_last, dc.half_q_last   the modulus dropped and floor(q_last / 2)
//     dc.r[k]                     q_last mod q_k
//     dc.inv[k]                   q_last^-1 mod q_k            (hybrid ModDown: P^-1 mod q_k)
//     dc.t[k], dc.qlt[k]          BGV: t mod q_k, (q_last mod t) mod q_k; zero for CKKS
//     small_rem                   1: q_last <= 2 q_k for every limb of the launch and the coefficient rows are strict -- the remainder
//                                 of c < q_last is c - [c >= q_k] q_k (the canonical residue either way; saves the Barrett quotient)
//     raw_input                   1: the transform's input rows already are the per-limb remainders (hybrid): no Barrett / centring
//     fin_on, fin[k]              1: one more multiplication AFTER the addend, by fin[k] (hybrid merged rescale: q_last^-1 mod q_k)
//     comb, comb_half             non-NULL (with raw_input): input = src + comb_mul[k] * centre_k(comb[p2]), comb [P2][N] strict
//                                 modulo 2 comb_half + 1
//     comb_mul[k], comb_r[k]      hybrid merged rescale: P mod q_k, q_last mod q_k
//
//   level A, one drop (hp_ntt_a.hip; drop_consts_to_a / hks_down_consts_a)
//     every constant is the bit pattern of a double; a multiplier v travels as the pair (v, RN(v / q_k))           (a_pair)
//     dc.q_last, dc.half_q_last   the doubles q_last, floor(q_last / 2); raw rows (hybrid): 0 and 2^62, which switches the centring off
//     (dc.inv, dc.inv_h)[k], (dc.t, dc.t_h)[k], (dc.qlt, dc.qlt_h)[k]   the pairs of the level-B values
//     r, small_rem, raw_input, fin, comb_r, comb_half are not read; output rows are canonical residues
//
//   level A, two drops in one transform (hp_ntt_a.hip: DropPre2A has the algebra; two_drop_consts / hks_down_rescale_consts_a)
//     z_k = ((A_k x_k + a_k) - NTT_k(m_k c1 + m2_k c2)) B_k with c1 = the transform's input rows, c2 = comb
//     (dc.inv, dc.inv_h)[k] = A_k, (dc.t, dc.t_h)[k] = m_k, (comb_mul, comb_mul_h)[k] = m2_k, (dc.qlt, dc.qlt_h)[k] = B_k, as pairs
//     dc.q_last, dc.half_q_last   the first modulus dropped (centres c1);  q2_last, half_q2_last   the second (centres c2)
//
//   every flavour (drop_args)
//     x, L                        [P2][L][n]: polynomial p2 at x + p2*L*n, limb k at + k*n; L limbs per polynomial of x
//     addend, add_*_stride, add_mask   an Addend (below); out, out_stride   [P2][out_stride][n]
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

typedef uint64_t u64;
typedef uint32_t u32;

#define HP_MAX_LIMBS 32

struct HpDropConsts {
    u64 q_last, half_q_last;
    u64 r[HP_MAX_LIMBS];
    u64 inv[HP_MAX_LIMBS];
    u64 inv_h[HP_MAX_LIMBS];
    int bgv;
    u64 t[HP_MAX_LIMBS], t_h[HP_MAX_LIMBS];
    u64 qlt[HP_MAX_LIMBS], qlt_h[HP_MAX_LIMBS];
};
struct HpDropArgs {
    HpDropConsts dc;
    int small_rem;
    int raw_input;
    u32 out_stride;
    int fin_on;
    u64 fin[HP_MAX_LIMBS], fin_h[HP_MAX_LIMBS];
    const u64 *comb;
    u64 comb_half, comb_r[HP_MAX_LIMBS], comb_mul[HP_MAX_LIMBS], comb_mul_h[HP_MAX_LIMBS];
    u64 q2_last, half_q2_last;
    const u64 *x;
    u32 L;
    const u64 *addend;
    u32 add_poly_stride, add_ct_stride;
    u32 add_mask;
    u64 *out;
};
// level A, inverse of ONE limb (job.L == 1) whose input is A * src + add and whose output has K * centre(cprev) subtracted
// (hp_ntt_a.hip: ntt_inv_a_body MIX); every constant as the bit pattern of a double, (v, RN(v / q)) for the multipliers
struct HpInvMixArgs {
    const u64 *add;            // addend rows already at the limb: polynomial p at (p >> 1) * add_ct_stride + (p & 1) * add_poly_stride limbs
    u32 add_poly_stride, add_ct_stride;
    u64 A, A_h;
    const u64 *cprev;          // [P][N] strict coefficients modulo prev_q
    u64 prev_q, prev_half;
    u64 K, K_h;
};

// the kernels take these structs by value: a field that moves here moves under them
static_assert(sizeof(HpDropConsts) == 1816 && sizeof(HpDropArgs) == 3192 && sizeof(HpInvMixArgs) == 72, "kernel argument struct resized");
static_assert(offsetof(HpDropConsts, r) == 16 && offsetof(HpDropConsts, inv) == 272 && offsetof(HpDropConsts, inv_h) == 528, "HpDropConsts moved");
static_assert(offsetof(HpDropConsts, bgv) == 784 && offsetof(HpDropConsts, t) == 792 && offsetof(HpDropConsts, qlt_h) == 1560, "HpDropConsts moved");
static_assert(offsetof(HpDropArgs, small_rem) == 1816 && offsetof(HpDropArgs, out_stride) == 1824 && offsetof(HpDropArgs, fin) == 1832, "HpDropArgs moved");
static_assert(offsetof(HpDropArgs, comb) == 2344 && offsetof(HpDropArgs, comb_r) == 2360 && offsetof(HpDropArgs, comb_mul_h) == 2872, "HpDropArgs moved");
static_assert(offsetof(HpDropArgs, q2_last) == 3128 && offsetof(HpDropArgs, x) == 3144 && offsetof(HpDropArgs, L) == 3152, "HpDropArgs moved");
static_assert(offsetof(HpDropArgs, addend) == 3160 && offsetof(HpDropArgs, add_mask) == 3176 && offsetof(HpDropArgs, out) == 3184, "HpDropArgs moved");
static_assert(offsetof(HpInvMixArgs, add_poly_stride) == 8 && offsetof(HpInvMixArgs, A) == 16 && offsetof(HpInvMixArgs, cprev) == 32, "HpInvMixArgs moved");
static_assert(offsetof(HpInvMixArgs, prev_q) == 40 && offsetof(HpInvMixArgs, K) == 56 && offsetof(HpInvMixArgs, K_h) == 64, "HpInvMixArgs moved");

// Which compiled flavour of the fused drop kernels a launch takes (the FLAV template argument; hp_ntt_fast.hip and hp_ntt_a.hip
// have the list).  Level B: 0 (every option read at run time) .. 5; *small: the SMALL form of that flavour (small_rem, never with 0).
// Level A: 1 .. 7, negative where level A has no kernel for the launch (fin_on, raw_input, or comb without an addend on both
// polynomials).
int hp_drop_flavour_b(const HpDropArgs &da, bool *small);
int hp_drop_flavour_a(const HpDropArgs &da);

namespace hp {
struct ModConsts;
}

namespace hpi {

// rows added in a drop's epilogue: polynomial p2, limb k takes row (p2 >> 1) * ct_stride + (p2 & 1) * poly_stride + k; bit h of mask:
// polynomial h of each ciphertext gets one (relinearize 3, rotate 1).  Default-constructed: none.
struct Addend {
    const u64 *rows = nullptr;
    u32 poly_stride = 0, ct_stride = 0, mask = 0;
    Addend() = default;
    Addend(const u64 *r, size_t ps, size_t cs, u32 m) : rows(r), poly_stride((u32)ps), ct_stride((u32)cs), mask(r ? m : 0u) {}
    Addend from(size_t words) const { return rows ? Addend(rows + words, poly_stride, ct_stride, mask) : Addend(); }
};

// the level-A form of a multiplier v modulo q: the bit patterns of the doubles (v, RN(v / q))
void a_pair(u64 v, u64 q, u64 &bits, u64 &bits_h);

// everything of a drop launch that is not arithmetic; the rest is zero
HpDropArgs drop_args(const u64 *x, size_t L, const Addend &add, u64 *out, size_t out_stride);

// ---- dropping the last modulus of chain[0 .. L) ------------------------------------------------------------------------
// level B, for the limbs [k0, k1) of the L - 1 that remain, numbered from k0 (a launch's limb 0 is the chain's k0)
void drop_consts(const hp::ModConsts *chain, size_t L, size_t k0, size_t k1, bool bgv, u64 t, HpDropConsts &dc);
// rescaling.cpp:54-58: strict_barrett_{q_k}(c), c < q_last, is one conditional subtraction when q_last <= 2 q_k for every k in [k0, k1)
int drop_small_rem(const hp::ModConsts *chain, size_t L, size_t k0, size_t k1);
// such a block (of the limbs [k0, k1)) to level A
void drop_consts_to_a(const hp::ModConsts *chain, size_t k0, size_t k1, HpDropConsts &dc);
// the scalar t^-1 mod q_last that the inverse transform of the last limb multiplies by (mod_switch.cpp:49-50), at either level
void drop_post_scalar(u64 t, u64 q_last, bool level_a, u64 &s, u64 &s_h);

// ---- level A: dropping chain[L] (p, with plain modulus t1) and then chain[L-1] (q', t2) in one transform -----------------
// fills the arithmetic of da for the limbs k < L - 1 and of mx for the combined limb L - 1, whose strict coefficients modulo q' are
// INTT(A x + a) - K cp (cp = centred coefficients modulo p): A = p^-1 [(p mod t1)], K = A [t1]      (bracketed factors: BGV)
void two_drop_consts(const hp::ModConsts *chain, size_t L, bool bgv, u64 t1, u64 t2, HpDropArgs &da, HpInvMixArgs &mx);

// ---- hybrid key switch: chain q_0..q_{L-1}, special primes p_0..p_{k-1} = mext[L .. L+k), P their product -----------------
struct HksLimbConsts {   // per ciphertext modulus q_i, with Harvey words
    std::vector<u64> pinv, pinv_h;         // P^-1 mod q_i
    std::vector<u64> p_mod_q, p_mod_q_h;   // P mod q_i
};
bool hks_limb_consts(const u64 *mext, size_t L, size_t k, HksLimbConsts &out);   // false: some q_i divides P
// How many rotations one launch of k_hks_inner_lintrans (hp_hks.hip) may sum before its 128-bit accumulators could wrap, at most
// table_max; 0: not even one.  With q the largest modulus of the chain and nd digits, a rotation's word (the Montgomery word of nd
// products of lazy words, plus the folded c0 term) is below w = 4 nd ceil(q^2 / 2^64) + 3q, which must be a 64-bit word, and a
// diagonal word below 2q: the largest R with R w 2q < 2^128.  Exact integers.
size_t hks_lintrans_max_rotations(const u64 *mext, size_t E, size_t nd, size_t table_max);
// How many terms one launch of k_tensor_sum (hp_ks.hip) may sum, at most table_max; 0: not even one.  With q the largest modulus
// of the chain, operand words at most 2q - 1 and the d1 column with two products per term, T terms sum to at most 2 T (2q - 1)^2.
// The Montgomery step returns hi + mulhi(u, q) + 1 in a 64-bit word, so the high word of the sum must stay at most 2^64 - 1 - q:
//   q == 0 or q >= 2^62: 0;  else min(table_max, floor(((2^64 - q) 2^64 - 1) / (2 (2q - 1)^2)))
// -- the whole table of 32 for every modulus the transforms accept (below 2^59.5), 30 at q = 2^60.  Exact integers.
size_t tensor_sum_max_terms(const u64 *moduli, size_t L, size_t table_max);
// How many terms one launch of k_ct_lincomb (hp_lincomb.hip) may sum, at most table_max; 0: not even one.  With q the largest modulus
// of the chain, operand words at most 2q - 1, coefficients at most q - 1, and the constant (below q) plus an accumulated word (below
// 2q) on top, T terms sum to at most T (q - 1)(2q - 1) + 3q, which the same Montgomery step must find at most (2^64 - q) 2^64 - 1:
//   q < 2 or q >= 2^62: 0;  else min(table_max, floor(((2^64 - q) 2^64 - 1 - 3q) / ((q - 1)(2q - 1))))
// -- the whole table of 32 for every modulus below 2^60.9, 28 at q = 2^61 - 1, 6 just below 2^62.  Exact integers.
size_t lincomb_max_terms(const u64 *moduli, size_t L, size_t table_max);
// The pass plan and the workspace of hp_dev_ckks_lintrans_bsgs_hks (hp_api_hks.cpp), a function of the shape alone -- never of the
// steps or of which diagonals are present.  With E = L + k, nd = ceil(L / alpha), pad(w) = w words rounded up to 256 bytes:
//   baby_pass     babies per pre-sum launch (and per baby-stage launch): hks_lintrans_max_rotations(mext, E, nd, HP_BSGS_TABLE_MAX) --
//                 the pre-sum multiplies a baby word (the bound of w_r plus the folded word) by a diagonal word below 2q, the flat
//                 kernel's range argument -- capped by `babies`
//   giant_pass    giants per accumulate launch: min(giants, HP_BSGS_TABLE_MAX) (their words are summed with weight 1)
//   presum_giants giants per pre-sum launch: min(giants, HP_BSGS_GIANT_MAX, HP_BSGS_DIAG_MAX / baby_pass) -- the launch's table holds
//                 HP_BSGS_DIAG_MAX diagonal addresses
//   words         max( pad(B L n) + pad(B nd E n) + pad(B babies 2 E n),            first digit rows + baby rows, dead after the pre-sum
//                      pad(B G L n) + pad(B G nd E n) )                            ... where the giants' digit rows then live
//                 + pad(B 2 E n) + pad(B G 2 E n)                                  acc, pre
//                 + pad(2 B G k n) + pad(2 B G L n) + pad(B G 2 L n)               yp, rem (both ModDown stages), u
//                 (B = batch, G = giants: an identity giant leaves its share unused)
// false: hks_lintrans_max_rotations returns 0 (HP_EUNSUPPORTED), or babies == 0 or giants == 0.
#define HP_BSGS_TABLE_MAX 32    // == HP_HOIST_TABLE_MAX (hp_kernels.h asserts it)
#define HP_BSGS_GIANT_MAX 32
#define HP_BSGS_DIAG_MAX 256
struct HksBsgsPlan {
    size_t baby_pass, giant_pass, presum_giants;
    size_t overlay_words;   // the first term of `words`: where the regions that outlive the pre-sum begin
    size_t words;
};
bool hks_bsgs_plan(const u64 *mext, size_t n, size_t L, size_t k, size_t alpha, size_t batch, size_t babies, size_t giants,
                   HksBsgsPlan &out);
// level A: the transform's input rows ARE the remainders -- centring against a threshold out of reach (2^62) does nothing
void a_raw_rows(HpDropArgs &da);
// ModDown of the limbs [i0, i0 + cnt): out = (x - NTT(rem)) P^-1 [+ addend]; level B, then that block to level A
void hks_down_consts(const HksLimbConsts &hc, size_t i0, size_t cnt, HpDropArgs &da);
void hks_down_consts_a(const u64 *mext, size_t i0, size_t cnt, HpDropArgs &da);
// ModDown merged with the rescale by q_last = q_{L-1}, limbs i < L - 1: ((x - NTT(rem + P centre(comb))) P^-1 + addend) q_last^-1.
// comb == NULL: the combination has been done by its own kernel.  Level B, then that block to the two-drop flavour of level A
// (A = m = P^-1, m2 = 1, B = q_last^-1)
void hks_down_rescale_consts(const HksLimbConsts &hc, const u64 *mext, size_t L, const u64 *comb, HpDropArgs &da);
void hks_down_rescale_consts_a(const u64 *mext, size_t L, HpDropArgs &da);

} // namespace hpi
