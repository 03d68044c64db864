// hp_kernels.h -- host-callable launchers of the HIP kernels (one per kernel family).
// Every launcher enqueues on `stream` and returns the hipError_t of the launch.
#pragma once
#include "hp_device.h"
#include "hp_drop.h"   // HP_MAX_LIMBS, HpDropConsts, HpDropArgs, HpInvMixArgs
#include "hp_sample.h" // HpSampleSeed, the kind tags
#include "hp_bfv.h"    // HpBfvBase, HpBfvConsts, HpBfvPlain, HpBfvDecPlain

// ---- transform jobs -----------------------------------------------------------
// A transform launch processes W independent limb transforms ("work items").
// Items are numbered modulus-major so that neighbouring items share a twiddle
// table; hp_xcd_remap() then gives each XCD a contiguous slice of them.
enum HpNttMode : int {
    HP_NTT_BATCH = 0,   // rows [P][L][N]: item w = k*P + p         -> src/dst row p*L + k, limb k
    HP_NTT_HKS = 2,     // hybrid key switch (extension): in-place transforms of the lifted digits [P][nd][E][N]; one item per
                        //   (modulus m, digit d, polynomial p) with m outside digit d, modulus-major, hole-free
    HP_NTT_SPREAD = 1,  // digit spread (rgsw.cpp:108-119): one item per (k, j != k, p), k in [0,L], numbered modulus-major
                        //   then digit then polynomial without holes, or by groups of moduli (pair_moduli, hp_ntt_job.h): src = coef row p*L + j,
                        //   dst = digit row (p*L + j)*(L+1) + k, limb k; a launch may cover only the moduli
                        //   k_first .. k_first + kc - 1 (W = their item count)
};

struct HpNttJob {
    const HpLimb *limbs;  // plan (device)
    const u64 *src;
    u64 *dst;
    u32 logn;
    u32 L;          // limbs per polynomial
    u32 P;          // polynomials
    u32 src_pstride;  // HP_NTT_BATCH / HP_NTT_LAST: rows (limbs) between consecutive polynomials of src
    u32 dst_pstride;  // HP_NTT_BATCH: same for dst
    u32 src_kstride;  // HP_NTT_BATCH: rows between consecutive limbs of src (1; 0 = every limb reads the same row)
    u32 W;          // work items
    u32 k_first;    // HP_NTT_SPREAD: first output modulus of the launch
    u32 pair_moduli;  // HP_NTT_SPREAD, whole launches only: G > 0 numbers the items by groups of G consecutive moduli so that
                      // the G transforms of one source row run in neighbouring workgroups (the row is re-read from L2)
    u32 hks_nd, hks_E, hks_alpha;   // HP_NTT_HKS: digits, moduli of the extended chain, limbs per digit (L = ciphertext moduli)
    u32 pack_mask;    // HP_NTT_SPREAD, tiled kernels: bit k set = the digit rows of output modulus k are written in the 48-bit
                      // packed row format (hp_device.h: HP_PACK48) that the inner-product kernel reads back; set by the engine only
                      // when every word of those rows is provably below 2^48 (hp_api_scheme.cpp: spread_pack_mask)
    u32 pack40_mask;  // level A only (hp_ntt_a.hip): bit k set = those rows in the 40-bit packed format HP_PACK40 instead (hp_device.h)
    int mode;
    int inverse;
    int strict;     // inverse only: reduce_strict epilogue (ntt.h:88-92)
    // inverse only: multiply by a per-launch scalar (s, s') with the Harvey
    // multiplication BEFORE the strict reduction (mod_switch.cpp:49-50); s_h == 0 and s == 0 -> off
    u64 post_scalar, post_scalar_h;
    int use_post_scalar;
    // parity level A (opt-in, hp_ctx_set_parity_level): non-NULL = the launch goes to the FP64 residue kernels of hp_ntt_a.hip,
    // which return CANONICAL residues (equal to reduce_strict of the level-B words); post_scalar / post_scalar_h then hold the
    // bit patterns of the doubles (s, RN(s / q))
    const HpLimbA *limbs_a;
    u32 src_words;  // level A, HP_NTT_SPREAD: the source rows are WORDS (strict coefficient rows a caller supplied: the limb-range stage
                    // hp_dev_ks_inner_range_strict), not the doubles k_ntt_inv_a writes with dst_f64 for the launch of its own call
    u32 dst_f64;    // level A, inverse: the output rows are the doubles themselves, not words -- only for rows that feed a level-A
                    // HP_NTT_SPREAD launch (k_ntt_fwd_a<., true> reads doubles), never for rows a caller sees
};

hipError_t hp_launch_ntt_generic(const HpNttJob &job, hipStream_t stream);
// fast path: logn in [11,15]; returns hipErrorNotSupported otherwise
hipError_t hp_launch_ntt_fast(const HpNttJob &job, hipStream_t stream);
// a limb split over N / 2048 workgroups and two launches (hp_ntt_split.hip): the latency path for launches with few limbs; logn in
// [12, 16], plain u64 rows, level B; returns hipErrorNotSupported otherwise
hipError_t hp_launch_ntt_split(const HpNttJob &job, hipStream_t stream);
// the same tiling with FP64 residue butterflies (job.limbs_a; HP_NTT_BATCH and HP_NTT_SPREAD; the inverse is always strict)
hipError_t hp_launch_ntt_a(const HpNttJob &job, hipStream_t stream);
// ModRaise (hp_ntt_raise.hip; hp_dev_ckks_mod_raise): the tiled forward transform whose loads centre a strict coefficient row modulo
// q_0 and reduce it into the item's modulus -- v = strict(barrett_q(c)) (+ q - (q_0 mod q) when c >= half), the load side of the
// fused drop without its epilogue.  job: HP_NTT_BATCH, forward, level B, logn in [11, 15], every limb reading its polynomial's one
// row (src_kstride 0, pair_moduli as in the fused drop); limb k of the job is job.limbs[k].  Output words are below 2 * modulus.
struct HpRaiseArgs {
    u64 half;               // floor(q_0 / 2): a coefficient from here on is negative
    u64 r[HP_MAX_LIMBS];    // q_0 mod (modulus of limb k of the job)
};
hipError_t hp_launch_ntt_raise(const HpNttJob &job, const HpRaiseArgs &ra, hipStream_t stream);

// ---- coefficient-wise kernels on [rows][n], limb of a row = row % L ---------------
enum HpBinOp : int { HP_ADD = 0, HP_SUB = 1, HP_MUL = 2 };
hipError_t hp_launch_poly_binary(int op, const HpLimb *limbs, u32 L, u32 n, u32 rows, const u64 *a,
                                 const u64 *b, u64 *out, hipStream_t stream);
struct HpScalars {
    u64 s[HP_MAX_LIMBS];
    u64 sh[HP_MAX_LIMBS];
};
hipError_t hp_launch_poly_scalar_mul(const HpLimb *limbs, const HpScalars &sc, u32 L, u32 n, u32 rows,
                                     const u64 *a, u64 *out, hipStream_t stream);
hipError_t hp_launch_poly_strict(const HpLimb *limbs, u32 L, u32 n, u32 rows, u64 *x, hipStream_t stream);
// out = in, `words` u64 (16-byte aligned rows; an odd last word goes through hipMemcpyAsync)
hipError_t hp_launch_copy(size_t words, const u64 *in, u64 *out, hipStream_t stream);
// rows of a polynomial in separate blocks of registered host memory (device-visible addresses), moved by one kernel
#define HP_HOST_ROWS_MAX 64
struct HpHostRows {
    u64 *p[HP_HOST_ROWS_MAX];
};
hipError_t hp_launch_host_rows(bool to_host, const HpHostRows &rows, u32 count, size_t words, u64 *dev, hipStream_t stream);
hipError_t hp_launch_gather(const u32 *perm, u32 n, u32 rows, const u64 *in, u64 *out, hipStream_t stream);
hipError_t hp_launch_reverse(u32 n, u32 rows, const u64 *in, u64 *out, hipStream_t stream);
// several ciphertexts moved in one launch: ciphertext b = polynomials src[b][0], src[b][1] (u64[L][N] each, anywhere), map perm[b]
// (NULL: involution) -> out u64[count][polys][L][N]; polys = 1: polynomial 0 alone
#define HP_GATHER_TABLE_MAX 32
struct HpGatherTable {
    const u64 *src[HP_GATHER_TABLE_MAX][2];
    const u32 *perm[HP_GATHER_TABLE_MAX];
};
hipError_t hp_launch_gather_many(const HpGatherTable &tab, u32 count, u32 n, u32 L, u64 *out, hipStream_t stream, u32 polys = 2);

// single-vector kernels behind the drop-in mod_arith entry points
enum HpVecOp : int {
    HP_V_BARRETT_LAZY = 0,
    HP_V_BARRETT = 1,
    HP_V_STRICT = 2,
    HP_V_MUL_HYBRID = 3,
    HP_V_MUL_BARRETT = 4,
    HP_V_MONTGOMERY128 = 5
};
struct HpVecConsts {
    u64 q, mqinv, r64, r64h, barrett_c, c128_hi, c128_lo;
};
hipError_t hp_launch_vec(int op, const HpVecConsts &c, size_t n, const u64 *a, const u64 *b, u64 *out,
                         hipStream_t stream);

// ---- scheme-level kernels ---------------------------------------------------------
// ckks/arith.cpp:55-62: ct1, ct2 [P][2][L][n] -> quad [P][3][L][n]
// only limbs [k_first, k_first + kc) are computed (kc = L: all)
hipError_t hp_launch_tensor(const HpLimb *limbs, u32 L, u32 k_first, u32 kc, u32 n, u32 P, const u64 *ct1,
                            const u64 *ct2, u64 *quad, hipStream_t stream);
// the same with the operands by address: polynomials ct1[0], ct1[1], ct2[0], ct2[1] (u64[L][N] each) of pair p at rows.p[p][0..3]
// a chain of lazy sums / differences per polynomial: rows.p[poly * terms + j] = term j of polynomial poly (u64[L][n]), bit j of neg: subtracted
#define HP_FOLD_ROWS_MAX 64
#define HP_FOLD_TERMS_MAX 32
struct HpFoldRows {
    const u64 *p[HP_FOLD_ROWS_MAX];
    u32 neg;
};
hipError_t hp_launch_poly_fold(const HpLimb *limbs, u32 L, u32 n, u32 polys, u32 terms, const HpFoldRows &rows, u64 *out, hipStream_t stream);
#define HP_TENSOR_ROWS_MAX 64
struct HpTensorRows {
    const u64 *p[HP_TENSOR_ROWS_MAX][4];
};
hipError_t hp_launch_tensor_rows(const HpLimb *limbs, u32 L, u32 k_first, u32 kc, u32 n, u32 P, const HpTensorRows &rows, u64 *quad,
                                 hipStream_t stream);
// sum of tensor products (hp_dev_ckks_tensor_sum): term t = the ciphertext batches a[t], b[t], each [P][2][L][n] with words below
// 2 * modulus  -> quad [P][3][L][n] = (sum a0 b0, sum (a0 b1 + a1 b0), sum a1 b1), words below 2 * modulus; add_prev: added to the
// words quad already holds (the launches after the first of a long list).  The addresses travel as kernel arguments.
// terms <= hpi::tensor_sum_max_terms (hp_drop.h): the 128-bit accumulators must stay within the Montgomery step's range
#define HP_TENSOR_SUM_MAX 32
struct HpTensorSumTable {
    const u64 *a[HP_TENSOR_SUM_MAX];
    const u64 *b[HP_TENSOR_SUM_MAX];
    u32 terms;
};
hipError_t hp_launch_tensor_sum(const HpLimb *limbs, u32 L, u32 n, u32 P, const HpTensorSumTable &tab, bool add_prev, u64 *quad,
                                hipStream_t stream);
// linear combination of ciphertexts (hp_lincomb.hip; hp_dev_ckks_lincomb, the linear forms of hp_dev_ckks_eval_plan_hks): term j = the
// batch src[j], [P][2][limbs[j]][n] with limbs[j] >= L and words below 2 * modulus, read in its first L limb rows
//   -> out [P][out_polys][L][n], polynomials 0 and 1 (out_polys = 2: a ciphertext batch; 3: the (d0, d1) of a quad):
//      ([accumulate] out + sum_j coef[j][m] src[j] + (polynomial 0) coef[terms][m]) mod q_m, canonical (below q_m)
// d_coef: DEVICE u64[terms + 1][L], residues below q_m (row `terms`: the constant).  terms <= hpi::lincomb_max_terms (hp_drop.h);
// terms == 0: the constant (and the accumulated word) alone.  The addresses travel as kernel arguments.
#define HP_LINCOMB_MAX 32
struct HpLincombTable {
    const u64 *src[HP_LINCOMB_MAX];
    u32 limbs[HP_LINCOMB_MAX];
    u32 terms;
};
hipError_t hp_launch_ct_lincomb(const HpLimb *limbs, u32 L, u32 n, u32 P, const HpLincombTable &tab, const u64 *d_coef, bool accumulate,
                                u64 *out, u32 out_polys, hipStream_t stream);
// rgsw.cpp:121-153: digits [P][L][L+1][n] (diagonal taken from pt [P][L][n]), key [L][2][L+1][n]
//   -> out [P][2][L+1][n]
// only output moduli [k_first, k_first + kc) of the L+1 are computed (kc = L+1: all)
// key_Le: limbs per key polynomial (L+1, or more for a key generated at a higher level: its last column is the special prime)
// pack_mask: bit k set = the digit rows of output modulus k are in the 48-bit packed row format (needs P >= 2)
// pack40_mask: bit k set = in the 40-bit offset format of parity level A (HP_PACK40; takes precedence)
hipError_t hp_launch_ks_inner(const HpLimb *limbs, u32 L, u32 k_first, u32 kc, u32 key_Le, u32 n, u32 P, const u64 *digits,
                              const u64 *pt, u32 pt_pstride, const u64 *key, u64 *out, u32 pack_mask, u32 pack40_mask,
                              hipStream_t stream);
// the same inner product when every ciphertext has its own key (hp_dev_ckks_rotate_many): key addresses as kernel arguments
#define HP_KEY_TABLE_MAX 32
struct HpKeyTable {
    const u64 *p[HP_KEY_TABLE_MAX];
};
hipError_t hp_launch_ks_inner_many(const HpLimb *limbs, u32 L, u32 k_first, u32 kc, u32 key_Le, u32 n, u32 P, const u64 *digits,
                                   const u64 *pt, u32 pt_pstride, const HpKeyTable &keys, u64 *out, hipStream_t stream);

// drop-last-prime (rescaling.cpp:46-75 / mod_switch.cpp:45-77).  Fused form for the tiled transform (rescaling.cpp:54-74 /
// mod_switch.cpp:52-76 in ONE launch): the forward NTT of the remainder limbs reads the strict last-limb coefficients, applies
// Barrett + centring (+ *t) while loading, and finishes with out = ((x - NTT(rem)) * inv) [* (q_last mod t)] [+ addend] while
// storing.  hp_drop.h has HpDropArgs field by field, at both parity levels.
// job: HP_NTT_BATCH over L-1 limbs and P2 polynomials with src = clast [P2][n] (src_pstride 1, src_kstride 0)
hipError_t hp_launch_ntt_fast_drop(const HpNttJob &job, const HpDropArgs &da, hipStream_t stream);
// the same for a launch of few limbs, split over N / 2048 workgroups per limb (hp_ntt_split.hip); job.dst = scratch rows [P2][kc][n]
hipError_t hp_launch_ntt_split_drop(const HpNttJob &job, const HpDropArgs &da, hipStream_t stream);
// level A (one drop, or two in one transform when da.comb is set); output rows are canonical residues
hipError_t hp_launch_ntt_a_drop(const HpNttJob &job, const HpDropArgs &da, hipStream_t stream);
// level A, inverse of ONE limb (job.L == 1) combined from a row and an addend (HpInvMixArgs, hp_drop.h)
hipError_t hp_launch_ntt_a_inv_mix(const HpNttJob &job, const HpInvMixArgs &mx, hipStream_t stream);

// clast [P2][n] (strict coefficients of the last limb) -> rem [P2][L-1][n]
hipError_t hp_launch_drop_rem(const HpLimb *limbs, const HpDropConsts &dc, u32 Lm1, u32 n, u32 P2,
                              const u64 *clast, u64 *rem, hipStream_t stream);
// x [P2][L][n] (first L-1 limbs used), rem [P2][L-1][n] (NTT form), optional addend [P2][addL][n]
//   -> out [P2][L-1][n]:  out = ((x - rem) * inv) [* qlt]  [+ addend]
// kc limbs per polynomial (L-1: all); for a limb range the caller shifts limbs / dc / x / addend / out to its first limb
hipError_t hp_launch_drop_fin(const HpLimb *limbs, const HpDropConsts &dc, u32 L, u32 kc, u32 n, u32 P2, const u64 *x,
                              const u64 *rem, const u64 *addend, u32 add_poly_stride, u32 add_ct_stride,
                              u32 add_mask, u64 *out, hipStream_t stream);

// constants of the CRT branch of rns_base_transform many -> one (device memory; built by the engine)
#define HP_CRT_MAX_LIMBS 16
struct HpCrtConsts {
    u64 t, q_mod_t;                                                  // new modulus, (q_0 ... q_{L-1}) mod t
    u64 inv[HP_CRT_MAX_LIMBS][HP_CRT_MAX_LIMBS], inv_h[HP_CRT_MAX_LIMBS][HP_CRT_MAX_LIMBS];   // [b][a], b < a: q_b^-1 mod q_a (+ Harvey word)
    u64 half[HP_CRT_MAX_LIMBS];                                      // mixed-radix digits of floor(Q/2)
    u64 pref[HP_CRT_MAX_LIMBS], pref_h[HP_CRT_MAX_LIMBS];            // q_0 ... q_{a-1} mod t (+ Harvey word)
};
// out: polynomial p at out + p*out_pstride*n; not_small == NULL: every polynomial takes the CRT composition
hipError_t hp_launch_base_to_single_crt(const HpLimb *limbs, const HpCrtConsts *cc, u32 L, u32 n, u32 P, const u64 *in, u64 *out,
                                        u32 out_pstride, const u32 *not_small, hipStream_t stream);

// ---- either side of the path ---------------------------------------
// noise [P][n] (int64) -> out rows p*out_pstride + k: the per-modulus lift of sampling.cpp:77-83
hipError_t hp_launch_lift_noise(const HpLimb *limbs, u32 L, u32 n, u32 P, const long long *noise, u64 *out, u32 out_pstride,
                                hipStream_t stream);
// coeffs [P][n] (any int64) -> out rows p*out_pstride + k: the strict residue of every coefficient in every modulus
hipError_t hp_launch_spread_signed(const HpLimb *limbs, u32 L, u32 n, u32 P, const long long *coeffs, u64 *out, u32 out_pstride,
                                   hipStream_t stream);
// ct[p][0] holds NTT(lift(noise)) on entry; c1, ptn [P][L][n], sk [L][n] -> ct [P][2][L][n]   (rlwe.cpp:52,70)
hipError_t hp_launch_enc_fin(const HpLimb *limbs, u32 L, u32 n, u32 P, const u64 *c1, const u64 *sk, const u64 *ptn, u64 *ct,
                             hipStream_t stream);
// out [P][L][n] = c0 + c1*sk   (rlwe.cpp:76)
hipError_t hp_launch_dec_fma(const HpLimb *limbs, u32 L, u32 n, u32 P, const u64 *ct, const u64 *sk, u64 *out,
                             hipStream_t stream);
// rns_transform.cpp:11-37 / :39-84; limbs = plan of the NEW (from_single) / OLD (to_single) moduli
hipError_t hp_launch_base_from_single(const HpLimb *limbs, u64 old_q, u32 L, u32 n, u32 P, const u64 *in, u64 *out,
                                      hipStream_t stream);
hipError_t hp_launch_base_to_single(const HpLimb *limbs, u32 L, u32 n, u32 P, u64 new_q, const u64 *in, u64 *out,
                                    u32 *not_small, hipStream_t stream);

// ---- hybrid key switch (extension; hp_hks.hip) ---------------------------------------------------
#define HP_HKS_MAX_ALPHA 8
#define HP_HKS_MAX_DIGITS 16
struct HpHksConsts {   // device memory, built by the engine per (moduli, k, alpha)
    u32 L, k, alpha, nd, E;   // ciphertext moduli, special primes, limbs per digit, digits, L + k
    // Garner inverses inside digit d: [d][b][a], b < a: (b-th modulus of the digit)^-1 mod (a-th modulus of the digit)
    u64 inv[HP_HKS_MAX_DIGITS][HP_HKS_MAX_ALPHA][HP_HKS_MAX_ALPHA], inv_h[HP_HKS_MAX_DIGITS][HP_HKS_MAX_ALPHA][HP_HKS_MAX_ALPHA];
    // [d][m][a]: product of the first a moduli of digit d, modulo modulus m of the extended chain
    u64 pref[HP_HKS_MAX_DIGITS][HP_MAX_LIMBS][HP_HKS_MAX_ALPHA], pref_h[HP_HKS_MAX_DIGITS][HP_MAX_LIMBS][HP_HKS_MAX_ALPHA];
    u64 pinv[HP_MAX_LIMBS], pinv_h[HP_MAX_LIMBS];   // (p_0...p_{k-1})^-1 mod q_i
    // ModDown (k <= HP_HKS_MAX_ALPHA special primes): Garner inverses among them, digits of floor(P/2), and per ciphertext
    // modulus q_i the prefix products p_0...p_{a-1} mod q_i and P mod q_i
    u64 pg_inv[HP_HKS_MAX_ALPHA][HP_HKS_MAX_ALPHA], pg_inv_h[HP_HKS_MAX_ALPHA][HP_HKS_MAX_ALPHA];
    u64 p_half[HP_HKS_MAX_ALPHA];
    u64 p_pref[HP_MAX_LIMBS][HP_HKS_MAX_ALPHA], p_pref_h[HP_MAX_LIMBS][HP_HKS_MAX_ALPHA];
    u64 p_mod_q[HP_MAX_LIMBS], p_mod_q_h[HP_MAX_LIMBS];
};
// yp [P2][k][n] (strict coefficients of the special-prime part) -> rem [P2][L][n]: the exact centred value in every q_i
hipError_t hp_launch_hks_moddown(const HpLimb *limbs, const HpHksConsts *hc, u32 k, u32 n, u32 P2, const u64 *yp, u64 *rem,
                                 hipStream_t stream);
// ModDown with a plain modulus t (BGV): rem = t * centre( [x]_P * t^-1 mod P ) in every q_i, canonical residues; k <= HP_HKS_MAX_ALPHA.
// What depends on t travels by value, built per call on the host: HpHksConsts stays a function of the chain.
struct HpHksPlain {
    u64 tinv_p[HP_HKS_MAX_ALPHA], tinv_p_h[HP_HKS_MAX_ALPHA];   // t^-1 mod p_a (+ Harvey word)
    u64 t_mod_q[HP_MAX_LIMBS], t_mod_q_h[HP_MAX_LIMBS];         // t mod q_i (+ Harvey word)
};
hipError_t hp_launch_hks_moddown_t(const HpLimb *limbs, const HpHksConsts *hc, const HpHksPlain &pc, u32 k, u32 n, u32 P2, const u64 *yp,
                                   u64 *rem, hipStream_t stream);
hipError_t hp_launch_hks_modup(const HpLimb *limbs, const HpHksConsts *hc, u32 alpha, u32 nd, u32 n, u32 P, const u64 *coef,
                               u64 *lifted, hipStream_t stream);
// The inner products.  KE >= E: the rows of one digit of every key (and of every diagonal) they read -- E for a key of this chain;
// key_L0 + k for one generated for key_L0 >= L ciphertext moduli (the _at entry points), of which modulus m of the level is row
// m + (m >= L ? KE - E : 0): the ciphertext moduli first, the special primes last.  Digit rows, baby rows and accumulators have E rows.
hipError_t hp_launch_hks_inner(const HpLimb *limbs, u32 L, u32 E, u32 KE, u32 nd, u32 alpha, u32 n, u32 P, const u64 *lifted, const u64 *pt,
                               u32 pt_pstride, const u64 *key, u64 *out, hipStream_t stream);
// hoisted rotations: the inner product of R rotations over ONE set of digit rows (of the unrotated polynomials), rotation r reading
// them through map[r] (a cycle map of the context's cache; NULL: the involution) and multiplying by key[r]
//   -> out [P][R][2][E][n]; keys and maps as kernel arguments
#define HP_HOIST_TABLE_MAX 32
struct HpHoistTable {
    const u64 *key[HP_HOIST_TABLE_MAX];
    const u32 *map[HP_HOIST_TABLE_MAX];
};
hipError_t hp_launch_hks_inner_hoisted(const HpLimb *limbs, u32 L, u32 E, u32 KE, u32 nd, u32 alpha, u32 n, u32 P, u32 R, const u64 *lifted,
                                       const u64 *pt, u32 pt_pstride, const HpHoistTable &tab, u64 *out, hipStream_t stream);
// diagonal linear transform in the extended basis (hp_dev_ckks_lintrans_hks): the R rotations of the table weighted and summed
// inside the thread, ct [P][2][L][n] (digit rows `lifted` of its polynomials 1, as for the hoisted product)
//   -> acc [P][2][E][n] = sum_r diag_r * ( sum_d map_r(D_d) * key_r[d] )  + on polynomial 0, limbs < L:  (P mod q) * diag_r * map_r(c0)
// words below 2 * modulus; add_prev: added to the words acc already holds (the launches after the first of a long list).
// R <= hpi::hks_lintrans_max_rotations (hp_drop.h): the 128-bit accumulators must not wrap
struct HpLinTable {   // a table of its own: the hoisted kernel's argument block stays as it is
    const u64 *key[HP_HOIST_TABLE_MAX];
    const u32 *map[HP_HOIST_TABLE_MAX];
    const u64 *diag[HP_HOIST_TABLE_MAX];   // [KE][n] plain words below 2 * modulus, NTT form; NULL: the constant 1
};
hipError_t hp_launch_hks_inner_lintrans(const HpLimb *limbs, const HpHksConsts *hc, u32 E, u32 KE, u32 n, u32 P, u32 R, const u64 *lifted,
                                        const u64 *ct, const HpLinTable &tab, bool add_prev, u64 *acc, hipStream_t stream);
// Baby-step giant-step transform (hp_dev_ckks_lintrans_bsgs_hks): two more flavours of the accumulate kernel, and the pre-sum.
//   babies: rotation r of the table -> its own row set, nothing summed: baby [P][Rtot][2][E][n] (the launch writes the R sets from
//           `baby` on) = sum_d map_r(D_d) * key_r[d]  + on polynomial 0, limbs < L: (P mod q) * map_r(c0); a NULL key: the identity,
//           (P mod q) * c_h on the limbs < L and zero on the special primes.  Words: the bound of w_r plus the folded word (hp_drop.h)
//   giants: the flat call's sum with every rotation reading ITS OWN polynomial -- digit rows `lifted` and rows u of polynomial
//           p * Rtot + r, u [P][Rtot][2][L][n] -- and no diagonal -> acc [P][2][E][n], words below 2 * modulus, add_prev as above
static_assert(HP_BSGS_TABLE_MAX == HP_HOIST_TABLE_MAX, "the plan of hp_drop.h counts in argument tables");
hipError_t hp_launch_hks_bsgs_babies(const HpLimb *limbs, const HpHksConsts *hc, u32 E, u32 KE, u32 n, u32 P, u32 R, u32 Rtot,
                                     const u64 *lifted, const u64 *ct, const HpLinTable &tab, u64 *baby, hipStream_t stream);
hipError_t hp_launch_hks_bsgs_giants(const HpLimb *limbs, const HpHksConsts *hc, u32 E, u32 KE, u32 n, u32 P, u32 R, u32 Rtot,
                                     const u64 *lifted, const u64 *u, const HpLinTable &tab, bool add_prev, u64 *acc, hipStream_t stream);
// pre-sum: dst[g][b][h][m] = sum_i diag[g * babies + i][m] * baby[b][i][h][m] for the `giants` giants and `babies` babies of the
// table (baby row set i of ciphertext b at baby + b * baby_pstride + i * 2 E n; giant g's rows of ciphertext b at
// dst[g] + b * dst_pstride), words below 2 * modulus; a NULL diagonal: the term is absent; add_prev: added to what dst holds.
// babies <= hpi::hks_bsgs_plan's baby_pass (the 128-bit sums), giants * babies <= HP_BSGS_DIAG_MAX, giants <= HP_BSGS_GIANT_MAX
struct HpPreTable {
    const u64 *diag[HP_BSGS_DIAG_MAX];   // [KE][n] plain words below 2 * modulus, NTT form
    u64 *dst[HP_BSGS_GIANT_MAX];
};
hipError_t hp_launch_hks_bsgs_presum(const HpLimb *limbs, u32 L, u32 E, u32 KE, u32 n, u32 P, u32 giants, u32 babies, const u64 *baby,
                                     size_t baby_pstride, const HpPreTable &tab, size_t dst_pstride, bool add_prev, hipStream_t stream);
// key generation (hp_dev_hks_keygen / _rot): keys [R][nd][2][E][n] with NTT(e[r][d]) in keys[r][d][0] on entry (any u64 words) ->
//   keys[r][d][0][m] = (NTT(e) - a[r][d][m] * s_to[m] + (m in digit d) * (P mod q_m) * from_r[m]) * 2^64,  keys[r][d][1][m] = a * 2^64,
// canonical residues.  a [R][nd][E][n], or NULL: the rows already in keys[r][d][1].  from_r = s_from [R][E][n] (maps == NULL), or
// s_to itself read through maps->map[r] (a cycle map of the context's cache; NULL: the involution), R <= HP_HOIST_TABLE_MAX then
struct HpKeygenMaps {
    const u32 *map[HP_HOIST_TABLE_MAX];
};
hipError_t hp_launch_hks_keygen(const HpLimb *limbs, const HpHksConsts *hc, u32 E, u32 nd, u32 n, u32 R, const u64 *s_to, const u64 *s_from,
                                const HpKeygenMaps *maps, const u64 *a, u64 *keys, hipStream_t stream);
// merged ModDown + rescale (hp_engine.cpp: hks_mult): rem[p2][i] += (P mod q_i) * centre(c_last[p2]) for i < L-1, in the
// coefficient domain; c_last = strict coefficients modulo q_{L-1} of the relinearised limb L-1
hipError_t hp_launch_hks_combine(const HpLimb *limbs, const HpHksConsts *hc, u32 L, u32 n, u32 P2, const u64 *clast, u64 *rem,
                                 hipStream_t stream);
hipError_t hp_launch_hks_down_fin(const HpLimb *limbs, const HpHksConsts *hc, u32 L, u32 n, u32 P2, const u64 *x, const u64 *rem,
                                  const u64 *addend, u32 add_poly_stride, u32 add_ct_stride, u32 add_mask, u64 *out,
                                  hipStream_t stream);
// ---- BFV (extension; hp_bfv.hip, constants in hp_bfv.h) ------------------------------------------------------------
// exact centred conversion: src [P][src_ps rows][n], strict coefficient rows modulo the cnt moduli of the plan xs -> dst [P][dst_ps
// rows][n], row m = the canonical residue modulo ys[m] (T of them) of x below floor(X/2), of x - X from there on.  cnt <= HP_BFV_MAX
static_assert(HP_BFV_MAX == HP_CRT_MAX_LIMBS && 2 * HP_BFV_MAX == HP_MAX_LIMBS, "hp_bfv.h counts in the engine's limits");
hipError_t hp_launch_bfv_lift(const HpLimb *xs, const HpLimb *ys, const HpBfvBase *bc, u32 cnt, u32 T, u32 n, u32 P, const u64 *src,
                              u32 src_ps, u64 *dst, u32 dst_ps, hipStream_t stream);
// src [P][L + M][n] strict coefficient rows over moduli_qb (plan limbs) -> y [P][M][n] = floor((t x + h) / Q) modulo every b_j, canonical
hipError_t hp_launch_bfv_scale(const HpLimb *limbs, const HpBfvConsts *bc, const HpBfvPlain &pc, u32 L, u32 n, u32 P, const u64 *src, u64 *y,
                               hipStream_t stream);
// x [P][L][n] strict coefficient rows -> out [P][n] = floor((t x + h) / Q) mod t; bc: the constants of (moduli, L, M = 0)
hipError_t hp_launch_bfv_decrypt_round(const HpLimb *limbs, const HpBfvConsts *bc, const HpBfvDecPlain &pc, u32 L, u32 n, u32 P, const u64 *x,
                                       u64 *out, hipStream_t stream);
// rows of any u64 words -> canonical residues: polynomial p, row k < R (modulus limbs[k]) from src + (p * src_ps + k) * n to
// dst + (p * dst_ps + k) * n; src == dst with equal strides: in place
hipError_t hp_launch_bfv_canonical(const HpLimb *limbs, u32 R, u32 n, u32 P, const u64 *src, u32 src_ps, u64 *dst, u32 dst_ps,
                                   hipStream_t stream);
// device samplers (hp_sample.hip; hp_sample.h has the stream layout).  One thread per ChaCha20 block of 8 words, at most
// HP_SAMPLE_MAX_BLOCKS workgroups of 256 threads to a launch.
// uniform: polynomial b < batch (id stream_id + b), row m < L (modulus rows.q[m], label rows.id[m]) -> out + b * stride + m * N, canonical
// residues; mont_limbs != NULL (the plan of the same moduli): every word times 2^64 mod q instead, canonical.  logn >= 3.
#define HP_SAMPLE_MAX_BLOCKS ((u64)1 << 30)
struct HpSampleRows {
    u64 q[HP_MAX_LIMBS];
    unsigned char id[HP_MAX_LIMBS];
};
hipError_t hp_launch_sample_uniform(const HpSampleSeed &seed, const HpSampleRows &rows, const HpLimb *mont_limbs, u32 L, u32 logn, u64 batch,
                                    u64 stream_id, u64 stride, u64 *out, hipStream_t stream);
// kind HP_SAMPLE_TERNARY / HP_SAMPLE_CBD / HP_SAMPLE_GAUSS: out [batch][N] = scale * the sample of id stream_id + b
hipError_t hp_launch_sample_signed(u32 kind, const HpSampleSeed &seed, u32 logn, u64 batch, u64 stream_id, long long scale, long long *out,
                                   hipStream_t stream);
// fresh ciphertexts.  spread: kind HP_SAMPLE_TERNARY / HP_SAMPLE_CBD / HP_SAMPLE_GAUSS; polynomial p < batch (id stream_id + p * id_step),
// row m < L -> out + p * pstride + m * N = the canonical residues of scale * the sample modulo rows.q[m], coefficient form (rows.id is not read)
hipError_t hp_launch_sample_spread(u32 kind, const HpSampleSeed &seed, const HpSampleRows &rows, u32 L, u32 logn, u64 batch, u64 stream_id,
                                   u64 id_step, long long scale, u64 pstride, u64 *out, hipStream_t stream);
// ciphertext b < batch at ct + b * (with_c1 ? 2 : 1) * L * N, its c0 rows holding NTT(e_b) on entry (lazy transform words):
// c0 = NTT(e) + ptn - a * sk, canonical, a = the uniform sample of id stream_id + b (labels rows.id), written to the c1 rows only
// with_c1.  ptn: rows ptn + b * pt_stride + m * N (lazy transform words; with_c1 they may be the c1 rows), or NULL: zero.  sk [L][N] < 2q
hipError_t hp_launch_enc_seeded(const HpSampleSeed &seed, const HpSampleRows &rows, const HpLimb *limbs, u32 L, u32 logn, u64 batch, u64 stream_id,
                                const u64 *sk, const u64 *ptn, u64 pt_stride, bool with_c1, u64 *ct, hipStream_t stream);
// ct [P][2][L][n] holding NTT(e0), NTT(e1) on entry; pk [2][L][n] < 2q; u, ptn [P][L][n] lazy transform words (ptn may be NULL)
//   -> ct[p] = (pk0 * u + e0 + ptn, pk1 * u + e1), canonical
hipError_t hp_launch_enc_pk_fin(const HpLimb *limbs, u32 L, u32 n, u32 P, const u64 *pk, const u64 *u, const u64 *ptn, u64 *ct,
                                hipStream_t stream);
// x [rows][n] lazy transform words -> canonical residues in place, limb of a row = row % L
hipError_t hp_launch_sample_canonical(const HpLimb *limbs, u32 L, u32 n, u32 rows, u64 *x, hipStream_t stream);
