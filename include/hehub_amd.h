/*
 * hehub_amd.h -- C ABI of the MI355X-native RNS ring-arithmetic engine.
 *
 * This is the drop-in boundary for primihub/hehub's data-parallel hot path
 * (negacyclic NTT/INTT, coefficient-wise modular arithmetic, key-switch inner
 * product, rescale / mod-switch).  hehub has no FFI layer of its own: its seam
 * is the set of free functions in namespace hehub declared in
 *   src/fhe/common/ntt.h, mod_arith.h, rns.h, src/fhe/primitives/rgsw.h,
 *   src/fhe/ckks/ckks.h, src/fhe/bgv/bgv.h .
 * Each entry point below names the reference declaration (file:line, relative
 * to the hehub source tree) it stands in for.  The C++ shim a hehub maintainer
 * links instead of hehub's own .cpp files is hehub_amd/host/ (see
 * INTEGRATION.md).
 *
 * Conventions
 *   - plain C: pointers, sizes, integers.  No torch / STL types.
 *   - every function returns an hp_status; nothing throws across the ABI; a NULL
 *     ctx is HP_EINVAL.  hp_last_error(ctx) gives the message of the calling
 *     thread's last failure on that ctx (valid until its next hp_* call).
 *   - one hp_ctx per GPU; calls on one ctx are serialised by an internal
 *     mutex; different ctxs are independent.
 *   - "host" entry points take caller-owned host pointers, are synchronous and
 *     retain nothing.  "dev" entry points take device pointers (hipMalloc'd by
 *     the caller, by hp_dev_alloc, or by any other allocator in the process,
 *     e.g. a torch tensor's data_ptr()), enqueue on the ctx stream and return
 *     without synchronising.
 *   - device pointers must be 16-byte aligned (the kernels move 16 bytes per lane; every allocator's blocks are, and
 *     so is every limb inside them); a NULL or misaligned operand is rejected with HP_EINVAL before anything runs.
 *   - all words are uint64_t, little-endian, in the reference's lazy
 *     (redundant) representation; outputs are bit-identical to the
 *     reference's for identical inputs.
 *
 * Device layouts (row-major):
 *   polynomial batch   u64[batch][L][N]
 *   ciphertext batch   u64[batch][2][L][N]     (quadratic: [batch][3][L][N])
 *   key-switch key     u64[L][2][L+1][N]       rgsw[j][half][k], Montgomery form
 *                                               (keys.cpp:8-36, rgsw.cpp:33-55)
 */
#ifndef HEHUB_AMD_H
#define HEHUB_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hp_ctx hp_ctx;

typedef enum {
    HP_OK = 0,
    HP_EINVAL = 1,       /* reference would throw std::invalid_argument */
    HP_EUNSUPPORTED = 2, /* reference throws "under development" / not built */
    HP_EHIP = 3,         /* HIP runtime failure */
    HP_ENOMEM = 4,
    HP_ELOGIC = 5,
    HP_ERANGE = 6        /* parity level A only: a kernel was handed a word that is not a lazy word of its limb (see hp_parity_level) */
} hp_status;

/* ---- engine ------------------------------------------------------------ */
int hp_ctx_create(int device, hp_ctx **out);
void hp_ctx_destroy(hp_ctx *ctx);
/* Parity level of the scheme-level pipelines ("Parity levels").
 *   HP_PARITY_B (default): every output word is the raw lazy u64 word hehub's CPU code produces, bit for bit.
 *   HP_PARITY_A (opt-in; HP_PARITY_LEVEL=A in the environment at hp_ctx_create): the key switch, drop-last-prime, relinearisation,
 *     rotation and fused mult entry points (hp_dev_ckks_rescale*, hp_dev_bgv_mod_switch, hp_dev_*_relinearize*,
 *     hp_dev_ckks_rotate* / conjugate*, hp_dev_*_mult_relin_*) return the CANONICAL residue in [0, q) of every word: congruent
 *     to hehub's word modulo its q and equal to reduce_strict (mod_arith.h:58-72) of it -- the contract of
 *     intt_negacyclic_inplace (ntt.h:88-92) extended to the whole pipeline.  hp_dev_ext_prod_montgomery* returns lazy words
 *     (< 2q, rgsw.cpp:151) with hehub's residues.  Their transforms then run on error-free FP64
 *     products (hp_ntt_a.hip: 8 instead of 16 instructions per butterfly).  Needs every modulus of the chain below 2^50 and
 *     exact under hehub's lazy fold (no prime a little above 2^k or well inside its octave: hp_tables.h level_a_modulus), a ring
 *     degree of 2^11 .. 2^15; a call whose chain does not qualify runs at level B.  Input words must be LAZY words of their limb
 *     (below 2 q: everything hehub or this engine produces is; hehub's own transforms take any u64, ntt.cpp:155-175, and level B
 *     reproduces that).  The precondition is CHECKED: every word a level-A kernel loads from a caller's row passes a range guard
 *     (one instruction), a word above 2 q sets a sticky flag, and the next synchronising call on the family (hp_sync,
 *     hp_memcpy_d2h) returns HP_ERANGE -- the results since the previous synchronisation are then void.  At this level the fused mult entry points (hp_dev_*_mult_relin_*) also merge relinearize's
 *     mod-down with the rescale / mod switch into one transform per output limb (same residues; HP_NO_DOUBLE_DROP=1 at
 *     hp_ctx_create keeps the two launches).  The NTT / mod-arith primitives (hp_ntt_*, hp_dev_ntt_*, hp_dev_poly_*, hp_batched_*) are
 *     never affected: they stay bit-exact with ntt.cpp:145-223 / mod_arith.cpp. */
/* A second LANE on the parent's GPU (hehub's callers are loops of independent single-ciphertext operations,
 * src/circuits/linear_algebra.h:109-133, bench/benchmarks.cpp:24-35: one ciphertext fills 10 .. 100 of the 256 CUs, so independent
 * calls should overlap): a context with its own stream and scratch workspace whose calls run concurrently on the device with those
 * of its parent and siblings.  The family shares ONE lock (host-side enqueueing is serialised exactly as on a single context) and ONE
 * copy of the twiddle tables / per-chain constants / gather maps.  Knobs, parity level and error sampler start as the parent's are at
 * the fork.
 * Destroy every member with hp_ctx_destroy (any order).  hp_ctx_wait_for is the ordering primitive between lanes: everything
 * `ctx` enqueues from now on runs after everything `other` has enqueued so far -- a device-side event, no host synchronisation.
 * Buffers are the caller's: a lane that reads what another lane wrote (or reuses memory another lane still reads) needs that
 * ordering; hehub_amd/host keeps the book per device block. */
int hp_ctx_fork(hp_ctx *parent, hp_ctx **out);
int hp_ctx_wait_for(hp_ctx *ctx, hp_ctx *other);
typedef enum { HP_PARITY_B = 0, HP_PARITY_A = 1 } hp_parity_level;
int hp_ctx_set_parity_level(hp_ctx *ctx, int level);
int hp_ctx_get_parity_level(hp_ctx *ctx);
/* The error distribution of the four seeded calls (hp_dev_hks_keygen_seeded, hp_dev_hks_keygen_rot_seeded, hp_dev_rlwe_encrypt_seeded,
 * hp_dev_rlwe_encrypt_pk_seeded): a sampler kind of "Sampling on the device" below, 3 = centred binomial (the default) or 4 = discrete
 * Gaussian of sigma 3.2; anything else is HP_EINVAL and leaves the setting as it was.  A setting of the context like the parity level
 * (hp_ctx_fork copies it); no environment variable.  The getter returns the kind, HP_EINVAL on a NULL context. */
int hp_ctx_set_error_sampler(hp_ctx *ctx, uint32_t kind);
int hp_ctx_get_error_sampler(hp_ctx *ctx);
const char *hp_last_error(hp_ctx *ctx);
const char *hp_version(void);
/* enqueue on an existing hipStream_t (e.g. torch's current stream); NULL = the HIP default stream.
 * A fresh ctx uses a private non-blocking stream; hp_ctx_reset_stream goes back to it.  Switching streams keeps device
 * order: the new stream first waits (event, no host synchronisation) for everything the ctx enqueued on the previous one,
 * because the scratch workspace and the cached tables are shared by all calls of a ctx.
 * HIP graphs: the first hp_dev_* call with a new (ring degree, moduli, shape) builds tables / constants and may grow the
 * workspace (allocations and host-to-device copies); every later call with the same parameters only enqueues kernels on the
 * ctx stream, so it can be recorded with hipStreamBeginCapture on that stream and replayed (tests/test_gpu_parity.py).
 * A later call that needs a LARGER workspace drains the device, frees the old block and allocates a new one: graphs captured
 * before that hold stale scratch pointers and must be re-captured -- hp_ctx_workspace_generation() changes whenever that
 * happened (also on hp_ctx_release_workspace).  Warm up with the largest shape first to avoid it. */
int hp_ctx_set_stream(hp_ctx *ctx, void *hip_stream);
int hp_ctx_reset_stream(hp_ctx *ctx);
void *hp_ctx_get_stream(hp_ctx *ctx);
int hp_sync(hp_ctx *ctx);
/* the engine's scratch workspace grows to the largest call so far and is reused; these report / release it */
size_t hp_ctx_workspace_bytes(hp_ctx *ctx);
unsigned long hp_ctx_workspace_generation(hp_ctx *ctx);
int hp_ctx_release_workspace(hp_ctx *ctx);
int hp_dev_alloc(hp_ctx *ctx, size_t bytes, void **dptr);
int hp_dev_free(hp_ctx *ctx, void *dptr);
/* page-locked host memory for batches that cross PCIe (hp_memcpy_*, the node layer's host entry points): copies from / to it are
 * DMA at the link rate whatever the state of the pages (pageable memory measured 22 .. 48 GB/s from box to box, page-locked
 * 49 .. 52 GB/s); portable across the devices of a node */
int hp_host_alloc(hp_ctx *ctx, size_t bytes, void **hptr);
int hp_host_free(hp_ctx *ctx, void *hptr);
int hp_memcpy_h2d(hp_ctx *ctx, void *dst, const void *src, size_t bytes);
int hp_memcpy_d2h(hp_ctx *ctx, void *dst, const void *src, size_t bytes);
/* Host memory the caller owns, made DMA-able in place (hipHostRegister) -- the limbs of hehub's SmartArray pool
 * (allocator.h:19-22: blocks are recycled, never returned to the OS) can be registered once and then cross PCIe at the link rate
 * without the runtime's staging of pageable memory.  The *_async copies only enqueue on the ctx stream: the host buffer must stay
 * untouched until hp_sync() (or any synchronous hp_* call on the ctx) returns. */
int hp_host_register(hp_ctx *ctx, void *hptr, size_t bytes);
int hp_host_unregister(hp_ctx *ctx, void *hptr);
int hp_memcpy_h2d_async(hp_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int hp_memcpy_d2h_async(hp_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* Device memory of one context -> device memory of another (the two may sit on different GPUs of the node, on one GPU, or be the same
 * context): enqueued on DST's stream.  Order it behind the producer with hp_ctx_wait_for(dst_ctx, src_ctx) first.  Between two GPUs the
 * copy crosses one xGMI link (peer access is enabled for the pair on first use; without it the runtime stages the copy).  hehub has no
 * devices; the host layer uses this when an operand lives on another GPU than the call (hehub_amd/host: "devices"). */
int hp_memcpy_peer_async(hp_ctx *dst_ctx, void *d_dst, hp_ctx *src_ctx, const void *d_src, size_t bytes);
int hp_ctx_device(hp_ctx *ctx);   /* the HIP device ordinal the context was created on (HP_EINVAL < 0 for NULL) */
/* A polynomial whose limbs are SEPARATE registered host blocks (rns.h:15-156: one SmartArray per limb) <-> its contiguous device rows
 * u64[rows][words], by ONE kernel that reads / writes the host blocks over PCIe: 47-49 GB/s either way on an MI355X against
 * 11-17 GB/s for one DMA command per 256 KiB block (tools/ubench/ubench_pcie.hip, profiles/archive/r04_ubench_pcie.txt).  Every h_rows[r] must be
 * 16-byte aligned memory from hp_host_alloc or registered with hp_host_register; words even.  Enqueue only (see above). */
int hp_dev_store_host_rows(hp_ctx *ctx, size_t rows, size_t words, const uint64_t *d_src, uint64_t *const *h_rows);
int hp_dev_load_host_rows(hp_ctx *ctx, size_t rows, size_t words, uint64_t *d_dst, const uint64_t *const *h_rows);
/* The same between device rows that lie ANYWHERE (the ciphertexts of an application are separate objects, rlwe.h:27; the batch
 * entry points below want u64[batch][2][L][N]) and one packed block u64[rows][words]: d_rows is a HOST array of `rows` device
 * pointers, 16-byte aligned; words even.  One streaming kernel per 64 rows on the ctx stream. */
int hp_dev_gather_rows(hp_ctx *ctx, size_t rows, size_t words, const uint64_t *const *d_rows, uint64_t *d_dst);
int hp_dev_scatter_rows(hp_ctx *ctx, size_t rows, size_t words, const uint64_t *d_src, uint64_t *const *d_rows);
/* force the simple one-stage-at-a-time transform kernels (debug / cross-check) */
int hp_ctx_set_force_generic(hp_ctx *ctx, int on);
/* timing of the last profiled launch group: see hp_prof_* below */

/* ---- drop-in, host pointers (one call = one reference call) -------------- */
/* ntt.h:33   void ntt_negacyclic_inplace_lazy(size_t log_dimension, u64 modulus, u64 coeffs[]) */
int hp_ntt_negacyclic_inplace_lazy(hp_ctx *ctx, size_t log_dimension, uint64_t modulus, uint64_t *coeffs);
/* ntt.h:64   void intt_negacyclic_inplace_lazy(size_t log_dimension, u64 modulus, u64 values[]) */
int hp_intt_negacyclic_inplace_lazy(hp_ctx *ctx, size_t log_dimension, uint64_t modulus, uint64_t *values);
/* ntt.h:102  void cache_ntt_factors_strict(u64 log_dimension, const std::vector<u64>&) */
int hp_cache_ntt_factors_strict(hp_ctx *ctx, size_t log_dimension, const uint64_t *moduli, size_t count);
/* Would the engine accept this modulus chain?  Builds (and keeps) exactly what the first real call on the chain builds -- per-limb
 * constants, and for log_dimension != 0 the twiddle tables of every modulus at that ring degree -- and returns what that call would:
 * HP_EINVAL for a modulus the transforms reject (2N does not divide q - 1, more than 59 bits: ntt.cpp:26-29,43-47), for moduli that are
 * not pairwise coprime, for an even modulus when `montgomery` is set (the products of rns.cpp:120-140 need -q^-1 mod 2^64,
 * mod_arith.cpp:49-52); HP_EUNSUPPORTED for a ring degree outside 2 .. 2^16.  log_dimension == 0: no transforms on the chain.
 * The host layer calls this when it RECORDS a call instead of running it, so that the exception comes at the call, as hehub's does. */
int hp_check_chain(hp_ctx *ctx, size_t log_dimension, const uint64_t *moduli, size_t count, int montgomery);
/* mod_arith.h:16   batched_barrett_lazy(modulus, vec_len, vec) */
int hp_batched_barrett_lazy(hp_ctx *ctx, uint64_t modulus, size_t vec_len, uint64_t *vec);
/* mod_arith.h:18   batched_barrett */
int hp_batched_barrett(hp_ctx *ctx, uint64_t modulus, size_t vec_len, uint64_t *vec);
/* mod_arith.h:58   batched_reduce_strict */
int hp_batched_reduce_strict(hp_ctx *ctx, uint64_t modulus, size_t vec_len, uint64_t *vec);
/* mod_arith.h:27   batched_mul_mod_hybrid_lazy(modulus, vec_len, in1, in2, out) */
int hp_batched_mul_mod_hybrid_lazy(hp_ctx *ctx, uint64_t modulus, size_t vec_len, const uint64_t *in1,
                                   const uint64_t *in2, uint64_t *out);
/* mod_arith.h:41   batched_mul_mod_barrett_lazy */
int hp_batched_mul_mod_barrett_lazy(hp_ctx *ctx, uint64_t modulus, size_t vec_len, const uint64_t *in1,
                                    const uint64_t *in2, uint64_t *out);
/* mod_arith.h:55   batched_montgomery_128_lazy(modulus, len, const u128 in[], u64 out[]); in = {lo,hi} pairs */
int hp_batched_montgomery_128_lazy(hp_ctx *ctx, uint64_t modulus, size_t len, const uint64_t *in128,
                                   uint64_t *out);

/* ---- device-resident batches (throughput path) --------------------------- */
/* ntt.h:41-51 / :72-82 applied to every polynomial of a batch u64[batch][L][N], in place.
 * strict != 0 on the inverse also applies reduce_strict (ntt.h:88-92). */
int hp_dev_ntt(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch, uint64_t *d_x);
int hp_dev_intt(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch, uint64_t *d_x,
                int strict);
/* The same transforms as RESIDUES (parity level A as explicit entry points, whatever the context's level; hp_ntt_a.hip: error-free
 * FP64 butterflies, 8 instead of 16 instructions each): in place, every output word is the canonical residue in [0, q).
 *   hp_dev_ntt_residues:  word == (ntt.cpp:145-176's lazy word) mod q, i.e. reduce_strict of it where that one is below 2q
 *   hp_dev_intt_residues: the words of intt_negacyclic_inplace (ntt.h:88-92 = lazy inverse + reduce_strict), bit for bit
 * Input words must be lazy words of their limb (below 2 q; checked: HP_ERANGE from the next hp_sync / hp_memcpy_d2h, see
 * hp_parity_level); N = 2^11 .. 2^15 and every modulus below 2^50 and exact under hehub's lazy fold (as hp_parity_level), else
 * HP_EUNSUPPORTED.  hp_dev_ntt / hp_dev_intt above stay bit-exact with the reference's lazy words. */
int hp_dev_ntt_residues(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch, uint64_t *d_x);
int hp_dev_intt_residues(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch, uint64_t *d_x);
/* rns.cpp:58-87 / :89-118 / :120-140 / :142-171 on u64[batch][L][N].  d_self may alias d_out. */
int hp_dev_poly_add(hp_ctx *ctx, size_t n, size_t L, const uint64_t *moduli, size_t batch,
                    const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out);
int hp_dev_poly_sub(hp_ctx *ctx, size_t n, size_t L, const uint64_t *moduli, size_t batch,
                    const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out);
/* A chain of operator+= / operator-= (rns.cpp:58-87 / :89-118 applied term after term, e.g. the accumulate of the diagonal loop in
 * src/circuits/linear_algebra.h:117-121) folded into one pass: d_out[p] = ((x_0 op_1 x_1) op_2 x_2) ... op_{terms-1} x_{terms-1} with
 * x_j = d_rows[p * terms + j] (u64[L][N] each, anywhere on the device, 16-byte aligned; d_rows itself is a HOST array) and op_j = -=
 * where negate[j] != 0 (negate[0] is ignored).  Each step is the lazy sum / difference of the single call, in the calls' order: the
 * words of the chain of single calls; the intermediate sums never cross HBM.  d_out u64[polys][L][N]: row p may be polynomial p's own
 * x_0 (the chain then runs in place); an output row that overlaps any other input row is refused (HP_EINVAL). */
int hp_dev_poly_fold_rows(hp_ctx *ctx, size_t n, size_t L, const uint64_t *moduli, size_t polys, size_t terms,
                          const uint8_t *negate, const uint64_t *const *d_rows, uint64_t *d_out);
int hp_dev_poly_mul(hp_ctx *ctx, size_t n, size_t L, const uint64_t *moduli, size_t batch,
                    const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out);
/* per-limb scalars (operator*=(vector<u64>)); pass the same value L times for operator*=(u64) */
int hp_dev_poly_scalar_mul(hp_ctx *ctx, size_t n, size_t L, const uint64_t *moduli, size_t batch,
                           const uint64_t *rns_scalar, const uint64_t *d_a, uint64_t *d_out);
/* mod_arith.h:65-72 */
int hp_dev_poly_reduce_strict(hp_ctx *ctx, size_t n, size_t L, const uint64_t *moduli, size_t batch,
                              uint64_t *d_x);
/* allocator.h:113-118 (SmartArray(const SmartArray&): a deep copy) for words that live on the device: d_dst[i] = d_src[i],
 * ranges must not overlap.  One streaming kernel on the ctx stream; bench.py also times it as the measured HBM stream ceiling. */
int hp_dev_copy(hp_ctx *ctx, size_t words, const uint64_t *d_src, uint64_t *d_dst);
/* permutation.cpp:59-75 / :28-57 (NTT-form gathers) */
int hp_dev_poly_involution(hp_ctx *ctx, size_t logn, size_t L, size_t batch, const uint64_t *d_in,
                           uint64_t *d_out);
int hp_dev_poly_cycle(hp_ctx *ctx, size_t logn, size_t L, size_t batch, size_t step, const uint64_t *d_in,
                      uint64_t *d_out);

/* ckks/arith.cpp:55-62, bgv/arith.cpp:59-69: ct1, ct2 u64[batch][2][L][N] -> u64[batch][3][L][N] */
int hp_dev_mult_low_level(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch,
                          const uint64_t *d_ct1, const uint64_t *d_ct2, uint64_t *d_quad);
/* rgsw.h:51  RlweCt ext_prod_montgomery(const RlwePt&, const RgswCt&):
 * pt u64[batch][L][N] (NTT form), key u64[L][2][L+1][N] -> out u64[batch][2][L+1][N].
 * moduli_ext = q_0..q_{L-1}, p. */
int hp_dev_ext_prod_montgomery(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli_ext, size_t batch,
                               const uint64_t *d_pt, const uint64_t *d_key, uint64_t *d_out);
/* ckks.h:313 rescale_inplace(ct, 1) -> rescaling.cpp:14-78: ct u64[batch][2][L][N] -> u64[batch][2][L-1][N] */
int hp_dev_ckks_rescale(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch,
                        const uint64_t *d_ct, uint64_t *d_out);
/* bgv.h:167 mod_switch_inplace(ct, 1) -> mod_switch.cpp:13-78 */
int hp_dev_bgv_mod_switch(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, uint64_t plain_modulus,
                          size_t batch, const uint64_t *d_ct, uint64_t *d_out);
/* ckks.h relinearize (ckks/arith.cpp:64-73): quad u64[batch][3][L][N] -> u64[batch][2][L][N] */
int hp_dev_ckks_relinearize(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli_ext, size_t batch,
                            const uint64_t *d_quad, const uint64_t *d_key, uint64_t *d_out);
/* bgv.h:159 relinearize (bgv/arith.cpp:71-79).  inner_plain_modulus = 1 reproduces the reference. */
int hp_dev_bgv_relinearize(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli_ext,
                           uint64_t inner_plain_modulus, size_t batch, const uint64_t *d_quad,
                           const uint64_t *d_key, uint64_t *d_out);
/* ckks.h:284 rotate(ct, rot_key, step) / ckks.h:282 conjugate(ct, conj_key)  (ckks/arith.cpp:75-93):
 * ct u64[batch][2][L][N], key u64[L][2][L+1][N] -> out u64[batch][2][L][N] */
int hp_dev_ckks_rotate(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli_ext, size_t batch, size_t step,
                       const uint64_t *d_ct, const uint64_t *d_rot_key, uint64_t *d_out);
int hp_dev_ckks_conjugate(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli_ext, size_t batch,
                          const uint64_t *d_ct, const uint64_t *d_conj_key, uint64_t *d_out);
/* ckks.h:270 mult(ct1, ct2, relin_key) followed by ckks.h:313 rescale_inplace:
 * ct1, ct2 u64[batch][2][L][N] -> out u64[batch][2][L-1][N] */
int hp_dev_ckks_mult_relin_rescale(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli_ext,
                                   size_t batch, const uint64_t *d_ct1, const uint64_t *d_ct2,
                                   const uint64_t *d_key, uint64_t *d_out);
/* bgv::mult_low_level + bgv::relinearize + bgv::mod_switch_inplace (bgv.h:150-167) */
int hp_dev_bgv_mult_relin_modswitch(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli_ext,
                                    uint64_t plain_modulus, size_t batch, const uint64_t *d_ct1,
                                    const uint64_t *d_ct2, const uint64_t *d_key, uint64_t *d_out);
/* Extension (SURVEY.md 8c caveat 1): the same pipeline with the inner switch of bgv::relinearize run with the plain modulus t
 * instead of hehub's 1, so that the key-switched term survives and the product decrypts.  The key must be made for it: row j
 * encrypts (p mod q_j) * ((p mod t)^-1 mod q_j) * s^2 in limb j with noise lifted by t (tests/test_extensions.py has the
 * recipe); with hehub's own keys use the parity entry point above.  Equals hp_dev_bgv_relinearize(inner_plain_modulus = t)
 * between hp_dev_mult_low_level and hp_dev_bgv_mod_switch, word for word. */
int hp_dev_bgv_mult_relin_modswitch_t(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli_ext,
                                      uint64_t plain_modulus, size_t batch, const uint64_t *d_ct1,
                                      const uint64_t *d_ct2, const uint64_t *d_key, uint64_t *d_out);

/* ---- either side of the path: what a pipeline needs to keep ciphertexts on the device ---- */
/* rlwe.cpp:57-72 encrypt_core with the samples of get_rlwe_sample supplied by the caller (sampling stays on the host):
 * noise int64[batch][N] rounded Gaussian integers (lifted per modulus and transformed as sampling.cpp:76-86 does),
 * c1 u64[batch][L][N] uniform NTT-form words, pt u64[batch][L][N] coefficient form, sk u64[L][N] NTT form
 * -> ct u64[batch][2][L][N].  (hp_dev_rlwe_encrypt_seeded, further down, draws the samples on the device from a seed.) */
int hp_dev_rlwe_encrypt_core(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch,
                             const int64_t *d_noise, const uint64_t *d_c1, const uint64_t *d_pt, const uint64_t *d_sk,
                             uint64_t *d_ct);
/* rlwe.h decrypt_core (rlwe.cpp:74-81): pt u64[batch][L][N] = strict(INTT(c0 + c1*sk)) */
int hp_dev_rlwe_decrypt_core(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch,
                             const uint64_t *d_ct, const uint64_t *d_sk, uint64_t *d_pt);
/* rns_transform.h rns_base_transform, one modulus -> many (rns_transform.cpp:113 + :11-37):
 * in u64[batch][N] (mod old_modulus, lazy allowed) -> out u64[batch][L][N] */
int hp_dev_rns_base_from_single(hp_ctx *ctx, size_t n, uint64_t old_modulus, size_t L, const uint64_t *new_moduli,
                                size_t batch, const uint64_t *d_in, uint64_t *d_out);
/* rns_base_transform, many -> one, small-coefficient branch (rns_transform.cpp:113 + :39-84):
 * in u64[batch][L][N] -> out u64[batch][N]; d_not_small u32[batch] is set non-zero for a polynomial whose coefficients
 * are not all small -- the reference then composes by CRT with BigInt (:86-104), which stays on the host */
int hp_dev_rns_base_to_single_small(hp_ctx *ctx, size_t n, size_t L, const uint64_t *old_moduli, uint64_t new_modulus,
                                    size_t batch, const uint64_t *d_in, uint64_t *d_out, uint32_t *d_not_small);

/* rns_base_transform, many -> one, COMPLETE (rns_transform.cpp:106-127 with one new modulus): per polynomial the
 * small-coefficient branch when all its coefficients are small, otherwise the CRT composition the reference does with
 * big integers (:86-104) -- here with mixed-radix word arithmetic, same values (including its returning new_modulus
 * itself when new_modulus divides Q - x).  At most 16 odd pairwise-coprime old moduli, new_modulus < 2^62. */
int hp_dev_rns_base_to_single(hp_ctx *ctx, size_t n, size_t L, const uint64_t *old_moduli, uint64_t new_modulus,
                              size_t batch, const uint64_t *d_in, uint64_t *d_out);

/* ---- limb-range stages: the limb-sharded ("latency") mode across GPUs -------------------------------------
 * one ciphertext operation is cut by OUTPUT MODULUS.  Rank g owns a contiguous range
 * [k0,k1) of the extended moduli q_0..q_{L-1},p.  Every buffer keeps the single-GPU layout of the entry points
 * above; a stage reads what it needs and writes only the limbs it is asked for, so ranks owning disjoint ranges
 * fill disjoint parts of identical buffers and exchange them between stages (hehub_amd/sharded.py: all-gather of
 * the coefficient-form digit limbs, broadcast of the one coefficient limb a drop needs).  Every sum over the
 * digits j is still formed on ONE GPU in the reference's order, so results stay bit-identical (Level B). */
/* ckks/arith.cpp:55-62 for the limbs k in [k0,k1) of L */
int hp_dev_mult_low_level_range(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch, size_t k0,
                                size_t k1, const uint64_t *d_ct1, const uint64_t *d_ct2, uint64_t *d_quad);
/* rgsw.cpp:103-105 for the digits j in [j0,j1) of L: coef[p][j] = strict(INTT(pt[p][j])).
 * pt: polynomial p starts pt_pstride limbs after polynomial p-1; coef u64[batch][L][N] */
int hp_dev_ks_coef_range(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli_ext, size_t batch, size_t j0,
                         size_t j1, const uint64_t *d_pt, size_t pt_pstride, uint64_t *d_coef);
/* rgsw.cpp:108-153 for the output moduli k in [k0,k1) of L+1: needs ALL L limbs of coef, writes out[p][half][k] */
int hp_dev_ks_inner_range(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli_ext, size_t batch, size_t k0,
                          size_t k1, const uint64_t *d_coef, const uint64_t *d_pt, size_t pt_pstride,
                          const uint64_t *d_key, uint64_t *d_out);
/* The same when the caller vouches that every row of coef holds strict residues (the rows were written by hp_dev_ks_coef_range, here or
 * on another rank): the digit rows of the workspace may then be packed (HP_PACK48), and at parity level A the digit transforms run on
 * the FP64 kernels (same residues; the output words are then lazy words with hehub's residues, as hp_dev_ext_prod_montgomery's). */
int hp_dev_ks_inner_range_strict(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli_ext, size_t batch, size_t k0,
                                 size_t k1, const uint64_t *d_coef, const uint64_t *d_pt, size_t pt_pstride,
                                 const uint64_t *d_key, uint64_t *d_out);
/* rescaling.cpp:47-50 / mod_switch.cpp:47-50 (plain_modulus 0 = CKKS): clast[p2] = strict(INTT_{q_last}(x[p2][L-1]))
 * for P2 polynomials of L limbs; run by the owner of the limb that is being dropped.  clast u64[P2][N] */
int hp_dev_drop_coeffs(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, uint64_t plain_modulus, size_t P2,
                       const uint64_t *d_x, uint64_t *d_clast);
/* rescaling.cpp:54-74 / mod_switch.cpp:52-76 for the limbs k in [k0,k1) of the L-1 that stay, given clast:
 * out[p2][k] = ((x[p2][k] - NTT_k(rem_k(clast[p2]))) * q_last^-1) [* (q_last mod t)] [+ addend], x u64[P2][L][N],
 * out u64[P2][L-1][N]; addend row of polynomial p2, limb k: (p2>>1)*add_ct_stride + (p2&1)*add_poly_stride + k,
 * applied to polynomial h = p2&1 of each ciphertext when bit h of add_mask is set (NULL: none) */
int hp_dev_drop_apply_range(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, uint64_t plain_modulus,
                            size_t P2, size_t k0, size_t k1, const uint64_t *d_x, const uint64_t *d_clast,
                            const uint64_t *d_addend, size_t add_poly_stride, size_t add_ct_stride, unsigned add_mask,
                            uint64_t *d_out);
/* The same when the caller vouches that every word of clast is below q_last (the rows were written by hp_dev_drop_coeffs):
 * where q_last <= 2 q_k the remainder of rescaling.cpp:54-58 is then one conditional subtraction instead of a Barrett quotient --
 * the canonical residue either way, so the words are identical.  hp_dev_drop_apply_range makes no such assumption.
 * The _strict stages (this one, hp_dev_ks_inner_range_strict) and hp_dev_ks_coef_range / hp_dev_drop_coeffs follow the context's parity
 * level: at HP_PARITY_A the limb-sharded pipeline returns canonical residues like the single-GPU entry points. */
int hp_dev_drop_apply_range_strict(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, uint64_t plain_modulus,
                                   size_t P2, size_t k0, size_t k1, const uint64_t *d_x, const uint64_t *d_clast,
                                   const uint64_t *d_addend, size_t add_poly_stride, size_t add_ct_stride, unsigned add_mask,
                                   uint64_t *d_out);

/* ---- node: several GPUs behind one handle (hehub_amd/csrc/hp_node.cpp) ------------------------------------------
 * hehub is a single-threaded CPU library; an application that holds a BATCH of ciphertexts uses all GPUs of a node through
 * this layer, from C, without Python.  A node owns one hp_ctx (own stream) and one worker thread per rank; ranks may share
 * a device (devices = {0, 0}: how the one-GPU tests exercise it).  Calls on a node are serialised.
 *
 * Batch-sharded mode (the throughput mode): item i of the batch belongs to the rank whose contiguous slice
 * [lo, hi) holds i (hp_node_slice; sizes differ by at most one); every rank runs the single-GPU entry point on its
 * slice; keys are replicated once (hp_node_replicate); there is NO exchange on the data path. */
typedef struct hp_node hp_node;
int hp_node_create(const int *devices, size_t count, hp_node **out);
void hp_node_destroy(hp_node *node);
size_t hp_node_size(const hp_node *node);
hp_ctx *hp_node_ctx(hp_node *node, size_t rank);      /* the rank's engine context, for the hp_dev_* entry points */
/* hp_ctx_set_parity_level on every rank's context: the batch-sharded entry points below then return canonical residues (level A);
 * the limb-sharded mode follows it too since round 5 (its stages run on rows the engine wrote itself: hp_dev_*_range_strict) */
int hp_node_set_parity_level(hp_node *node, int level);
const char *hp_node_last_error(hp_node *node);   /* "rank r: <message of that rank's failing call>"; the first rank with a failure of its own */
/* matrix[a * size + b] = 1 when rank a can write rank b's device memory directly (same device, or hipDeviceEnablePeerAccess
 * succeeded at hp_node_create), else 0.  The limb-sharded plan below writes peers directly where it can and stages through
 * page-locked host memory where it cannot (sender: one device-to-host copy of its block; receiver: host-to-device after the
 * rendezvous).  HP_NODE_NO_PEER in the environment at hp_node_create forces 0 for every pair a != b (tests / debugging). */
int hp_node_peer_matrix(const hp_node *node, int *matrix);
/* NUMA placement: every rank's worker thread is bound to the CPUs of the socket its GPU hangs off (PCI address of the HIP device ->
 * sysfs numa_node -> that node's cpulist, intersected with the process's affinity mask; HP_NODE_NO_AFFINITY in the environment at
 * hp_node_create leaves the threads alone).  hp_node_placement reports what was done for a rank (numa_node -1 / cpus_bound 0: the
 * platform does not say, nothing was bound); hp_device_numa is the lookup itself, for a process that places its own ranks
 * (bench.py binds each rank's process the same way). */
int hp_node_placement(const hp_node *node, size_t rank, int *numa_node, int *cpus_bound);
int hp_device_numa(int device, int *numa_node, char *cpulist, size_t cap);
int hp_node_slice(const hp_node *node, size_t total, size_t rank, size_t *lo, size_t *hi);
int hp_node_sync(hp_node *node);
/* copy a read-only host object (a key-switching key) to every rank: d_copies[rank] receives the device pointers */
int hp_node_replicate(hp_node *node, const uint64_t *h_words, size_t words, uint64_t **d_copies);
int hp_node_free_replicas(hp_node *node, uint64_t **d_copies);
/* host-resident batches (what a hehub application holds): each rank stages its slice in, computes, stages it out
 * ckks.h:270 mult + ckks.h:313 rescale_inplace / bgv mult_low_level + relinearize + mod_switch_inplace:
 * h_ct1, h_ct2 u64[batch][2][L][N] -> h_out u64[batch][2][L-1][N]; d_key[rank] from hp_node_replicate */
int hp_node_ckks_mult_relin_rescale(hp_node *node, size_t logn, size_t L, const uint64_t *moduli_ext, size_t batch,
                                    const uint64_t *h_ct1, const uint64_t *h_ct2, uint64_t *const *d_key, uint64_t *h_out);
int hp_node_bgv_mult_relin_modswitch(hp_node *node, size_t logn, size_t L, const uint64_t *moduli_ext, uint64_t plain_modulus,
                                     size_t batch, const uint64_t *h_ct1, const uint64_t *h_ct2, uint64_t *const *d_key,
                                     uint64_t *h_out);
/* ntt.h:41-51 / :72-92 on a host-resident batch u64[batch][L][N], in place */
int hp_node_ntt(hp_node *node, size_t logn, size_t L, const uint64_t *moduli, size_t batch, uint64_t *h_x, int inverse,
                int strict);
/* device-resident slices: rank r works on counts[r] items behind d_*[r] (allocated on hp_node_ctx(node, r)) */
int hp_node_dev_ckks_mult_relin_rescale(hp_node *node, size_t logn, size_t L, const uint64_t *moduli_ext, const size_t *counts,
                                        const uint64_t *const *d_ct1, const uint64_t *const *d_ct2, uint64_t *const *d_key,
                                        uint64_t *const *d_out);
int hp_node_dev_bgv_mult_relin_modswitch(hp_node *node, size_t logn, size_t L, const uint64_t *moduli_ext, uint64_t plain_modulus,
                                         const size_t *counts, const uint64_t *const *d_ct1, const uint64_t *const *d_ct2,
                                         uint64_t *const *d_key, uint64_t *const *d_out);
/* Limb-sharded ("latency") mode: ONE batch processed by all ranks, cut by output modulus (the limb-range stages above);
 * rank r owns a contiguous range of q_0..q_{L-1}, p (hp_node_sharded_range; sizes differ by at most one, the special prime
 * in a smallest range).  Exchanges are direct peer writes: the owner copies its limbs into every peer's buffer (one xGMI link
 * per shard, no ring, no padding), ordered by HIP events; all buffers belong to the plan.  Pairs without peer access
 * (hp_node_peer_matrix) go through the owner's page-locked staging buffer instead.  With L+1 moduli over W ranks the
 * speed-up is bounded by (L+1) / ceil((L+1)/W): 11 moduli over 8 GPUs -> 5.5 x.  plain_modulus 0: CKKS pipeline. */
typedef struct hp_node_sharded hp_node_sharded;
/* How the plans made FROM NOW ON exchange their limbs (the four exchanges of one multiplication: the all-gather of the key-switch
 * coefficient limbs, the broadcasts of the two dropped limbs' coefficients, the all-gather of the result limbs):
 *   HP_TRANSPORT_PEER    (default) direct peer writes, one xGMI link per shard, ordered by HIP events (staged through page-locked host
 *                        memory for a pair without peer access)
 *   HP_TRANSPORT_RCCL    the collective the north star names: ncclAllGather of the packed, padded per-rank parts and ncclBroadcast from
 *                        the owner, on the ranks' streams.  librccl.so is loaded when this is first asked for (the engine does not link
 *                        it); one communicator rank per node rank (ncclCommInitAll over the node's devices), so every rank needs its
 *                        own device -- HP_EUNSUPPORTED otherwise, or when the library cannot be loaded
 *   HP_TRANSPORT_PACKED  the same packed send / receive buffers as _RCCL, moved by plain device copies (ranks that share a GPU cannot
 *                        form a communicator: this is how the one-GPU tests cover the packing)
 * Every sum over the digits for an output modulus is formed on ONE rank in hehub's order (rgsw.cpp:98-153) whatever the transport:
 * the words are identical under all three (tests/test_gpu_node.py). */
enum { HP_TRANSPORT_PEER = 0, HP_TRANSPORT_RCCL = 1, HP_TRANSPORT_PACKED = 2 };
int hp_node_set_transport(hp_node *node, int transport);
int hp_node_get_transport(const hp_node *node);
int hp_node_sharded_create(hp_node *node, size_t logn, size_t L, const uint64_t *moduli_ext, uint64_t plain_modulus, size_t batch,
                           hp_node_sharded **out);
void hp_node_sharded_destroy(hp_node_sharded *plan);
int hp_node_sharded_range(const hp_node_sharded *plan, size_t rank, size_t *k0, size_t *k1);
/* host operands (copied to every rank), result gathered on rank 0 and copied back */
int hp_node_sharded_mult(hp_node_sharded *plan, const uint64_t *h_ct1, const uint64_t *h_ct2, uint64_t *const *d_key,
                         uint64_t *h_out);
/* operands already replicated on every rank; every rank ends up with the whole result in d_out[rank] */
int hp_node_sharded_mult_dev(hp_node_sharded *plan, const uint64_t *const *d_ct1, const uint64_t *const *d_ct2,
                             uint64_t *const *d_key, uint64_t *const *d_out);

/* ---- extensions beyond the reference ---------------------------------------------------
 * hehub throws for both cases; these entry points are additions, not replacements, and are pinned by equivalence to
 * the reference-parity entry points (tests/test_extensions.py):
 * (1) a key-switching key generated for key_L0 ciphertext moduli used at a LOWER level L <= key_L0 (hehub requires
 *     exactly L+1 limbs, rgsw.cpp:84-87, so one key serves one level only): key u64[key_L0][2][key_L0+1][N]; digit rows
 *     j >= L and modulus columns L..key_L0-1 are ignored, the special prime is the last column.  moduli_ext stays
 *     q_0..q_{L-1}, p.  Identical, word for word, to calling the plain entry point with the extracted sub-key.
 * (2) rescale by several primes (hehub: "under development", rescaling.cpp:83-85) = successive exact one-prime drops. */
int hp_dev_ext_prod_montgomery_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, const uint64_t *moduli_ext,
                                  size_t batch, const uint64_t *d_pt, const uint64_t *d_key, uint64_t *d_out);
int hp_dev_ckks_relinearize_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, const uint64_t *moduli_ext,
                               size_t batch, const uint64_t *d_quad, const uint64_t *d_key, uint64_t *d_out);
int hp_dev_ckks_rotate_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, const uint64_t *moduli_ext, size_t batch,
                          size_t step, const uint64_t *d_ct, const uint64_t *d_rot_key, uint64_t *d_out);
int hp_dev_ckks_conjugate_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, const uint64_t *moduli_ext,
                             size_t batch, const uint64_t *d_ct, const uint64_t *d_conj_key, uint64_t *d_out);
/* (3) ckks.h:284 rotate / ckks.h:282 conjugate of `batch` ciphertexts, EACH WITH ITS OWN KEY AND STEP: hehub's circuits rotate one
 *     vector by many steps, every step under its own key (src/circuits/linear_algebra.h:123-130: rotate(ct_vec, rot_key_set[s]) for
 *     2 (width - 1) values of s) -- independent calls, but no two share a key, so the one-key batch form above does not apply.
 *     d_ct u64[batch][2][L][N]; steps[b] and d_keys[b] (a HOST array of device addresses, key b laid out as for
 *     hp_dev_ckks_rotate_at with key_L0) belong to ciphertext b; conj (may be NULL) marks the ciphertexts that are conjugated
 *     instead (their step is ignored).  -> d_out u64[batch][2][L][N], word for word what `batch` calls of
 *     hp_dev_ckks_rotate_at / hp_dev_ckks_conjugate_at with batch 1 write (ckks/arith.cpp:75-93). */
int hp_dev_ckks_rotate_many(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, const uint64_t *moduli_ext, size_t batch,
                            const size_t *steps, const unsigned char *conj, const uint64_t *d_ct,
                            const uint64_t *const *d_keys, uint64_t *d_out);
/*     The same with the ciphertexts' polynomials anywhere in device memory: d_polys[2 b + h] (a HOST array of device addresses) is
 *     polynomial h of ciphertext b, u64[L][N] -- an application's ciphertexts are separate objects, and the rotations of ONE vector
 *     (linear_algebra.h:123-130) all read the same two polynomials: no packed copy of the batch is made. */
int hp_dev_ckks_rotate_many_rows(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, const uint64_t *moduli_ext, size_t batch,
                                 const size_t *steps, const unsigned char *conj, const uint64_t *const *d_polys,
                                 const uint64_t *const *d_keys, uint64_t *d_out);
/* (4) The fused multiplication pipelines with the OPERANDS BY ADDRESS: d_polys[4 b + {0, 1, 2, 3}] (a HOST array of device addresses)
 *     = polynomials ct1[b][0], ct1[b][1], ct2[b][0], ct2[b][1], u64[L][N] each, anywhere in device memory.  An application's
 *     ciphertexts are separate objects (hehub's are: ckks.h:73-93); the packed forms above would cost a gather of 4 L limbs per pair
 *     (12 % of a C3 step), here the tensor product -- the only kernel that reads the operands -- takes the addresses as arguments.
 *     Same words as hp_dev_ckks_mult_relin_rescale_at / hp_dev_bgv_mult_relin_modswitch. */
int hp_dev_ckks_mult_relin_rescale_rows(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, const uint64_t *moduli_ext,
                                        size_t batch, const uint64_t *const *d_polys, const uint64_t *d_key, uint64_t *d_out);
int hp_dev_bgv_mult_relin_modswitch_rows(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli_ext,
                                         uint64_t plain_modulus, size_t batch, const uint64_t *const *d_polys,
                                         const uint64_t *d_key, uint64_t *d_out);
int hp_dev_ckks_mult_relin_rescale_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, const uint64_t *moduli_ext,
                                      size_t batch, const uint64_t *d_ct1, const uint64_t *d_ct2,
                                      const uint64_t *d_key, uint64_t *d_out);
/* (3) many -> many base conversion (hehub: "under development", rns_transform.cpp:123): the exact CRT value x of every
 *     coefficient, centred around Q/2 the way the many -> one CRT branch does it (x mod m below the half,
 *     m - ((Q - x) mod m) from the half on), in every new modulus.  in u64[batch][L][N] -> out u64[batch][Lnew][N] */
int hp_dev_rns_base_many_to_many(hp_ctx *ctx, size_t n, size_t L, const uint64_t *old_moduli, size_t Lnew,
                                 const uint64_t *new_moduli, size_t batch, const uint64_t *d_in, uint64_t *d_out);
/* (4) hybrid key switch: alpha consecutive ciphertext moduli form one digit (dnum = ceil(L/alpha) digits) and k special
 *     primes p_0..p_{k-1} (product >= every digit's modulus product) replace hehub's single one: dnum*(L+k) - L digit
 *     transforms per switch instead of L*L.  moduli_ext = q_0..q_{L-1}, p_0..p_{k-1}.  The key has its own format,
 *     u64[dnum][2][L+k][N], NTT + Montgomery form like hehub's: row d is an RLWE encryption, under all L+k moduli, of
 *     (P mod q_i) * s_from in the limbs i of digit d and of 0 elsewhere -- hehub's key is the case alpha = 1, k = 1.
 *     Every step is exact integer arithmetic (ModUp / ModDown by mixed-radix composition), pinned by an exact integer
 *     model and by decryption (tests/test_hks.py); results are NOT comparable with hehub's (different keys, less noise).
 *     Limits: alpha <= 8, at most 16 digits, k <= 16 (one fused conversion kernel up to k = 8), L + k <= 32.
 *     hp_dev_hks_switch: pt u64[batch][L][N] (NTT form) -> out u64[batch][2][L][N] with out0 + out1*s ~ pt*s_from. */
int hp_dev_hks_switch(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t batch,
                      const uint64_t *d_pt, const uint64_t *d_key, uint64_t *d_out);
/* ckks::rotate / conjugate with a hybrid rotation / conjugation key: ct u64[batch][2][L][N] -> out u64[batch][2][L][N] */
int hp_dev_ckks_rotate_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                           size_t batch, size_t step, const uint64_t *d_ct, const uint64_t *d_rot_key, uint64_t *d_out);
int hp_dev_ckks_conjugate_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                              size_t batch, const uint64_t *d_ct, const uint64_t *d_conj_key, uint64_t *d_out);
/* Hoisted rotations: every ciphertext of d_ct u64[batch][2][L][N] rotated by steps[r] (conjugated where conj[r] != 0; conj may
 * be NULL, a conjugation ignores its step) and switched with the hybrid key d_keys[r] -- a HOST array of `rotations` device
 * addresses, each key u64[dnum][2][L+k][N] as for hp_dev_hks_switch -- into d_out u64[batch][rotations][2][L][N].  The digits
 * of c1 (L inverse transforms, ModUp, L*(dnum-1) + k*dnum forward transforms) are computed ONCE per ciphertext; every rotation
 * reads the transformed digit rows through its own index map inside the inner product and then pays only ModDown:
 * 2k inverse + 2L forward transforms per rotation instead of L + L*(dnum-1) + k*dnum + 2k + 2L (L = 10, k = 4, alpha = 3:
 * 28 instead of 84, plus 56 once per call).
 * Moving a transformed digit row is the transform of the moved digit read as a SIGNED integer (the automorphism's negated
 * coefficients stay -x in every modulus), where hp_dev_ckks_rotate_hks lifts the non-negative residues of the moved polynomial:
 * on the lifted limbs the words DIFFER from hp_dev_ckks_rotate_hks's (step 0 excepted).  Both representatives are bounded by the
 * digit's modulus product, so the noise bound is the same and both results decrypt alike.
 * HP_EINVAL before anything is enqueued: the limits of hp_dev_hks_switch, rotations == 0, a step >= 2^17 (not a conjugation), a
 * NULL or misaligned key address, d_out overlapping d_ct. */
int hp_dev_ckks_rotate_hoisted_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                   size_t batch, size_t rotations, const size_t *steps, const unsigned char *conj,
                                   const uint64_t *d_ct, const uint64_t *const *d_keys, uint64_t *d_out);
/* Diagonal linear transform, double hoisted: d_out u64[batch][2][L][N] ~ sum_r diag_r * rot_r(ct) -- the diagonal loop of a
 * matrix-vector product -- with steps, conj and d_keys as for hp_dev_ckks_rotate_hoisted_hks and d_diags a HOST array of
 * `rotations` device addresses: diagonal r as u64[L+k][N], NTT form over the EXTENDED chain (the caller encodes it modulo the
 * special primes too), plain lazy words (not Montgomery form); a NULL entry is the constant 1.
 * Every diagonal word MUST be below 2 * modulus, at either parity level: unlike the other level-B calls this one does not take any
 * u64 there -- a larger word can wrap the 128-bit sum over the rotations unnoticed, and the residues are then undefined.
 * The weighted sum is formed in the basis Q*P before ModDown: with D the digit rows of the unrotated c1 and move_r rotation r's
 * cycle / involution,
 *     acc[b][h][m] = sum_r diag_r[m] * ( sum_d move_r(D[b][d][m]) * key_r[d][h][m] )        for all L + k moduli m
 *     out[b][h]    = ModDown(acc[b][h]) + (h == 0) * sum_r diag_r[:L] * move_r(c0[b])        (mod each q_i; words < 2 q_i)
 * so a call costs ONE digit stage, one accumulate kernel and ONE ModDown per ciphertext whatever `rotations` is (L = 10, k = 4,
 * alpha = 3, 16 rotations: 84 transforms instead of the hoisted call's 504), its workspace is that of hp_dev_hks_switch, and the
 * result carries the rounding of one ModDown instead of the sum of R scaled ones.  The contract is on residues, as for every
 * hybrid call; parity level A follows the context.
 * HP_EINVAL before anything is enqueued: the limits of hp_dev_hks_switch, rotations == 0, a step >= 2^17 (not a conjugation), a
 * NULL or misaligned key address, a misaligned diagonal address, d_out overlapping d_ct in any way.  HP_EUNSUPPORTED: moduli so
 * large (near 2^61 with 16 digits, 2^62 at the latest) that one rotation's products no longer fit the 128-bit accumulators. */
int hp_dev_ckks_lintrans_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                             size_t batch, size_t rotations, const size_t *steps, const unsigned char *conj,
                             const uint64_t *d_ct, const uint64_t *const *d_keys, const uint64_t *const *d_diags,
                             uint64_t *d_out);
/* Diagonal linear transform, baby-step giant-step: with every rotation r of a matrix written r = g + i over `babies` baby steps i
 * and `giants` giant steps g,
 *     d_out u64[batch][2][L][N] ~ sum_g rot_g( sum_i diag_{g,i} * rot_i(ct) )
 * with babies + giants hybrid keys where hp_dev_ckks_lintrans_hks needs babies * giants (16 x 16 diagonals at N = 32768, L = 10, k = 4,
 * alpha = 3: 32 keys of 29.4 MB instead of 256, 7.5 GB).  baby_steps / baby_conj / d_baby_keys and giant_steps / giant_conj /
 * d_giant_keys are HOST arrays as for hp_dev_ckks_rotate_hoisted_hks (conj may be NULL), the keys u64[dnum][2][L+k][N].
 * d_diags is a HOST array of giants * babies device addresses, entry g * babies + i being diag_{g,i} as u64[L+k][N]: NTT form over the
 * EXTENDED chain, plain lazy words, every word BELOW 2 * modulus at either parity level -- the precondition of
 * hp_dev_ckks_lintrans_hks, for its reason: a larger word can wrap a 128-bit sum unnoticed and the residues are then undefined.
 * !! A NULL diagonal means the term (g, i) is ABSENT.  In hp_dev_ckks_lintrans_hks a NULL diagonal is the constant 1.  The two calls
 * !! differ here on purpose: real matrices are sparse in (g, i).
 * !! The call does NOT rotate the diagonals.  To apply the matrix with diagonals diag_r the caller passes
 * !! diag_{g,i} = rot_g^-1(diag_{g+i}): the outer rotation by g then moves the weight back to where diag_{g+i} has it.
 * A NULL key is allowed exactly on an entry with step 0 that is not a conjugation: that entry is the identity and pays no key switch,
 * baby or giant alike.  A step-0 entry WITH a key is switched like any other.
 * The contract is on residues, every output word below 2 q_i.  With D(x) the digit rows of polynomial x, move_s the cycle /
 * involution of entry s and unmont = 2^-64 (the keys are in Montgomery form), for every one of the L + k moduli m:
 *     baby_i[h][m] = unmont * sum_d move_i(D(c1)[d][m]) * key_i[d][h][m]  + (h == 0, m < L) * (P mod q_m) * move_i(c0[m])
 *                    (identity baby: (m < L) * (P mod q_m) * c_h[m], zero on the special primes)
 *     pre_g[h][m]  = sum_i diag_{g,i}[m] * baby_i[h][m]                                          (absent terms skipped)
 *     identity giant:  acc[h][m] += pre_g[h][m]                                                  (no ModDown, no digits, no key)
 *     other giants:    (u0, u1) = ModDown(pre_g);
 *                      acc[h][m] += unmont * sum_d move_g(D(u1)[d][m]) * key_g[d][h][m]  + (h == 0, m < L) * (P mod q_m) * move_g(u0[m])
 *     out[h]       = ModDown(acc[h])
 * The baby results stay in the basis Q*P, each keyed giant pays one ModDown and one digit stage, and all of them go through every stage
 * together: the launch count does not grow with `giants` (beyond one argument table of 32 entries per launch).  The workspace depends
 * on (N, L, k, alpha, batch, babies, giants) alone.  Parity level A follows the context.
 * HP_EINVAL before anything is enqueued: the limits of hp_dev_hks_switch, babies == 0 or giants == 0, a step >= 2^17 (not a
 * conjugation), a NULL key on an entry that is not the identity, a misaligned key or diagonal address, a giant step all of whose
 * diagonals are NULL, d_out overlapping d_ct in any way.  HP_EUNSUPPORTED: moduli as large as hp_dev_ckks_lintrans_hks refuses. */
int hp_dev_ckks_lintrans_bsgs_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t batch,
                                  size_t babies, const size_t *baby_steps, const unsigned char *baby_conj, const uint64_t *const *d_baby_keys,
                                  size_t giants, const size_t *giant_steps, const unsigned char *giant_conj, const uint64_t *const *d_giant_keys,
                                  const uint64_t *const *d_diags, const uint64_t *d_ct, uint64_t *d_out);
/* ckks::mult_low_level + relinearisation with a hybrid key + rescale by q_{L-1}: out u64[batch][2][L-1][N].
 * For N = 2^11 .. 2^15 ModDown and the rescale share one transform per limb: the residues of hp_dev_hks_switch followed by
 * hp_dev_ckks_rescale, in a lazy representative (< 2q) of their own; HP_HKS_TWO_STEP=1 in the environment at hp_ctx_create
 * runs the two steps separately and reproduces those words. */
int hp_dev_ckks_mult_relin_rescale_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha,
                                       const uint64_t *moduli_ext, size_t batch, const uint64_t *d_ct1,
                                       const uint64_t *d_ct2, const uint64_t *d_key, uint64_t *d_out);
/* Lazy relinearisation: sums of ciphertext products that pay ONE hybrid key switch.  Everything after the tensor product is linear in
 * the quadratic ciphertext (d0, d1, d2), so, residue for residue,
 *     rescale(relin(sum_t a_t (x) b_t)) = rescale(sum_t (d0_t, d1_t) + switch(sum_t d2_t))
 * with the noise of one switch and one rounding instead of T: an encrypted dot product, a row of a matrix-matrix product, a sum of
 * squares, the power-basis combinations of a polynomial evaluation.
 *
 * hp_dev_ckks_tensor_sum: d_a and d_b are HOST arrays of `terms` device addresses (an application's ciphertexts are separate objects:
 * the convention of d_keys in the hoisted calls), each a batch u64[batch][2][L][N] in NTT form.  d_quad u64[batch][3][L][N] =
 *     d0 = sum_t a0 b0,    d1 = sum_t (a0 b1 + a1 b0),    d2 = sum_t a1 b1        (mod each q_i; every word below 2 q_i)
 * in the layout of hp_dev_mult_low_level.  The contract is on residues: with one term they are those of hp_dev_mult_low_level, in a
 * lazy representative of their own.
 * Every operand word MUST be below 2 * modulus, at either parity level: unlike the other level-B calls this one does not take any
 * u64 there -- a larger word can wrap the 128-bit sum over the terms unnoticed, and the residues are then undefined.
 * d_a[t] == d_b[t] (squares) and repeated addresses are allowed; d_quad must not overlap any operand.  One streaming kernel, one
 * launch per 32 terms, 32 * terms + 24 bytes of device memory traffic per output word; no workspace.
 * HP_EINVAL before anything is enqueued: L == 0 or L > 32, batch == 0, terms == 0, a NULL array, a NULL or misaligned address in
 * either array, d_quad NULL, misaligned or overlapping an operand.  HP_EUNSUPPORTED: a modulus of 2^62 or more. */
int hp_dev_ckks_tensor_sum(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch, size_t terms,
                           const uint64_t *const *d_a, const uint64_t *const *d_b, uint64_t *d_quad);
/* hp_dev_ckks_relin_rescale_hks: the tail of hp_dev_ckks_mult_relin_rescale_hks on the caller's quadratic ciphertexts d_quad
 * u64[batch][3][L][N], words below 2q (what hp_dev_mult_low_level and hp_dev_ckks_tensor_sum write): hybrid relinearisation of d2,
 * + (d0, d1), rescale by q_{L-1} -> d_out u64[batch][2][L-1][N].  The same code as the fused call after its tensor product: on the
 * same quad, the same words.  The workspace is the fused call's minus its quad block.
 * HP_EINVAL as for hp_dev_ckks_mult_relin_rescale_hks, and d_out overlapping d_quad. */
int hp_dev_ckks_relin_rescale_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                  size_t batch, const uint64_t *d_quad, const uint64_t *d_key, uint64_t *d_out);
/* hp_dev_ckks_dot_relin_rescale_hks: the two calls above in one -- the sum into a workspace quad, then the tail:
 * d_out u64[batch][2][L-1][N] = rescale(relin(sum_t a_t (x) b_t)), d_a / d_b as for hp_dev_ckks_tensor_sum over the first L moduli
 * of moduli_ext, with its precondition on the operand words.  d_out must not overlap any operand.  One workspace reservation, a
 * function of (N, L, k, alpha, batch) alone, never of `terms`.
 * HP_EINVAL before anything is enqueued: everything either call above refuses. */
int hp_dev_ckks_dot_relin_rescale_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                      size_t batch, size_t terms, const uint64_t *const *d_a, const uint64_t *const *d_b,
                                      const uint64_t *d_key, uint64_t *d_out);
/* Hybrid keys generated for key_L0 ciphertext moduli used at a LOWER level L <= key_L0 -- extension (1) for the hybrid path: one
 * top-level key set serves every level of a circuit (hp_dev_ckks_mult_relin_rescale_hks returns L-1 limbs; the next call takes the
 * same keys).  Every _at call has the plain call's arguments with key_L0 after L:
 *   - moduli_ext stays the chain of the LEVEL: q_0..q_{L-1}, p_0..p_{k-1};
 *   - every key is u64[ceil(key_L0/alpha)][2][key_L0+k][N], as hp_dev_hks_keygen writes it for q_0..q_{key_L0-1}, p_0..p_{k-1};
 *     digit rows d >= ceil(L/alpha) and modulus rows L..key_L0-1 are ignored, the special primes are the last k rows;
 *   - the diagonals of the two linear transforms follow the same rule: u64[key_L0+k][N], encoded once over the top chain, read in
 *     rows 0..L-1 and key_L0..key_L0+k-1;
 *   - ciphertexts, outputs and workspace are those of the plain call at L.
 * Digits are cut at multiples of alpha from limb 0, so the limbs below L of level digit d are a subset of top digit d, and row d of
 * the top key restricted to those moduli IS the key hp_dev_hks_keygen writes for the level's chain from the same a rows and the same
 * e (P >= every digit product holds a fortiori).  Identical, word for word and at either parity level, to the plain entry point on
 * the extracted sub-key (and diagonals); with key_L0 == L it is the plain call.  Only the inner products' key and diagonal addresses
 * differ: no copy is made.
 * HP_EINVAL before anything is enqueued: everything the plain call refuses, key_L0 < L, key_L0 + k > 32, ceil(key_L0/alpha) > 16. */
int hp_dev_hks_switch_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext,
                         size_t batch, const uint64_t *d_pt, const uint64_t *d_key, uint64_t *d_out);
int hp_dev_ckks_rotate_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext,
                              size_t batch, size_t step, const uint64_t *d_ct, const uint64_t *d_rot_key, uint64_t *d_out);
int hp_dev_ckks_conjugate_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                 size_t batch, const uint64_t *d_ct, const uint64_t *d_conj_key, uint64_t *d_out);
int hp_dev_ckks_rotate_hoisted_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                      const uint64_t *moduli_ext, size_t batch, size_t rotations, const size_t *steps,
                                      const unsigned char *conj, const uint64_t *d_ct, const uint64_t *const *d_keys, uint64_t *d_out);
int hp_dev_ckks_lintrans_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                size_t batch, size_t rotations, const size_t *steps, const unsigned char *conj, const uint64_t *d_ct,
                                const uint64_t *const *d_keys, const uint64_t *const *d_diags, uint64_t *d_out);
int hp_dev_ckks_lintrans_bsgs_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                     const uint64_t *moduli_ext, size_t batch, size_t babies, const size_t *baby_steps,
                                     const unsigned char *baby_conj, const uint64_t *const *d_baby_keys, size_t giants,
                                     const size_t *giant_steps, const unsigned char *giant_conj, const uint64_t *const *d_giant_keys,
                                     const uint64_t *const *d_diags, const uint64_t *d_ct, uint64_t *d_out);
int hp_dev_ckks_mult_relin_rescale_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                          const uint64_t *moduli_ext, size_t batch, const uint64_t *d_ct1, const uint64_t *d_ct2,
                                          const uint64_t *d_key, uint64_t *d_out);
int hp_dev_ckks_relin_rescale_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                     const uint64_t *moduli_ext, size_t batch, const uint64_t *d_quad, const uint64_t *d_key,
                                     uint64_t *d_out);
int hp_dev_ckks_dot_relin_rescale_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                         const uint64_t *moduli_ext, size_t batch, size_t terms, const uint64_t *const *d_a,
                                         const uint64_t *const *d_b, const uint64_t *d_key, uint64_t *d_out);
/* Polynomial evaluation: the non-linear half of a CKKS program (a sigmoid, GELU or comparison approximated by a polynomial, the
 * EvalMod step of bootstrapping) over the hybrid key switch.  The engine is exact integer arithmetic and "scale" is the caller's
 * notion, so -- as with keys and diagonals -- the caller supplies the constants: the NTT form of a constant is that constant in every
 * position, so a plaintext constant is an integer given by its residues, and no encoder is involved.
 *
 * hp_dev_ckks_lincomb: d_out u64[batch][2][L][N] = sum_{j < terms} coef_j * ct_j + cst  (mod each q_m), every word CANONICAL (< q_m),
 * the same at either parity level.  d_cts is a HOST array of device addresses (the convention of hp_dev_ckks_tensor_sum); ciphertext
 * j is a batch u64[batch][2][ct_limbs[j]][N] with ct_limbs[j] >= L, read in its first L limb rows -- dropping limbs costs no copy.
 * coefs is a HOST array of HOST pointers, coefs[j] = the L residues of coefficient j, each below q_m (coefs == NULL or coefs[j] ==
 * NULL: 1); cst = L residues below q_m, added to every position of polynomial 0 only (NULL: 0).
 * Every operand word MUST be below 2 * modulus (the precondition of hp_dev_ckks_tensor_sum, for its reason: a larger word can wrap the
 * 128-bit sums unnoticed).  One streaming kernel, one launch per 32 terms (fewer from q = 2^61 on), one reduction per output word,
 * 8 * (terms + 1) bytes of device memory traffic per output word; the workspace holds the coefficients, (terms + launches) * L words.
 * HP_EINVAL before anything is enqueued: L == 0 or L > 32, batch == 0, terms == 0, a NULL array (coefs and cst excepted), a NULL or
 * misaligned operand address, ct_limbs[j] < L or > 32, a coefficient or constant residue >= its modulus, d_out NULL, misaligned or
 * overlapping an operand.  HP_EUNSUPPORTED: a modulus of 2^62 or more. */
int hp_dev_ckks_lincomb(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch, size_t terms,
                        const uint64_t *const *d_cts /* HOST */, const size_t *ct_limbs /* each >= L */,
                        const uint64_t *const *coefs /* HOST, entries u64[L] or NULL */, const uint64_t *cst, uint64_t *d_out);
/* hp_dev_ckks_eval_plan_hks: a straight-line program of steps of ONE kind.  Element 0 is the input batch d_ct u64[batch][2][L][N];
 * element s + 1 is the result of step s.  A linear form over earlier elements is F = sum_j coef_j * E_{elem_j} + cst, coef_j and cst
 * HOST arrays of `level` residues below q_m (coef == NULL: 1, cst == NULL: 0; cst goes to polynomial 0 only).  Step s:
 *     E_{s+1} = rescale_{q_{level-1}}( relin( sum_{t < products} X_t (x) Y_t ) + Z )               -> level - 1 limbs
 * Every referenced element is read in its first `level` limb rows (its own limb count must be >= level: the mod-drop, no copy).
 * products == 0: the step is rescale(Z) by hp_dev_ckks_rescale's code, no key switch.  This expresses a power B_a B_b, the Chebyshev
 * recurrence rescale(relin(2 T_a (x) T_b) - kappa T_{a-b}), a leaf sum_j lambda_j B_j + c, the flat recombination
 * sum_g leaf_g (x) G_g under ONE key switch, and the recursive form node = left (x) G + right.
 * A step is, word for word and at either parity level (which follows the context), this composition of the calls above at
 * moduli_ext = q_0..q_{level-1}, p_0..p_{k-1}: each X, Y form by hp_dev_ckks_lincomb into workspace (a form of one term with coef ==
 * NULL, cst == NULL and an element of exactly `level` limbs is passed by address, no copy); the quadratic sum into a workspace quad
 * -- products == 1: the tensor product of hp_dev_ckks_mult_relin_rescale_hks_at (with pass-through forms the step IS that call),
 * more: hp_dev_ckks_tensor_sum --; Z added to the quad's (d0, d1) by the lincomb kernel; hp_dev_ckks_relin_rescale_hks_at on it.
 * After the last step, final_drops rescales by hp_dev_ckks_rescale_n's code: d_out u64[batch][2][level_last - 1 - final_drops][N].
 * d_relin_key: as the _at calls take it, generated for key_L0 >= L ciphertext moduli; one key serves every level.
 * Every operand word of d_ct MUST be below 2 * modulus.
 * Workspace, reserved once before anything is enqueued, a function of (N, k, alpha, batch, the plan's levels and counts), with
 * pad = rounded up to 256 bytes and B = batch:
 *     sum over the forms that are not passed by address of (terms + launches) * level words            the constants
 *   + sum_s pad(B 2 (level_s - 1) N)                every element stays live (the last is d_out itself when final_drops == 0)
 *   + 2 pad(B 2 (level_last - 2) N)                 only with final_drops >= 2
 *   + the largest, over the steps, of  materialised forms * pad(B 2 level N) + pad(B 3 level N) + the workspace of
 *     hp_dev_ckks_relin_rescale_hks_at at that level  (products == 0: pad(B 2 level N) + hp_dev_ckks_rescale's).
 * HP_EINVAL before anything is enqueued, d_out untouched: a NULL or misaligned pointer, steps == 0 or > 64, level < 2, a level above
 * a referenced element's limb count (or above L), a reference to an element not yet computed, an X or Y form with no term, a step
 * with neither a product nor a term, a coefficient or constant residue >= its modulus, final_drops that leaves no limb, d_out
 * overlapping d_ct; and everything the _at calls refuse at any of the plan's levels, with their code.  HP_EUNSUPPORTED: a modulus of
 * 2^62 or more.
 * Out of scope: a tree-mode (depth-optimal, recursive) plan builder; the node, sharded and C++ host layers; CKKS encoding; the
 * odd/even polynomial optimisation; freeing dead elements. */
typedef struct { uint32_t elem; const uint64_t *coef; } hp_eval_term;                 /* coef: HOST u64[level], NULL = 1 */
typedef struct { uint32_t terms; const hp_eval_term *term; const uint64_t *cst; } hp_eval_form;
typedef struct { uint32_t level, products; const hp_eval_form *x, *y; hp_eval_form z; } hp_eval_step;
int hp_dev_ckks_eval_plan_hks(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                              const uint64_t *moduli_ext /* q_0..q_{L-1}, p_0..p_{k-1} */, size_t batch,
                              size_t steps, const hp_eval_step *plan, size_t final_drops,
                              const uint64_t *d_ct, const uint64_t *d_relin_key /* as the _at calls, for key_L0 */,
                              uint64_t *d_out /* u64[batch][2][level_last - 1 - final_drops][N] */);
/* hp_dev_ckks_mod_raise: the first step of bootstrapping -- a ciphertext that has reached its last limb q_0 is read as a ciphertext
 * over the whole chain q_0 .. q_{L-1}.  d_ct is u64[batch][2][in_limbs][N] in NTT form, of which only limb row 0 is read (the
 * mod-drop convention of hp_dev_ckks_lincomb: no copy); every word read MUST be below 2 q_0.  With c = INTT_{q_0}(row 0) taken
 * strict in [0, q_0) and v_i = c_i where c_i < floor(q_0 / 2), c_i - q_0 from there on (the centring of
 * hp_dev_rns_base_from_single), d_out u64[batch][2][L][N] holds, as RESIDUES like every hybrid call's output: row m >= 1 congruent
 * to NTT_{q_m}(v mod q_m), row 0 congruent to the input's row 0 and canonical, every word below 2 q_m; for every modulus the
 * residues equal those of hp_dev_intt (strict) on row 0, hp_dev_rns_base_from_single, hp_dev_ntt.  The raised ciphertext decrypts
 * to m + q_0 I for a small integer polynomial I, which the rest of a bootstrap removes (hehub_amd/bootstrap.py).
 * For N = 2^11 .. 2^15 at parity level B: one strict inverse transform of the 2 * batch rows into workspace, then ONE forward launch
 * of 2 * batch * (L - 1) transforms whose loads centre and reduce the coefficient row -- the lifted block is never written: L + 4
 * rows per polynomial cross device memory instead of the 3 L + 3 of the three calls -- and a canonical copy of row 0.  Other ring
 * degrees, launches of few transforms (the split-limb path's) and parity level A compose the existing kernels on d_out; at level A
 * every word is canonical where the chain has level-A transforms.
 * Workspace: 2 * batch * N words, a function of (N, batch) alone, reserved before anything is enqueued.
 * HP_EINVAL before anything is enqueued, d_out untouched: L < 2 or L > 32, in_limbs == 0 or > 32, batch == 0, a NULL or misaligned
 * pointer, d_out overlapping d_ct, a repeated modulus, a modulus the transforms refuse (2N does not divide q - 1).
 * HP_EUNSUPPORTED: a modulus of more than 59 bits as hehub counts them (q >= 2^59.5).  That is the transforms' own limit; the
 * lift's arithmetic -- a residue below q plus q - (q_0 mod q), or (floor(q_0 / q) + 1) q - q_0 + c <= q_0 + q in the composed form --
 * needs only q_0 + q < 2^64.
 * The rest of a bootstrap -- CoeffToSlot, EvalMod, SlotToCoeff -- is a plan over the calls above (hp_dev_ckks_lintrans_bsgs_hks_at,
 * hp_dev_ckks_rescale, hp_dev_ckks_conjugate_hks_at, hp_dev_ckks_lincomb, hp_dev_ckks_eval_plan_hks) built and run by
 * hehub_amd/bootstrap.py, because scales are the caller's notion.  Out of scope: sparse packing / SubSum; a single C entry for the
 * pipeline (a C caller chains the same calls); the node, sharded and C++ host layers; a device encoder; sparse-secret encapsulation;
 * the arcsine correction; iterated bootstrapping; hoisting across factors. */
int hp_dev_ckks_mod_raise(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli /* q_0..q_{L-1} */, size_t in_limbs, size_t batch,
                          const uint64_t *d_ct /* u64[batch][2][in_limbs][N] */, uint64_t *d_out /* u64[batch][2][L][N] */);
/* Hybrid keys generated on the device.  In the three calls below the uniform rows a and the error polynomials e are INPUTS (the
 * seeded forms further down draw them on the device, hp_dev_sample_*), so
 * a call is deterministic and every output word is pinned by the exact model (tests/test_gpu_hks_keygen.py); what runs here is the
 * arithmetic -- residues of small signed polynomials, batched forward transforms, one streaming multiply-add in Montgomery form.
 * None of the three calls needs workspace: the error rows are spread into d_keys[r][d][0] and transformed there in place.
 *
 * hp_dev_poly_from_signed: small signed polynomials -> NTT form.  Coefficient i of polynomial b as a strict residue of every modulus
 * (a negative c maps to q_m - (|c| mod q_m), to 0 when that is q_m; defined for every int64_t, INT64_MIN included), then the forward
 * transform: row [b][m] holds the words hp_dev_ntt produces from those residues.  How a ternary secret or an error polynomial gets
 * to the device.  HP_EINVAL: L == 0 or L > 32, batch == 0, a pointer that is NULL or not 16-byte aligned, d_out overlapping d_coeffs. */
int hp_dev_poly_from_signed(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch,
                            const int64_t *d_coeffs /* i64[batch][N] */, uint64_t *d_out /* u64[batch][L][N] */);
/* hp_dev_hks_keygen: `keys` keys u64[dnum][2][L+k][N] for hp_dev_hks_switch and every call built on it.  With P = p_0...p_{k-1},
 * E = L + k, dnum = ceil(L / alpha) and digit d = the limbs d*alpha .. min((d+1)*alpha, L) - 1, for key r, digit d, modulus m < E:
 *     b[m]            = NTT(e[r][d])[m] - a[r][d][m] * s_to[m] + (m in digit d) * (P mod q_m) * s_from[r][m]      (mod q_m)
 *     key[r][d][0][m] = b[m]       * 2^64 mod q_m
 *     key[r][d][1][m] = a[r][d][m] * 2^64 mod q_m
 * Every output word is the CANONICAL residue (< q_m) at either parity level: the words of keygen() in tests/hks_model.py given the same
 * a and e.  The key switches a polynomial under s_from to s_to; a relinearisation key is s_from = s * s (hp_dev_poly_mul).
 * d_a == NULL: row a[r][d] already lies, in plain form, in d_keys[r][d][1] and is converted to Montgomery form in place (a key set
 * then needs no second buffer of half its size).
 * HP_EINVAL before anything is enqueued: the limits of hp_dev_hks_switch, keys == 0, a NULL pointer (d_a excepted), a pointer that is
 * not 16-byte aligned, d_keys overlapping any input.  Chains that hp_dev_hks_switch refuses are refused with its code. */
int hp_dev_hks_keygen(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t keys,
                      const uint64_t *d_s_to,    /* u64[L+k][N]        NTT form, words < 2 * modulus            */
                      const uint64_t *d_s_from,  /* u64[keys][L+k][N]  NTT form, words < 2 * modulus; only the limbs < L are read */
                      const uint64_t *d_a,       /* u64[keys][dnum][L+k][N] uniform rows, NTT form, words < 2 * modulus; may be NULL */
                      const int64_t *d_e,        /* i64[keys][dnum][N] error polynomials, coefficient domain    */
                      uint64_t *d_keys);         /* u64[keys][dnum][2][L+k][N]                                  */
/* hp_dev_hks_keygen_rot: rotation / conjugation keys -- the same call with s_to = s and s_from[r] = move_r(s), move_r being
 * hp_dev_poly_involution where conj[r] != 0 and hp_dev_poly_cycle by steps[r] otherwise: key r is the one the rotate entry points take
 * for that entry.  steps and conj are HOST arrays as for hp_dev_ckks_rotate_hoisted_hks (conj may be NULL; a conjugation ignores its
 * step).  The moved secret is read through the automorphism's index map inside the kernel, never materialised.
 * HP_EINVAL as for hp_dev_hks_keygen, and for a step >= 2^17 on an entry that is not a conjugation. */
int hp_dev_hks_keygen_rot(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t keys,
                          const size_t *steps, const unsigned char *conj, const uint64_t *d_s /* u64[L+k][N] */,
                          const uint64_t *d_a, const int64_t *d_e, uint64_t *d_keys);
/* Sampling on the device: a counter-based ChaCha20 keystream (RFC 8439 section 2.3, 20 rounds) and four samplers over it.  Every
 * output is a function of (seed, stream) alone -- no generator state, no host draws, nothing crossing PCIe -- and is pinned word for
 * word by tests/sample_model.py and tests/gauss_model.py.  (hehub's samplers use a default-seeded std::default_random_engine and double arithmetic that is
 * not exact above 2^53; they are not reproduced: its rounded Gaussian, std::round of a std::normal_distribution draw, has no
 * portable word-for-word definition, so the Gaussian below is an exact integer rule over the same stream.)
 *
 * The stream.  One block yields 16 output words o[0..15] and serves the 8 coefficients 8j .. 8j+7 of one row, so logn >= 3; its state:
 *     words 0-3    the four ChaCha constants
 *     words 4-11   the 32 seed bytes as little-endian u32
 *     word  12     the block index j
 *     word  13     attempt (bits 0-15) | kind << 16 (bits 16-23) | limb_id << 24 (bits 24-31)
 *     words 14,15  low / high half of the 64-bit polynomial id
 * Coefficient 8j + c owns the candidate v_c = o[2c] | o[2c+1] << 32 (keystream bytes 8c .. 8c+7, little-endian).  The kind (1 uniform,
 * 2 ternary, 3 centred binomial, 4 discrete Gaussian) keeps the samplers from sharing keystream under one (seed, stream).  Polynomial b of a call has the
 * id stream + b in 64-bit arithmetic.
 *   uniform, modulus q (2 <= q < 2^63): w = v_c & (2^bit_length(q) - 1), accepted when w < q; otherwise the same candidate position
 *     of the same block under attempt + 1.  Bounded: after 64 rejected attempts (0 .. 63; probability < 2^-64 per word, acceptance
 *     being at least 1/2) the word is w - q of the last candidate.  The canonical residue; a row is sampled directly as an NTT-form
 *     row (uniform in either domain).  limb_id is the caller's label of the modulus, by default the row index.
 *   ternary (limb_id 0, attempt 0): the first of the 32 two-bit fields of v_c, from the low end, that is not 3, minus 1; 0 if all are 3.
 *   centred binomial, eta = 21 (limb_id 0, attempt 0): popcount(v_c & (2^21 - 1)) - popcount((v_c >> 21) & (2^21 - 1)): range +-21,
 *     variance 10.5 (sigma 3.24: close to hehub's default std_dev = 3.2, but a binomial, not a Gaussian).
 *   discrete Gaussian, sigma = 16/5 (limb_id 0, attempt 0): the distribution D_{Z,3.2} of the HE security standard's tables, by a
 *     cumulative table.  rho(k) = exp(-25 k^2 / 512), S = the sum of rho(k) over all integers k; a magnitude m has the probability
 *     P(0) = rho(0) / S, P(m) = 2 rho(m) / S.  C[m] = floor(2^63 * (P(0) + ... + P(m))) for m = 0 .. 29 -- 30 entries, integer literals
 *     of hp_sample.h; C[29] = 2^63 - 1, and so would every further entry be.  sign = v_c & 1, u = v_c >> 1 (63 bits),
 *     m = #{ i in 0..29 : u >= C[i] }; the word is -m where sign = 1 and m != 0, else m.  Range +-30, variance 10.24, zero carries no
 *     sign; statistical distance to D_{Z,3.2} below 2^-57.  One candidate per coefficient and all 30 compares whatever the value: the
 *     work does not depend on what is drawn.
 *
 * hp_dev_sample_uniform: row m of polynomial b goes to d_out + b * stride + m * N words, stride = stride_words, or L * N where that
 * is 0; the words between the rows of two polynomials are not touched (uniform rows can be written straight into d_keys[r][d][1]).
 * hp_dev_sample_ternary / hp_dev_sample_cbd / hp_dev_sample_gauss: i64[batch][N], for hp_dev_poly_from_signed or as error rows.
 * HP_EINVAL before anything is enqueued: logn < 3 or above 16, L == 0 or L > 32, batch == 0, a modulus < 2 or >= 2^63, a limb id
 * >= 256, a stride that is odd or below L * N, a NULL seed or moduli, a device pointer that is NULL or not 16-byte aligned.
 * Out of scope: a wire kind for half keys; sparse / fixed-Hamming-weight secrets; discrete Gaussians of any other width, or from a
 * run-time table; Gaussian secrets; sampling inside the inner product; the node, sharded and C++ host layers. */
int hp_dev_sample_uniform(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli,
                          const uint32_t *limb_ids /* HOST, L entries < 256, NULL = 0..L-1 */, size_t batch,
                          const uint8_t *seed /* HOST, 32 bytes */, uint64_t stream,
                          size_t stride_words /* 0 = L*N; else >= L*N and even */, uint64_t *d_out);
int hp_dev_sample_ternary(hp_ctx *ctx, size_t logn, size_t batch, const uint8_t *seed, uint64_t stream,
                          int64_t *d_out /* i64[batch][N] */);
int hp_dev_sample_cbd(hp_ctx *ctx, size_t logn, size_t batch, const uint8_t *seed, uint64_t stream, int64_t *d_out);
int hp_dev_sample_gauss(hp_ctx *ctx, size_t logn, size_t batch, const uint8_t *seed, uint64_t stream, int64_t *d_out);
/* The seeded key generators: hp_dev_hks_keygen / hp_dev_hks_keygen_rot on rows drawn here.  For key r, digit d, with the polynomial id
 * stream + r * dnum + d:  a[r][d] is the uniform sample over all L + k moduli with limb ids 0 .. L+k-1, e[r][d] is error_scale times
 * the sample of the context's error sampler (hp_ctx_set_error_sampler: centred binomial by default, or discrete Gaussian; error_scale
 * = 1 for CKKS, = t for BGV, whose keys need error rows t * e).  The key is word for word
 * what the plain call writes for those rows: the samplers write a into the [1] halves and e into workspace, then the plain call's
 * in-place path (d_a == NULL) runs.  Workspace: keys * dnum * N words, whatever L and k are.
 * hp_dev_hks_key_expand rewrites only the [r][d][1] halves (a * 2^64 mod q_m, canonical) from (seed, stream) and leaves the [0]
 * halves as the caller loaded them: a key set can be stored or shipped as its [0] halves plus 40 bytes.
 * HP_EINVAL before anything is enqueued: logn < 3, a NULL seed, keys == 0, error_scale == 0 or >= 2^58 (21 * error_scale, or 30 * error_scale
 * under the Gaussian sampler, must fit an int64_t); then everything the plain call refuses, with its code. */
int hp_dev_hks_keygen_seeded(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t keys,
                             const uint64_t *d_s_to, const uint64_t *d_s_from, const uint8_t *seed, uint64_t stream,
                             uint64_t error_scale, uint64_t *d_keys);
int hp_dev_hks_keygen_rot_seeded(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t keys,
                                 const size_t *steps, const unsigned char *conj, const uint64_t *d_s, const uint8_t *seed,
                                 uint64_t stream, uint64_t error_scale, uint64_t *d_keys);
int hp_dev_hks_key_expand(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t keys,
                          const uint8_t *seed, uint64_t stream, uint64_t *d_keys);
/* Fresh ciphertexts from a seed: secrets, public keys, secret-key and public-key encryption drawn on the device from the stream
 * above.  The contract of the seeded key generators holds for the three calls: every output word is the CANONICAL residue (< q_m),
 * the same word at either parity level, a function of (seed, stream) and the inputs alone; a refusal comes before anything is
 * enqueued and leaves the output untouched.  hp_dev_rlwe_encrypt_core (caller's noise and c1 rows, hehub's lazy words) is unchanged.
 *
 * hp_dev_sample_small_ntt: kind 2 (ternary) or 3 (centred binomial); polynomial b has the id stream + b.  Row [b][m] holds the
 * canonical residues of the words hp_dev_poly_from_signed produces from scale * hp_dev_sample_ternary / _cbd(seed, stream + b) --
 * the same polynomial, reduced below q_m -- without the int64 rows ever reaching memory: one thread turns a block into the
 * residues of its 8 coefficients in all L moduli (a coefficient v, |v| <= 21 * scale, maps to |v| mod q_m, negated to q_m - r where
 * v < 0 and r != 0), the forward transform and one reduction follow.  How a secret, or the u of a public-key encryption, gets to
 * the device from 40 bytes.  The call uses the ids stream .. stream + batch - 1.  (Kind 4 is not taken here: Gaussian rows in NTT form
 * are hp_dev_poly_from_signed of hp_dev_sample_gauss; the seeded calls below draw theirs in registers the same way as the binomial ones.)
 *
 * hp_dev_rlwe_encrypt_seeded: for ciphertext b, with the polynomial id stream + b:  a_b = the uniform sample over `moduli` with limb
 * ids 0 .. L-1, e_b = error_scale times the sample of the context's error sampler (hp_ctx_set_error_sampler; the kind tag
 * keeps the two apart), and
 *     c1 = a_b        c0 = NTT(e_b) + NTT(pt_b) - a_b * s      (mod q_m)
 * error_scale = 1 is the CKKS form, error_scale = t the BGV form t * e - a * s + m.  d_pt is in coefficient form, hp_dev_ntt's input
 * contract; NULL is the zero plaintext.  The call uses the ids stream .. stream + batch - 1.
 *   with_c1 == 1: d_ct is u64[batch][2][L][N] = (c0, c1).
 *   with_c1 == 0: d_ct is u64[batch][L][N], c0 alone -- the ciphertext is c0 plus the 40 bytes (seed, stream), half the bytes to store
 *     or ship.  There is no expand call: with c0_b copied to the [0] half of ciphertext b,
 *         hp_dev_sample_uniform(ctx, logn, L, moduli, NULL, batch, seed, stream, 2 * L * N, d_ct + L * N)
 *     writes exactly the c1 rows of the with_c1 == 1 call.
 *   d_pt == NULL and with_c1 == 1 is public-key generation, pk = (e - a * s, a), for hp_dev_rlwe_encrypt_pk_seeded; the compressed
 *     form (with_c1 == 0) is pk0 plus the seed.
 * a is drawn in registers by the kernel that forms c0: it is never read from memory and, in the compressed form, never written.
 * Workspace: none when d_pt == NULL or with_c1 == 1 (NTT(pt) passes through the c1 rows); else batch * L * N words.
 *
 * hp_dev_rlwe_encrypt_pk_seeded: for ciphertext b:  u_b = the ternary sample of the id stream + 2b, e0_b = error_scale times the
 * sample of the context's error sampler of stream + 2b, e1_b = the same of stream + 2b + 1 (the kind tag keeps u_b and e0_b apart; u_b
 * is ternary whatever the error sampler), and
 *     ct0 = pk0 * NTT(u_b) + NTT(e0_b) + NTT(pt_b)        ct1 = pk1 * NTT(u_b) + NTT(e1_b)      (mod q_m)
 * The call uses the ids stream .. stream + 2 * batch - 1.  With pk = (e_pk - a * s, a) the ciphertext decrypts to pt plus
 * error_scale * (u * e_pk + e0 + e1 * s) -- pk generated with the same error_scale.  Workspace: at most 2 * batch * L * N words.
 *
 * HP_EINVAL before anything is enqueued: logn < 3 or above 16, L == 0 or L > 32, batch == 0 (not the silent HP_OK of
 * hp_dev_rlwe_encrypt_core), a modulus < 2 or >= 2^63, a NULL seed, moduli, d_sk / d_pk, d_ct or d_out, a device pointer that is not
 * 16-byte aligned, a scale that is 0 or >= 2^58, a kind outside {2, 3}, with_c1 outside {0, 1}, d_ct overlapping d_sk, d_pk or
 * d_pt.  Chains that hp_dev_ntt refuses are refused with its code.
 * Out of scope: a wire kind for seeded ciphertexts; the node, sharded and C++ host layers; CKKS encoding; discrete Gaussians of any
 * other width, or from a run-time table; kind 4 in hp_dev_sample_small_ntt; regenerating pk1 from a seed inside the public-key call. */
int hp_dev_sample_small_ntt(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch,
                            uint32_t kind /* 2 ternary, 3 centred binomial */, const uint8_t *seed /* HOST, 32 bytes */,
                            uint64_t stream, uint64_t scale, uint64_t *d_out /* u64[batch][L][N] */);
int hp_dev_rlwe_encrypt_seeded(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch,
                               const uint64_t *d_sk /* u64[L][N] NTT form, words < 2 * modulus */,
                               const uint64_t *d_pt /* u64[batch][L][N] coefficient form; NULL = zero */,
                               const uint8_t *seed, uint64_t stream, uint64_t error_scale, int with_c1,
                               uint64_t *d_ct /* with_c1: u64[batch][2][L][N]; else u64[batch][L][N] */);
int hp_dev_rlwe_encrypt_pk_seeded(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t batch,
                                  const uint64_t *d_pk /* u64[2][L][N] NTT form, words < 2 * modulus */,
                                  const uint64_t *d_pt /* as above, may be NULL */, const uint8_t *seed, uint64_t stream,
                                  uint64_t error_scale, uint64_t *d_ct /* u64[batch][2][L][N] */);
/* BGV over the hybrid key switch.  hehub's bgv::relinearize pays L*L digit transforms, carries the noise of one special prime and runs
 * its inner switch with plain modulus 1; it has no rotation.  Of the hybrid path only ModDown knows the scheme -- digits, ModUp, the
 * inner products, hoisting and the _at key addressing never see the plaintext -- so the calls below are their CKKS twins with one
 * other conversion kernel.  plain_modulus = t comes directly after moduli_ext, as in hp_dev_bgv_mult_relin_modswitch.
 *
 * The convention (pinned by tests/hks_bgv_model.py).  P = p_0...p_{k-1}; ModDown_t takes the accumulator x over the basis Q P and,
 * for every coefficient,
 *     u = ([x]_P * t^-1) mod P                        0 <= u < P
 *     c = u  if u < floor(P/2),  u - P  otherwise     (the centring of the CKKS ModDown)
 *     delta = t * c                                   delta = x mod P,  delta = 0 mod t,  |delta| <= t (P + 1) / 2
 *     ModDown_t(x) = (x - delta) / P   mod every q_i
 * NO factor (P mod t) follows: a key encrypts (P mod q_i) * s_from with error t * e, so x = P * (c1 s_from) + t E and
 * (x - delta) / P = c1 s_from (mod t) exactly.  (hehub's mod switch multiplies by q_last mod t because it divides the message
 * itself; the two mod-switch calls below end with exactly that drop.)  t = 1 gives the residues of the CKKS ModDown.
 * Keys: a BGV hybrid key is the output of hp_dev_hks_keygen / hp_dev_hks_keygen_rot, unchanged, for the error rows d_e = t * e --
 * the rows are int64_t, so t * e is one multiplication by the caller; a relinearisation key is s_from = s * s.
 * Contract as for every hybrid call: on residues, every output word below 2 q_i, parity level A follows the context; the workspace is
 * that of the CKKS call of the same shape.  Each call has its _at twin (key_L0 after L, the rule above).
 * Refused before anything is enqueued: everything the corresponding CKKS call refuses, with its code; plain_modulus == 0 or
 * plain_modulus >= any modulus of moduli_ext (HP_EINVAL: the moduli are primes, so t is then invertible everywhere); k > 8
 * (HP_EUNSUPPORTED: the conversion by one composition per modulus is not extended); L < 2 for the two mod-switch calls (HP_EINVAL).
 * Out of scope: ModDown_t merged with the mod switch into one transform (the fast path of hp_dev_ckks_mult_relin_rescale_hks stays
 * CKKS-only); BGV forms of the diagonal / BSGS transforms and of the fused dot call; the node and sharded layers; the C++ host layer,
 * which has no hybrid calls at all.
 *
 * hp_dev_bgv_hks_switch: hp_dev_hks_switch with ModDown_t.  d_pt u64[batch][L][N] -> d_out u64[batch][2][L][N], and with a key for
 * error rows t * e:  out0 + out1 * s_to = pt * s_from + t * (small)  (mod Q). */
int hp_dev_bgv_hks_switch(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                          uint64_t plain_modulus, size_t batch, const uint64_t *d_pt, const uint64_t *d_key, uint64_t *d_out);
int hp_dev_bgv_hks_switch_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext,
                             uint64_t plain_modulus, size_t batch, const uint64_t *d_pt, const uint64_t *d_key, uint64_t *d_out);
/* hp_dev_bgv_rotate_hoisted_hks: the arguments, the digit sharing, the signed-digit property and the refusals of
 * hp_dev_ckks_rotate_hoisted_hks (steps / conj / d_keys are HOST arrays): one digit stage per ciphertext, one ModDown_t per rotation;
 * a single rotation is rotations == 1.  On the BGV slots (two rows of N/2) the cycle by `step` rotates both rows, the involution
 * (conj[r] != 0) swaps them.  d_out u64[batch][rotations][2][L][N]. */
int hp_dev_bgv_rotate_hoisted_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                  uint64_t plain_modulus, size_t batch, size_t rotations, const size_t *steps, const unsigned char *conj,
                                  const uint64_t *d_ct, const uint64_t *const *d_keys, uint64_t *d_out);
int hp_dev_bgv_rotate_hoisted_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                     const uint64_t *moduli_ext, uint64_t plain_modulus, size_t batch, size_t rotations,
                                     const size_t *steps, const unsigned char *conj, const uint64_t *d_ct,
                                     const uint64_t *const *d_keys, uint64_t *d_out);
/* hp_dev_bgv_relin_modswitch_hks: d_quad u64[batch][3][L][N], words below 2q -> d_out u64[batch][2][L-1][N]: the hybrid switch of d2
 * with (d0, d1) as its addend, then hehub's mod_drop_one_prime_inplace (the drop of hp_dev_bgv_mod_switch, its q_last mod t factor
 * included).  d_quad is hp_dev_mult_low_level's, or a sum of products by hp_dev_ckks_tensor_sum -- whose arithmetic is scheme-free
 * despite its name: T products then pay one switch and one mod switch.  d_out must not overlap d_quad. */
int hp_dev_bgv_relin_modswitch_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                   uint64_t plain_modulus, size_t batch, const uint64_t *d_quad, const uint64_t *d_key, uint64_t *d_out);
int hp_dev_bgv_relin_modswitch_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                      const uint64_t *moduli_ext, uint64_t plain_modulus, size_t batch, const uint64_t *d_quad,
                                      const uint64_t *d_key, uint64_t *d_out);
/* hp_dev_bgv_mult_relin_modswitch_hks: the tensor product into a workspace quad, then the tail above: on the same operands the words
 * of hp_dev_mult_low_level followed by hp_dev_bgv_relin_modswitch_hks. */
int hp_dev_bgv_mult_relin_modswitch_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                        uint64_t plain_modulus, size_t batch, const uint64_t *d_ct1, const uint64_t *d_ct2,
                                        const uint64_t *d_key, uint64_t *d_out);
int hp_dev_bgv_mult_relin_modswitch_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha,
                                           const uint64_t *moduli_ext, uint64_t plain_modulus, size_t batch, const uint64_t *d_ct1,
                                           const uint64_t *d_ct2, const uint64_t *d_key, uint64_t *d_out);
/* BFV: the exact scale-invariant multiplication and the decryption rounding.  hehub names BFV first among its schemes and has no code
 * for it; everything around BFV's multiplication is scheme-free and already here (hp_dev_mult_low_level over any moduli list, the
 * hybrid switch with the CKKS ModDown -- BFV keys carry the error e, no factor t --, hp_dev_hks_keygen*, hp_dev_rlwe_encrypt_seeded,
 * hp_dev_rlwe_decrypt_core).  What the calls below add is the pair of EXACT base conversions with the scaling between them.
 *
 * The convention (pinned by tests/bfv_model.py).  Q = q_0...q_{L-1} is the ciphertext modulus, odd, h = (Q - 1) / 2; B = b_0...b_{M-1}
 * the auxiliary base; all L + M moduli distinct NTT primes of the ring degree; t the plain modulus, 2 <= t < every modulus.
 * moduli_qb = q_0 .. q_{L-1}, b_0 .. b_{M-1}.  A BFV ciphertext (c0, c1) is u64[batch][2][L][N] in NTT form with
 * c0 + c1 s = Delta m + e (mod Q), Delta = floor(Q / t).
 *     centre_Q(x) = x  if x < floor(Q/2),  x - Q  otherwise     (the centring of ModDown and of hp_dev_rns_base_many_to_many)
 *     lift        the integer centre_Q(x) behind the strict coefficient residues over Q, reduced into every b_j
 *     scale       for a signed integer x given by its residues over Q B:  y = floor((t x + h) / Q), rounding to nearest (Q is odd:
 *                 no ties).  v = t x + h residue-wise; r = [v]_Q in [0, Q), NOT centred, by mixed-radix composition over Q, reduced into
 *                 every b_j; y = (v - r) Q^-1 mod b_j; then centre_B(y) reduced into every q_i
 *     decryption  for x in [0, Q):  m = floor((t x + h) / Q) mod t = (h - r) Q^-1 mod t,  r = [t x + h]_Q reduced mod t  (t coprime to Q)
 * Base size: the calls with a plain modulus require B >= 4 t N Q, decided exactly in multiword integers on the host.  Every tensor
 * coefficient then has |x| <= N (Q + 1)^2 / 2, so t |x| + h < Q B / 2 and |y| < B / 2: both centrings are unambiguous.
 * A plaintext is encrypted by hp_dev_rlwe_encrypt_seeded(error_scale = 1) on the coefficient rows (Delta mod q_i) * m, which the
 * caller forms (for example with hp_dev_poly_scalar_mul); a relinearisation key is hp_dev_hks_keygen's for s_from = s * s and plain
 * error rows; decryption is hp_dev_rlwe_decrypt_core followed by hp_dev_bfv_decrypt_round.
 * Output contract of lift, scale_round, mult_low_level and decrypt_round: every word is the canonical residue (below q_m, below t),
 * one reduction after the last transform, the same word at either parity level (the transforms inside are the level-B launches).
 * mult_relin_hks[_at] have the contract of every hybrid call: on residues, words below 2 q_i, parity level A follows the context.
 * Workspace, reserved up front (E = L + M): lift polys * L * N words; scale_round polys * (E + M) * N; mult_low_level
 * batch * (10 E + 3 M) * N; mult_relin_hks that plus batch * 3 L * N plus the workspace of hp_dev_hks_switch.
 * Refused with HP_EINVAL before anything is enqueued, the output untouched: a NULL context or pointer, a misaligned pointer;
 * logn < 3 or > 16; L == 0, M == 0, polys or batch == 0; t < 2 or t >= any modulus; a modulus shared between Q and B, an even
 * modulus; B < 4 t N Q; an output overlapping an input; everything hp_dev_hks_switch[_at] refuses, with its code.  HP_EUNSUPPORTED:
 * L > 16, M > 16 or L + M > 32.  Chains that hp_dev_ntt refuses are refused with its code.
 * Out of scope: a fused plaintext-scaling call; BFV rotations (the hoisted CKKS calls serve them: the ModDown is the same); a
 * tensor-sum / dot form; modulus switching of BFV ciphertexts; the node, sharded and C++ host layers.
 *
 * hp_dev_bfv_lift: inverse transforms over Q, strict; the conversion; forward transforms over B.  The Q rows are carried over. */
int hp_dev_bfv_lift(hp_ctx *ctx, size_t logn, size_t L, size_t M, const uint64_t *moduli_qb, size_t polys,
                    const uint64_t *d_in /* u64[polys][L][N] NTT form, words < 2 * modulus */,
                    uint64_t *d_out /* u64[polys][L+M][N] NTT form */);
/* hp_dev_bfv_scale_round: inverse transforms over Q B, strict; the scaling; forward transforms over Q. */
int hp_dev_bfv_scale_round(hp_ctx *ctx, size_t logn, size_t L, size_t M, const uint64_t *moduli_qb, uint64_t t, size_t polys,
                           const uint64_t *d_in /* u64[polys][L+M][N] NTT form, words < 2 * modulus */,
                           uint64_t *d_out /* u64[polys][L][N] NTT form */);
/* hp_dev_bfv_mult_low_level: the lift of the four polynomials, hp_dev_mult_low_level's tensor product over L + M limbs into the
 * workspace, hp_dev_bfv_scale_round of the three: word for word that composition. */
int hp_dev_bfv_mult_low_level(hp_ctx *ctx, size_t logn, size_t L, size_t M, const uint64_t *moduli_qb, uint64_t t, size_t batch,
                              const uint64_t *d_ct1, const uint64_t *d_ct2, uint64_t *d_quad /* u64[batch][3][L][N] */);
/* hp_dev_bfv_mult_relin_hks: hp_dev_bfv_mult_low_level into the workspace, then hp_dev_hks_switch of y2 with (y0, y1) as its addend.
 * moduli_ext = q_0 .. q_{L-1}, p_0 .. p_{k-1}; the auxiliary base may share primes with the special primes, none with Q. */
int hp_dev_bfv_mult_relin_hks(hp_ctx *ctx, size_t logn, size_t L, size_t k, size_t alpha, const uint64_t *moduli_ext, size_t M,
                              const uint64_t *aux_moduli, uint64_t t, size_t batch, const uint64_t *d_ct1, const uint64_t *d_ct2,
                              const uint64_t *d_key, uint64_t *d_out /* u64[batch][2][L][N] */);
int hp_dev_bfv_mult_relin_hks_at(hp_ctx *ctx, size_t logn, size_t L, size_t key_L0, size_t k, size_t alpha, const uint64_t *moduli_ext,
                                 size_t M, const uint64_t *aux_moduli, uint64_t t, size_t batch, const uint64_t *d_ct1,
                                 const uint64_t *d_ct2, const uint64_t *d_key, uint64_t *d_out);
/* hp_dev_bfv_decrypt_round: n = N (a power of two, 8 .. 65536); t only has to be coprime to Q. */
int hp_dev_bfv_decrypt_round(hp_ctx *ctx, size_t n, size_t L, const uint64_t *moduli, uint64_t t, size_t polys,
                             const uint64_t *d_x /* u64[polys][L][N] strict coefficient form */, uint64_t *d_m /* u64[polys][N], words < t */);
/* ct u64[batch][2][L][N] -> out u64[batch][2][L-drops][N]; d_tmp: 2 * batch*2*(L-1)*N words (may be NULL for drops == 1) */
int hp_dev_ckks_rescale_n(hp_ctx *ctx, size_t logn, size_t L, const uint64_t *moduli, size_t drops, size_t batch,
                          const uint64_t *d_ct, uint64_t *d_tmp, uint64_t *d_out);

/* ---- wire / on-disk format (hehub itself has none) -------------------------------------
 * "HEHUBAMD" header + moduli + the words in device order + FNV-1a-64 trailer; the exact byte layout is documented in
 * hehub_amd/csrc/hp_wire.cpp.  Loading a key or ciphertext is one validation pass and one host-to-device copy. */
typedef enum { HP_WIRE_POLY = 1, HP_WIRE_CT = 2, HP_WIRE_QUAD_CT = 3, HP_WIRE_KSK = 4 } hp_wire_kind;
typedef struct {
    uint32_t kind;           /* hp_wire_kind */
    uint32_t log_dimension;  /* log2 N */
    uint32_t limbs;          /* limbs per polynomial (a key: L+1) */
    uint32_t polys;          /* 1, 2, 3; a key: 2*digits, rgsw[j][half] digit-major */
    uint32_t rep_form;       /* 0 coefficient, 1 NTT value */
    uint64_t scheme_scalar;  /* IEEE-754 bits of the CKKS scaling factor / BGV plain modulus / 0 */
} hp_wire_desc;
/* the format's checksum: FNV-1a-64 over `bytes` bytes (little-endian words as they lie in memory) */
uint64_t hp_wire_fnv1a64(const void *data, size_t bytes);
size_t hp_wire_payload_words(const hp_wire_desc *d);   /* 0 for an invalid descriptor */
size_t hp_wire_bytes(const hp_wire_desc *d);
/* host words -> buffer, and back (payload_offset: where the words start inside buf) */
int hp_wire_pack(const hp_wire_desc *d, const uint64_t *moduli, const uint64_t *words, void *buf, size_t cap);
int hp_wire_unpack(const void *buf, size_t len, hp_wire_desc *d, uint64_t *moduli, size_t moduli_cap,
                   size_t *payload_offset);
/* buffer -> device words (validated: magic, version, sizes, checksum), device words -> buffer */
int hp_dev_wire_load(hp_ctx *ctx, const void *buf, size_t len, uint64_t *d_words);
int hp_dev_wire_store(hp_ctx *ctx, const hp_wire_desc *d, const uint64_t *moduli, const uint64_t *d_words, void *buf,
                      size_t cap);

/* ---- in-library kernel timing (HIP events on the ctx stream) -------------- */
/* Between hp_prof_begin and hp_prof_end every kernel launch of the named
 * family is bracketed by hipEvents on the stream it is launched on.
 * hp_prof_end synchronises and returns launches and total milliseconds. */
int hp_prof_begin(hp_ctx *ctx, const char *kernel_family);
int hp_prof_end(hp_ctx *ctx, size_t *launches, double *total_ms);
/* With the family "*" every launch of every family is bracketed; this returns the totals per family (at most `cap` of them, in
 * order of first appearance): names[i] is a static string ("tensor", "intt", "ntt", "ks_inner", "ntt_drop", "elem", "copy", ...). */
int hp_prof_end_families(hp_ctx *ctx, size_t cap, const char **names, size_t *launches, double *total_ms, size_t *count);

#ifdef __cplusplus
}
#endif
#endif
