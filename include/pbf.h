/*
 * pbf.h — C-ABI of the MI355X-native PLONK hot path (libpbf.so, gfx950).
 *
 * Drop-in boundary for adria0/plonk-by-fingers (Rust). The reference has no FFI;
 * every entry point below replaces one of its trait methods / free functions and
 * cites it as file:line relative to the reference root. A Rust caller binds these
 * with an `extern "C"` block; here they are exercised from C++
 * and from Python (ctypes) tests.
 *
 * Conventions:
 *   - Field elements cross the ABI canonical, in [0, modulus), one uint64_t each
 *     (the reference's U64Field<M> is one u64, u64field.rs:27-28). 256-bit
 *     elements are 4 x uint64_t little-endian limbs, canonical (never Montgomery).
 *   - Vectors are natural order (fft.rs:98-104 writes o[i] / o[i+len/2]).
 *   - Host-pointer entry points are synchronous: copy in, compute, copy out, on
 *     the context's host stream. `_dev` entry points take device pointers and a
 *     hipStream_t (void*) and are stream-ordered on that stream (NULL = the HIP null
 *     stream, as everywhere in HIP): their work starts after everything enqueued on
 *     it before the call and finishes before anything enqueued after. Two entry points
 *     also use streams private to the context, always joined back by events (waits in
 *     the command processor, never a spinning kernel) on the caller's stream before
 *     they return: a batched Goldilocks NTT of >= 8 polynomials
 *     (pbf_ntt_u64_batch_dev, pbf_ntt_u64_coset_batch_dev) forks half its groups onto a
 *     second stream, and the
 *     fixed-base MSM (pbf_msm_g1_bn254_fixed_dev, and the commitments inside
 *     pbf_plonk_prove_bn254*) runs its bucket join and reduction on a side stream while
 *     the caller's stream goes on; the fixed-base MSM, prove and verify order the
 *     caller's stream after that side stream (an event wait) before returning. Nothing
 *     else is ever enqueued on streams the caller did not pass.
 *   - Input and output may alias (in-place is allowed).
 *   - Supported moduli for the u64 entry points: Goldilocks p = 2^64-2^32+1, and any
 *     odd M < 2^32 (the range where the reference's `(a*b)%M` in u64 is exact,
 *     u64field.rs:177).
 *   - Errors are returned, never aborted on. pbf_last_error() gives the text.
 *   - One pbf_ctx per host thread; distinct contexts are independent (no shared
 *     streams, buffers or caches; every entry point selects the context's device).
 */
#ifndef PBF_H
#define PBF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum pbf_status {
  PBF_OK = 0,
  PBF_EINVAL = 1,      /* bad size / not a power of two / omega order != n / non-canonical input */
  PBF_ENOINV = 2,      /* n has no inverse mod M: the reference panics at fft.rs:73 `.unwrap()` */
  PBF_EDEVICE = 3,     /* HIP error (allocation, launch, copy) */
  PBF_ECOMM = 4,       /* RCCL / multi-GPU exchange error */
  PBF_EUNSUPPORTED = 5 /* modulus outside the supported set */
};

typedef struct pbf_ctx pbf_ctx;

/* ---- context ------------------------------------------------------------ */
/* Owns the device, a stream, twiddle tables (cached per (modulus, omega, n)) and
 * scratch buffers. Replaces nothing in the reference (its types are plain values). */
int pbf_ctx_create(int device, pbf_ctx** out);
void pbf_ctx_destroy(pbf_ctx* ctx);
const char* pbf_last_error(void);
/* Stream used by the synchronous host-pointer entry points (default: a private
 * non-blocking stream created with the context). `_dev` calls ignore it.     */
int pbf_ctx_set_stream(pbf_ctx* ctx, void* stream);
/* Context options: select among product code paths of this context (never read from the
 * environment). `value` NULL removes the option; unknown names return PBF_EINVAL. Every
 * option gives the same results, bit for bit; they exist for cross-checks and tuning:
 *   ntt.passes     "a,b,..."  radix bits per pass of u64 NTT plans (each 6..12, sum log2 n)
 *   ntt.group      G          polynomials per group of a batched Goldilocks NTT (0: one group)
 *   ntt.streams    k          streams the groups rotate over (1: the caller's stream only)
 *   ntt.twmax_log  L          per-pass twiddle tables up to 2^L entries (default 24)
 *   ntt.twsplit    1 / 0      last pass: force the split table / keep the two-level table
 *   ntt.no_rg      1          2^24: the round-2 passes instead of the regrouped plan
 *   ntt256.maxr    4..9       largest radix (bits) of the 256-bit NTT passes (default 9)
 *   ntt256.twlog   L          256-bit per-pass twiddle tables up to 2^L entries (default 26)
 *   ntt256.l29     0          256-bit NTT passes and the prover's quotient kernel on 8 x 32-bit
 *                             limbs instead of nine 29-bit ones
 *   msm.fx_c       16/20/22   fixed-base MSM window bits (default by size)
 *   g1ntt.tile_log 6..20      G1 NTT: 2^L twiddle products per launch, each with 15 x 128 B of
 *                             window table (default 14: 30 MiB)
 *   g1.mul_base    "daa"      G1 fixed-base products by double-and-add instead of the comb
 *   pair.engine    "lane"/"wg" pairing engine (default: lanes from 4096 pairings)
 *   pair.lane_wpe  1 / 2      lane engine built for 1 or 2 waves per SIMD (default by size)
 *   prover.pk      0          no proving-key cache: every proof recomputes the preprocessed
 *                             polynomials, as the reference does (plonk.rs:233-243, 339-370)
 *   prover.timing  1          synchronise at every prover round mark (per-round times)
 *   verifier.vk    0          no verification-key cache
 *   recover.timing 1          synchronise at every stage mark of the recovery from cells and print
 *                             the stage's time on stderr (per-stage times)
 * Options are read when used; an ntt* option also drops the context's cached NTT plans (after a
 * device synchronisation), which are rebuilt under the new value. */
int pbf_ctx_set_option(pbf_ctx* ctx, const char* name, const char* value);
int pbf_device_sync(pbf_ctx* ctx);
/* Frees the context's derived caches -- the prover's proving key, the verifier's
 * verification key, the fixed-base MSM window table, the pairing check's prepared lines
 * and the device copies that validate them -- after waiting for the context's streams.
 * The next call that needs one rebuilds it. Plans and scratch buffers stay.   */
int pbf_ctx_release_caches(pbf_ctx* ctx);

/* ---- FFT trait ------------------------------------------------------------ */
/* CooleyTurkey::new(EvaluationDomainGenerator{omega, size: n}) + fft / fft_inv
 * (fft.rs:6-21, 55-78). out[k] = sum_j in[j] * omega^(j*k)           (inverse = 0)
 *                       out[j] = n^-1 * sum_k in[k] * omega^(-j*k)    (inverse = 1)
 * omega must have multiplicative order exactly n (the reference assumes it).   */
int pbf_ntt_u64(pbf_ctx* ctx, uint64_t modulus, uint64_t omega, const uint64_t* in, uint64_t* out,
                size_t n, int inverse);
/* Device-pointer, batched: `batch` independent transforms, polynomial b at
 * d_in + b*n. Inputs must already be canonical (not checked on this path).   */
int pbf_ntt_u64_batch_dev(pbf_ctx* ctx, uint64_t modulus, uint64_t omega, const uint64_t* d_in,
                          uint64_t* d_out, size_t n, size_t batch, int inverse, void* stream);

/* ---- coset NTT / low-degree extension ------------------------------------------
 * The same transform on the coset shift * <omega> (the reference has none; its quotient,
 * plonk.rs:339-370, is the caller that would want one: SURVEY.md §8(f)). modulus, omega and n
 * as for pbf_ntt_u64 (omega of order exactly n).
 *   inverse = 0: polynomial b is the in_len coefficients at in + b*in_len, compact, with
 *     1 <= in_len <= n (any value: n/4 + 3 is legal), and
 *       out[b*n + k] = sum_{j < in_len} in[b*in_len + j] * (shift * omega^k)^j,   natural order:
 *     the low-degree extension with blow-up n / in_len. The zero padding is never stored or read.
 *   inverse = 1: needs in_len == n (else PBF_EINVAL);
 *       out[j] = shift^-j * n^-1 * sum_k in[k] * omega^(-j*k),
 *     so inverse(forward(a)) == a bit for bit.
 * shift must be canonical and non-zero; shift = 1 gives exactly pbf_ntt_u64*. shift = 0,
 * shift >= modulus, in_len = 0 and in_len > n return PBF_EINVAL before anything is enqueued.
 * Input and output may alias only when in_len == n. The host entry point checks its input
 * canonical as pbf_ntt_u64 does. The _dev entry point follows the stream contract above; a
 * batch of >= 8 Goldilocks polynomials forks half its groups onto the context's second stream,
 * joined back by events before it returns, like pbf_ntt_u64_batch_dev. Standard-root
 * Goldilocks transforms of n > 4096 apply the factors inside their first pass's loads
 * (forward) or last pass's stores (inverse): no extra kernel or pass over the data. The
 * context keeps the factor tables of the last 4 shifts used with each (modulus, omega, n,
 * direction).                                                                            */
int pbf_ntt_u64_coset(pbf_ctx* ctx, uint64_t modulus, uint64_t omega, uint64_t shift, const uint64_t* in,
                      size_t in_len, uint64_t* out, size_t n, int inverse);
int pbf_ntt_u64_coset_batch_dev(pbf_ctx* ctx, uint64_t modulus, uint64_t omega, uint64_t shift,
                                const uint64_t* d_in, size_t in_len, uint64_t* d_out, size_t n, size_t batch,
                                int inverse, void* stream);

/* ---- mul_ntt ---------------------------------------------------------------- */
/* fft.rs:109-132: zero-pad a (la) and b (lb) to la+lb (= the domain size, a power
 * of two), forward NTT both, multiply pointwise, inverse NTT. out has la+lb entries
 * and is NOT normalised (the reference's caller wraps it in Poly::new, fft.rs:180). */
int pbf_mul_ntt_u64(pbf_ctx* ctx, uint64_t modulus, uint64_t omega, const uint64_t* a, size_t la,
                    const uint64_t* b, size_t lb, uint64_t* out);

/* ---- Poly ------------------------------------------------------------------- */
/* Poly::eval (poly.rs:71-79) at nx points: ys[i] = sum_j coeffs[j] * xs[i]^j. */
int pbf_poly_eval_u64(pbf_ctx* ctx, uint64_t modulus, const uint64_t* coeffs, size_t n,
                      const uint64_t* xs, size_t nx, uint64_t* ys);

/* ---- Poly arithmetic (poly.rs:165-247) -----------------------------------------------
 * Results normalised as Poly::normalize (poly.rs:96-105): trailing zeros stripped, at least
 * one coefficient; *lout / *lq / *lr receive the lengths. Inputs: >= 1 coefficient each.
 * pbf_poly_add_u64 / pbf_poly_sub_u64: AddAssign / SubAssign<&Poly> (poly.rs:165-176,
 *   192-203); `out` holds max(la, lb). Subtraction keeps the reference's quirk: where only
 *   b has a coefficient it is appended as +b[i] (poly.rs:196).
 * pbf_poly_div_u64: Div for Poly (poly.rs:230-247), num = q * den + r, deg r < deg den,
 *   computed in O(n log n) (reversed-series inverse by Newton's iteration, NTT products);
 *   `root` has multiplicative order 2^root_log and bounds the NTT sizes (Goldilocks:
 *   7^((p-1)/2^32), 32). q holds >= nn, r >= nn coefficients. PBF_ENOINV when the divisor's
 *   leading coefficient has no inverse (the reference's unwrap at poly.rs:238).         */
int pbf_poly_add_u64(pbf_ctx* ctx, uint64_t modulus, const uint64_t* a, size_t la, const uint64_t* b, size_t lb,
                     uint64_t* out, size_t* lout);
int pbf_poly_sub_u64(pbf_ctx* ctx, uint64_t modulus, const uint64_t* a, size_t la, const uint64_t* b, size_t lb,
                     uint64_t* out, size_t* lout);
int pbf_poly_div_u64(pbf_ctx* ctx, uint64_t modulus, uint64_t root, uint32_t root_log, const uint64_t* num,
                     size_t nn, const uint64_t* den, size_t nd, uint64_t* q, size_t* lq, uint64_t* r, size_t* lr);

/* ---- multi-GPU stride-sharded NTT ---------------------------
 * A transform of N = G * nl points (G = world size 2, 4 or 8; omega of order N) is
 * sharded by coefficient stride: rank g holds a[g + G*m], m < nl, for `batch`
 * polynomials ([b][m] layout). This is the top log2(G) levels of the reference's
 * even/odd recursion (fft.rs:94-96) assigned to ranks. Forward on every rank:
 *   pbf_ntt_shard_local_dev(fwd):  [b][m] stride shard -> send [dst][b][kk]   (S = nl/G)
 *   all-to-all (RCCL, nl*batch/G elements per peer): send -> recv [src][b][kk]
 *   pbf_ntt_shard_combine_dev(fwd): recv -> out[b][q*S + kk] = X[q*nl + rank*S + kk]
 * Inverse runs the same steps backwards with the same omega:
 *   combine(inv): out-layout X -> send [dst][b][kk]; all-to-all; local(inv): recv -> [b][m]
 * and returns the stride shard a[g + G*m] (scaled by N^-1 overall).                  */
int pbf_ntt_shard_local_dev(pbf_ctx* ctx, uint64_t modulus, uint64_t omega, uint32_t world,
                            const uint64_t* d_in, uint64_t* d_out, size_t nl, size_t batch, int inverse,
                            void* stream);
int pbf_ntt_shard_combine_dev(pbf_ctx* ctx, uint64_t modulus, uint64_t omega, uint32_t world,
                              uint32_t rank, const uint64_t* d_in, uint64_t* d_out, size_t nl,
                              size_t batch, int inverse, void* stream);

/* c[i] = a[i] * b[i] for `count` elements (the pointwise step of mul_ntt, fft.rs:125-129;
 * the sharded mul_ntt multiplies its blocks with it)                                  */
int pbf_pointwise_mul_u64_dev(pbf_ctx* ctx, uint64_t modulus, const uint64_t* d_a, const uint64_t* d_b,
                              uint64_t* d_c, size_t count, void* stream);

/* ---- BN254 scalar field (BASELINE config 3) ----------------------------------
 * r = 21888242871839275222246405745257275088548364400416034343698204186575808495617,
 * elements 4 x uint64_t little-endian, canonical; n a power of two <= 2^28.
 * The reference has no 256-bit field: these are fft.rs:66-78 and fft.rs:109-132
 * instantiated for the field SURVEY.md §0.5 picks for configs 3-5.              */
int pbf_ntt_fr256(pbf_ctx* ctx, const uint64_t* omega, const uint64_t* in, uint64_t* out, size_t n,
                  int inverse);
int pbf_ntt_fr256_batch_dev(pbf_ctx* ctx, const uint64_t* omega, const uint64_t* d_in, uint64_t* d_out,
                            size_t n, size_t batch, int inverse, void* stream);
/* pbf_ntt_u64_coset* for Fr (shift: 4 x u64, canonical, non-zero): the same semantics, argument
 * checks and aliasing rule; elements 4 x u64. A scaling kernel runs before the forward transform
 * (which reads no zero padding) or after the inverse one.                                    */
int pbf_ntt_fr256_coset(pbf_ctx* ctx, const uint64_t* omega, const uint64_t* shift, const uint64_t* in,
                        size_t in_len, uint64_t* out, size_t n, int inverse);
int pbf_ntt_fr256_coset_batch_dev(pbf_ctx* ctx, const uint64_t* omega, const uint64_t* shift, const uint64_t* d_in,
                                  size_t in_len, uint64_t* d_out, size_t n, size_t batch, int inverse, void* stream);
int pbf_mul_ntt_fr256(pbf_ctx* ctx, const uint64_t* omega, const uint64_t* a, size_t la,
                      const uint64_t* b, size_t lb, uint64_t* out);
/* batched device mul_ntt: a, b already zero-padded to n = la + lb; out = batch x n  */
int pbf_mul_ntt_fr256_dev(pbf_ctx* ctx, const uint64_t* omega, const uint64_t* d_a, const uint64_t* d_b,
                          uint64_t* d_out, size_t n, size_t batch, void* stream);

/* Stride-sharded Fr NTT across G GPUs: pbf_ntt_shard_local_dev / _combine_dev (above) for
 * 256-bit elements (omega: 4 x u64, order G*nl). Same layouts, 4 x u64 per element.     */
int pbf_ntt_fr256_shard_local_dev(pbf_ctx* ctx, const uint64_t* omega, uint32_t world, const uint64_t* d_in,
                                  uint64_t* d_out, size_t nl, size_t batch, int inverse, void* stream);
int pbf_ntt_fr256_shard_combine_dev(pbf_ctx* ctx, const uint64_t* omega, uint32_t world, uint32_t rank,
                                    const uint64_t* d_in, uint64_t* d_out, size_t nl, size_t batch, int inverse,
                                    void* stream);
/* c[i] = a[i] * b[i] over Fr (canonical in and out)                                      */
int pbf_pointwise_mul_fr256_dev(pbf_ctx* ctx, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c,
                                size_t count, void* stream);

/* ---- BN254 G1 MSM / SRS (BASELINE config 4) -----------------------------------
 * Points: affine, 8 x uint64_t (x then y, each 4 little-endian limbs, canonical in Fq);
 * (0, 0) encodes the identity. Scalars: Fr canonical, 4 x uint64_t.              */
/* SRS::eval_at_s (plonk.rs:51-58): out = sum_i scalars[i] * points[i]               */
int pbf_msm_g1_bn254(pbf_ctx* ctx, const uint64_t* points, const uint64_t* scalars, size_t n,
                     uint64_t* out);
int pbf_msm_g1_bn254_dev(pbf_ctx* ctx, const uint64_t* d_points, const uint64_t* d_scalars, size_t n,
                         uint64_t* out, void* stream);
/* The same sum against a FIXED base set (KZG commitments: the SRS): out = sum_{i<n}
 * scalars[i] * points[i], n <= n_points. The first call for a base set precomputes its
 * window table 2^(16w) P_i (16 x n_points affine points, cached in the context with a
 * device copy of the points it was built from, and revalidated against that copy word for
 * word on every call, so rewriting the points in place is safe); then every (point,
 * window) digit shares one set of 2^15 buckets.                                           */
int pbf_msm_g1_bn254_fixed_dev(pbf_ctx* ctx, const uint64_t* d_points, size_t n_points, const uint64_t* d_scalars,
                               size_t n, uint64_t* out, void* stream);
/* The same against points [first, first + n) of the fixed base set: out = sum_{i<n}
 * scalars[i] * points[first + i] (one rank's point range of a sharded commitment; the
 * window table still covers all n_points and is shared with the call above).               */
int pbf_msm_g1_bn254_fixed_range_dev(pbf_ctx* ctx, const uint64_t* d_points, size_t n_points, size_t first,
                                     const uint64_t* d_scalars, size_t n, uint64_t* out, void* stream);
/* out_i = scalars_i * G (G = (1, 2)), device pointers                               */
int pbf_g1_bn254_mul_base_dev(pbf_ctx* ctx, const uint64_t* d_scalars, uint64_t* d_out, size_t n,
                              void* stream);
/* SRS::create (plonk.rs:35-48): out = [G, G*s, ..., G*s^n] (n+1 points)             */
int pbf_srs_create_bn254(pbf_ctx* ctx, const uint64_t* s, size_t n, uint64_t* out);

/* ---- BN254 pairing (BASELINE config 4 "pairing check") ------------------------
 * The BN254 instance of Pairing::pairing (src/ec.rs:87-93; the reference's own is the
 * toy reduced Tate pairing, src/pbh/pairing.rs:12-47) as Plonk::verify uses it
 * (src/plonk.rs:646-647): optimal ate, e(P, Q) = f_{6u+2,Q}(P)...^((q^12-1)/r).
 * G1: 8 x uint64_t affine (as above). G2: 16 x uint64_t affine on the twist
 * y^2 = x^3 + 3/(9+u) over Fq2 = Fq[u]/(u^2+1): x.c0, x.c1, y.c0, y.c1 (4 limbs each),
 * all zero = identity. GT: 48 x uint64_t = 12 Fq in the tower order of
 * Fq12 = Fq6[w]/(w^2-v), Fq6 = Fq2[v]/(v^3-(9+u)): c0.a0, c0.a1, c0.a2, c1.a0, c1.a1,
 * c1.a2 (each Fq2 as c0, c1). Inputs must be subgroup points (not checked; coordinates
 * are checked canonical, else PBF_EINVAL).                                             */
int pbf_pairing_bn254(pbf_ctx* ctx, const uint64_t* g1, const uint64_t* g2, size_t n, uint64_t* out);
int pbf_pairing_bn254_dev(pbf_ctx* ctx, const uint64_t* d_g1, const uint64_t* d_g2, size_t n, uint64_t* d_out,
                          void* stream);
/* *ok = (prod_i e(g1_i, g2_i) == 1): n Miller loops, one shared final exponentiation.
 * The KZG opening check of Plonk::verify (plonk.rs:646-650) is n = 2:
 * e(W, [s]G2) * e(-(C - y G + z W), G2) == 1.                                          */
int pbf_pairing_check_bn254(pbf_ctx* ctx, const uint64_t* g1, const uint64_t* g2, size_t n, int* ok);
/* out_i = scalars_i * pts_i on the twist (G2P::mul, src/pbh/g2.rs:82-101): SRS [s]G2  */
int pbf_g2_bn254_mul(pbf_ctx* ctx, const uint64_t* pts, const uint64_t* scalars, size_t n, uint64_t* out);

/* ---- Generalised PLONK prover / verifier over BN254 (BASELINE config 5) ---------
 * Plonk::prove / Plonk::verify (src/plonk.rs:191-650) for n = 2^k >= 8 gates with
 * HF = GF = Fr, G1/G2 of BN254 and the pairing above; t(x) split into three parts of
 * n+2 coefficients (plonk.rs:376-378 generalised). Field elements canonical 4 x u64.
 *   q:      5 x n x 4   (columns q_l, q_r, q_o, q_m, q_c)
 *   copies: 3 x n x 2   (columns c_a, c_b, c_c; per wire (kind 0=A 1=B 2=C, 1-based index))
 *   abc:    3 x n x 4   (witness columns a, b, c)
 *   chal:   5 x 4       (alpha, beta, gamma, z, v)      rnd: 9 x 4 (b1..b9)
 *   k1k2:   2 x 4       (PlonkTypes::K1, K2: cosets k1 H, k2 H, plonk.rs:133-139)
 *   srs:    srs_m x 8   affine G1 [G, sG, s^2 G, ...] (SRS::create); prove needs
 *           srs_m >= 2n+2 in mode 0, >= n+3 in mode 1; verify >= n. g2: [G2, [s]G2].
 *   out_pts 9 x 8: a_s b_s c_s z_s t_lo_s t_mid_s t_hi_s w_z_s w_zw_s
 *   out_f   7 x 4: a_z b_z c_z s_sigma_1_z s_sigma_2_z r_z z_omega_z   (Proof, plonk.rs:61-95)
 * mode 0 = the reference's formulas (r_3(x) of plonk.rs:414-416; verifier step 7 of
 * plonk.rs:575-581), mode 1 = the paper linearisation the verifier checks (SURVEY §0.7:
 * with mode 0 an honest proof verifies only when (a_z+b*s1_z+g)(b_z+b*s2_z+g)*alpha = 0,
 * as in the reference's n = 4 KAT).
 * Errors: PBF_EINVAL for an unsatisfied circuit (constraints.rs:198), a zero permutation
 * denominator (plonk.rs:297), a non-divisible quotient (plonk.rs:370), short SRS.
 * Keys: the context keeps the circuit's preprocessed polynomials (q_*, s_sigma_*, l1:
 * 8 coefficient slots of n+8 and 9 coset slots of 4n (of 4n/world when sharded) Fr
 * elements, ~1.4 KiB per gate, ~23.6 GB at 2^24 gates on one GPU) and the verifier's 8
 * preprocessed commitments, plus device copies of the q / copies (and, for verify, SRS)
 * arrays they were built from (~0.2 KiB per gate each); every call compares its inputs
 * with those copies word for word and rebuilds on any difference. Outputs are identical
 * either way; the context options prover.pk = 0 / verifier.vk = 0 (pbf_ctx_set_option)
 * disable the keys, and pbf_ctx_release_caches frees them (and the MSM window table)
 * between circuits.                                                                     */
int pbf_plonk_prove_bn254(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies, const uint64_t* abc,
                          const uint64_t* chal, const uint64_t* rnd, const uint64_t* k1k2, const uint64_t* srs,
                          size_t srs_m, int mode, uint64_t* out_pts, uint64_t* out_f);
int pbf_plonk_prove_bn254_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                              const uint64_t* d_abc, const uint64_t* chal, const uint64_t* rnd, const uint64_t* k1k2,
                              const uint64_t* d_srs, size_t srs_m, int mode, uint64_t* out_pts, uint64_t* out_f,
                              void* stream);
int pbf_plonk_verify_bn254(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies, const uint64_t* srs,
                           size_t srs_m, const uint64_t* g2, const uint64_t* proof_pts, const uint64_t* proof_f,
                           const uint64_t* chal, const uint64_t* u, const uint64_t* k1k2, int mode, int* ok);
int pbf_plonk_verify_bn254_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                               const uint64_t* d_srs, size_t srs_m, const uint64_t* g2, const uint64_t* proof_pts,
                               const uint64_t* proof_f, const uint64_t* chal, const uint64_t* u, const uint64_t* k1k2,
                               int mode, int* ok, void* stream);

/* Batched Plonk::verify: `count` proofs of ONE circuit and SRS, one 2-pair pairing check.
 * Per proof i the single verifier checks e(E1_i, [s]G2) == e(E2_i, G2) with
 * E1_i = W_z,i + u_i W_zw,i and E2_i the 18-term combination of the proof's points, the
 * circuit's 8 preprocessed commitments and G. The batch checks the random linear combination
 *     e(sum_i rho_i E1_i, [s]G2) * e(-sum_i rho_i E2_i, G2) == 1
 * as one MSM over 9 count + 9 points, one over 2 count points and one pairing check, whatever
 * `count` is. Arrays are proof-major, host pointers in both forms (as the single verifier
 * takes its proof): proof_pts count x 9 x 8, proof_f count x 7 x 4, chal count x 5 x 4
 * (alpha beta gamma z v per proof), u count x 4, rho count x 4. The circuit, SRS, g2, k1k2,
 * mode, the stream contract, the verification-key cache and option verifier.vk are those of
 * pbf_plonk_verify_bn254 / _dev.
 * Randomness: the library reads none. In this form soundness rests on the caller choosing the
 * weights rho unpredictably and AFTER seeing the proofs; with predictable or equal weights the
 * errors of two bad proofs can cancel and the batch passes. rho_0 = 1 is fine; 128-bit weights are
 * enough. pbf_plonk_verify_bn254_batch_fs ("Fiat-Shamir" below) takes no rho: it derives the
 * weights, with chal and u, by hashing all the proofs on the device.
 * Result: a proof is rejected outright when one of its 9 points is not canonical or not on the
 * curve ((0,0) is accepted), one of its 7 fields is >= r, or Z_H(z_i) = 0 -- the single
 * verifier's ok = 0 cases. *ok = 1 iff no proof is rejected and the combined check passes.
 * ok_each (count ints, or NULL): rejected proofs get 0; if the combined check over the others
 * passes they all get 1; if not, the index range is halved recursively down to single proofs
 * (a one-proof range is the single verifier's equation times rho_i != 0), reusing the
 * per-proof scalars on the device: each range costs its two MSMs and one pairing check. With
 * NULL no localisation runs.
 * Errors (PBF_EINVAL, before anything is enqueued): count = 0 or > 2^20, a rho_i that is zero
 * or >= r, and every error of the single verifier (NULL arguments, bad n, short SRS). chal
 * and u are taken as the single verifier takes them: any 256-bit value, reduced mod r.      */
int pbf_plonk_verify_bn254_batch(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                 const uint64_t* srs, size_t srs_m, const uint64_t* g2, size_t count,
                                 const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* chal,
                                 const uint64_t* u, const uint64_t* rho, const uint64_t* k1k2, int mode, int* ok,
                                 int* ok_each);
int pbf_plonk_verify_bn254_batch_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                     const uint64_t* d_srs, size_t srs_m, const uint64_t* g2, size_t count,
                                     const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* chal,
                                     const uint64_t* u, const uint64_t* rho, const uint64_t* k1k2, int mode, int* ok,
                                     int* ok_each, void* stream);

/* Public inputs: one circuit, many statements. Public input i < npub <= n sits on gate row i:
 * with PI(w^i) = -pub_i for i < npub, 0 on the other rows of H, and PI(x) its interpolation
 * (degree < n), the gate equation is
 *     q_l a + q_r b + q_o c + q_m a b + q_c + PI = 0   on H,
 * whatever the row's selectors are (the classic public row is q_l = 1, a_i = pub_i). PI(x) enters
 * the quotient's gate term t_1 (plonk.rs:339-344) and the verifier's step 7 only,
 *     t_z = (r_z + PI(z) - perm - L_1(z) alpha^2) / Z_H(z),
 *     PI(z) = -(z^n - 1)/n * sum_{i<npub} pub_i w^i / (z - w^i);
 * r(x) keeps q_c(x) and gains no PI term in either mode, so r_z and the opening batching are as
 * without public inputs and the t parts and W_z are those of the new t(x).
 *   pub: npub x 4 u64, canonical. Prover: a device pointer in the _dev form (like d_abc), a host
 *   pointer in the host form. Verifiers: a host pointer in both forms (as the proof is); the batch
 *   takes count x npub x 4, proof-major and compact, one npub per batch (it is a property of the
 *   circuit). Every other argument, the stream contract, the keys and the options are those of the
 *   entry point without _pi.
 * Contract:
 *   - npub = 0 (pub may then be NULL) is the entry point without _pi: the same launches, bit for
 *     bit the same output.
 *   - npub > n, a pub value >= r, or NULL pub with npub > 0 give PBF_EINVAL before anything is
 *     enqueued, in prover and verifiers alike (pbf_plonk_prove_bn254_pi_dev, whose pub is on the
 *     device, finds a value >= r in its first kernel, the constraint check, before any other
 *     work). Public inputs are the caller's statement, not part of a proof, so they are never a
 *     reason for ok = 0.
 *   - a witness that does not meet the gate equation including -pub_i gives the "constraints not
 *     satisfied" PBF_EINVAL (the pre-check keeps the reference's form, its q_l * b term included).
 *   - the proving and verification keys do not depend on pub: changing pub between calls rebuilds
 *     nothing. The prover forms q_c(x) + PI(x) on the coset in per-proof scratch it already owns
 *     (one INTT of n and one coset NTT of 4n per proof; no added buffer); the key's q_c slot is
 *     never written, and a _pi call does not alter what a later plain call returns on the context.
 *   - Soundness: these entries derive no challenge, so the caller's transcript must absorb pub
 *     before beta; the _fs forms ("Fiat-Shamir" below) do, and theirs does.
 *   - the sharded and _multi provers take no public inputs.                                      */
int pbf_plonk_prove_bn254_pi(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies, const uint64_t* abc,
                             const uint64_t* pub, size_t npub, const uint64_t* chal, const uint64_t* rnd,
                             const uint64_t* k1k2, const uint64_t* srs, size_t srs_m, int mode, uint64_t* out_pts,
                             uint64_t* out_f);
int pbf_plonk_prove_bn254_pi_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                 const uint64_t* d_abc, const uint64_t* d_pub, size_t npub, const uint64_t* chal,
                                 const uint64_t* rnd, const uint64_t* k1k2, const uint64_t* d_srs, size_t srs_m,
                                 int mode, uint64_t* out_pts, uint64_t* out_f, void* stream);
int pbf_plonk_verify_bn254_pi(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies, const uint64_t* srs,
                              size_t srs_m, const uint64_t* g2, const uint64_t* proof_pts, const uint64_t* proof_f,
                              const uint64_t* pub, size_t npub, const uint64_t* chal, const uint64_t* u,
                              const uint64_t* k1k2, int mode, int* ok);
int pbf_plonk_verify_bn254_pi_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                  const uint64_t* d_srs, size_t srs_m, const uint64_t* g2, const uint64_t* proof_pts,
                                  const uint64_t* proof_f, const uint64_t* pub, size_t npub, const uint64_t* chal,
                                  const uint64_t* u, const uint64_t* k1k2, int mode, int* ok, void* stream);
/* PI_i(z_i) of all `count` proofs comes from one kernel pair (partial fractions per chunk of 256
 * public inputs and proof, then one fraction per proof), once per call; localisation reuses it. */
int pbf_plonk_verify_bn254_batch_pi(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                    const uint64_t* srs, size_t srs_m, const uint64_t* g2, size_t count,
                                    const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* pub,
                                    size_t npub, const uint64_t* chal, const uint64_t* u, const uint64_t* rho,
                                    const uint64_t* k1k2, int mode, int* ok, int* ok_each);
int pbf_plonk_verify_bn254_batch_pi_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                        const uint64_t* d_srs, size_t srs_m, const uint64_t* g2, size_t count,
                                        const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* pub,
                                        size_t npub, const uint64_t* chal, const uint64_t* u, const uint64_t* rho,
                                        const uint64_t* k1k2, int mode, int* ok, int* ok_each, void* stream);

/* ---- Fiat-Shamir: a Keccak-256 transcript, derived challenges ------------------------------
 * The entry points above take alpha beta gamma z v, u and rho from the caller. For the prover no
 * caller can choose them soundly: beta and gamma must depend on a_s b_s c_s, alpha on z_s, z on the
 * t commitments, all outputs of the same call. The _fs forms below take no challenge: they derive
 * them from the transcript fixed here (normative), so prove_fs returns a
 * non-interactive proof and verify_fs / verify_batch_fs check one.
 *
 * H is Keccak-256 (rate 136 bytes, padding 0x01 .. 0x80, 32-byte digest: Ethereum's variant, not
 * SHA3-256). All integers are big-endian: u64(k) is 8 bytes; be32(x) is 32 bytes, for an Fr value
 * or an Fq coordinate, from the canonical 4 x u64 limbs; pt(P) = be32(x) | be32(y), the identity
 * (0,0) being 64 zero bytes. A challenge is int(digest) mod r. Every item is a multiple of 8
 * bytes, so a message is a sequence of whole Keccak lanes.
 *   Tree digest of m 32-byte items under tag g: root = 32 zero bytes if m = 0; otherwise replace the
 *   items by H(c_0 | .. | c_k-1) over consecutive groups of 4 (the last group has k = 1..4), repeat,
 *   at least once, until one item remains: root. The digest is H(u64(g) | u64(m) | root); the
 *   length fixes the tree's shape, so nodes carry no tag.
 *   Circuit digest (the verification key only):
 *     h0 = H(D | u64(mode) | u64(n) | u64(npub) | be32(k1) | be32(k2) | pt(q_m) | pt(q_l) | pt(q_r)
 *            | pt(q_o) | pt(q_c) | pt(s_sigma_1) | pt(s_sigma_2) | pt(s_sigma_3) | G2S)
 *     D = the 30 ASCII bytes "pbf-plonk-bn254-fiat-shamir-v1" and two zero bytes; the 8 points are
 *     the verifier's preprocessed commitments; G2S = g2[1] = [s]G2, four coordinates as be32 in the
 *     order of the 16 x u64 array.
 *   Per proof (pub, out_pts and out_f orders):
 *     P  = tree digest, tag 7, of be32(pub_0) .. be32(pub_npub-1)
 *     t1 = H(h0 | u64(1) | P | pt(a_s) | pt(b_s) | pt(c_s))        beta  = t1 mod r
 *     t2 = H(t1 | u64(2))                                          gamma = t2 mod r
 *     t3 = H(t2 | u64(3) | pt(z_s))                                alpha = t3 mod r
 *     t4 = H(t3 | u64(4) | pt(t_lo) | pt(t_mid) | pt(t_hi))        z     = t4 mod r
 *     t5 = H(t4 | u64(5) | be32 of the 7 proof fields, in order)   v     = t5 mod r
 *     t6 = H(t5 | u64(6) | pt(W_z) | pt(W_zw))                     u     = t6 mod r
 *   Per batch of count proofs: T = tree digest, tag 8, of t6_0 .. t6_count-1;
 *     rho_i = H(T | u64(9) | u64(i)) mod r, 0 replaced by 1.
 * The reduction mod r of a 256-bit digest is biased (a residue has 5 or 6 preimages), as in the
 * on-chain verifiers of this curve. Proof bytes are hashed as given, canonical and on the curve or
 * not: rejecting them stays the verifier's business, and the transcript has no failing case.
 *
 * Where it runs: single proofs (prove_fs, verify_fs, the circuit digest) hash on the host; a batch
 * (pbf_plonk_challenges_bn254, verify_batch_fs) on the GPU, one lane per proof, next to the proofs
 * the batch uploads anyway -- its chal, u and rho never exist on the host. Public inputs are hashed
 * where they are: the prover's d_pub by the tree kernel.
 *
 *   pbf_keccak256_batch*: count messages of len >= 0 bytes each, `pitch` >= len bytes apart ->
 *     out count x 32 bytes. _dev: device pointers (d_out 8-byte aligned), enqueued on `stream`.
 *   pbf_plonk_circuit_digest_bn254*: h0 (32 bytes, host) of the circuit, SRS, g2, k1k2, mode and
 *     npub, through the verification key and its cache (pbf_plonk_verify_bn254); no kernel of its own.
 *   pbf_plonk_challenges_bn254: all host pointers; digest h0; proof_pts count x 9 x 8, proof_f
 *     count x 7 x 4, pub count x npub x 4 -> chal count x 5 x 4 in the order alpha beta gamma z v
 *     of the entry points above, u count x 4, rho count x 4 (or NULL: not derived). A caller of the
 *     plain entry points gets its challenges here.
 *   pbf_plonk_prove_bn254_fs*: the arguments of _pi / _pi_dev with chal replaced by digest (h0 of
 *     THIS circuit, SRS and npub: the prover does not check it, a proof under another digest simply
 *     does not verify), and out_chal: NULL, or 6 x 4 receiving alpha beta gamma z v u. Each round's
 *     commitments are collected when the round ends and the next challenge derived before the next
 *     round is enqueued: four collections (slots 0-2, 3, 4-6, 7-8) in place of the plain entry's
 *     one, so three stream synchronisations more; the launches are otherwise the plain entry's. pbf_plonk_prove_bn254_pi with those challenges returns the
 *     same proof bit for bit.
 *   pbf_plonk_verify_bn254_fs*: the arguments of _pi* without chal and u. The circuit digest comes
 *     from the verification key, so a proof made under another digest fails (ok = 0). pub is hashed
 *     on one host thread, about npub / 3 permutations at 0.3 us each where measured: 0.11 s at
 *     npub = 2^20 against a verification of 4 ms. A caller with statements that large verifies
 *     through the batch form with count = 1, which hashes pub on the device.
 *   pbf_plonk_verify_bn254_batch_fs*: the arguments of _batch_pi* without chal, u and rho; ok_each
 *     localises with the derived values.
 * Errors (PBF_EINVAL, before anything is enqueued): a NULL pointer (pub may be NULL with npub = 0,
 * out_chal, rho and ok_each are optional), npub > n, a pub value >= r (the prover's _dev form finds
 * it in its first kernel), count = 0 or > 2^20 (pbf_keccak256_batch*: count = 0 or > 2^37 - 64, one
 * launch of blocks of 64), count x ceil(npub / 4) > 2^37 - 64, pitch < len. The sharded and _multi provers and the
 * stand-alone KZG entry points have no transcript (their callers can use pbf_keccak256_batch). */
int pbf_keccak256_batch(pbf_ctx* ctx, const uint8_t* msgs, size_t count, size_t len, size_t pitch, uint8_t* out);
int pbf_keccak256_batch_dev(pbf_ctx* ctx, const uint8_t* d_msgs, size_t count, size_t len, size_t pitch,
                            uint8_t* d_out, void* stream);
int pbf_plonk_circuit_digest_bn254(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                   const uint64_t* srs, size_t srs_m, const uint64_t* g2, const uint64_t* k1k2,
                                   int mode, size_t npub, uint8_t* digest);
int pbf_plonk_circuit_digest_bn254_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                       const uint64_t* d_srs, size_t srs_m, const uint64_t* g2, const uint64_t* k1k2,
                                       int mode, size_t npub, uint8_t* digest, void* stream);
int pbf_plonk_challenges_bn254(pbf_ctx* ctx, const uint8_t* digest, size_t count, const uint64_t* proof_pts,
                               const uint64_t* proof_f, const uint64_t* pub, size_t npub, uint64_t* chal, uint64_t* u,
                               uint64_t* rho);
int pbf_plonk_prove_bn254_fs(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies, const uint64_t* abc,
                             const uint64_t* pub, size_t npub, const uint8_t* digest, const uint64_t* rnd,
                             const uint64_t* k1k2, const uint64_t* srs, size_t srs_m, int mode, uint64_t* out_pts,
                             uint64_t* out_f, uint64_t* out_chal);
int pbf_plonk_prove_bn254_fs_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                 const uint64_t* d_abc, const uint64_t* d_pub, size_t npub, const uint8_t* digest,
                                 const uint64_t* rnd, const uint64_t* k1k2, const uint64_t* d_srs, size_t srs_m,
                                 int mode, uint64_t* out_pts, uint64_t* out_f, uint64_t* out_chal, void* stream);
int pbf_plonk_verify_bn254_fs(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies, const uint64_t* srs,
                              size_t srs_m, const uint64_t* g2, const uint64_t* proof_pts, const uint64_t* proof_f,
                              const uint64_t* pub, size_t npub, const uint64_t* k1k2, int mode, int* ok);
int pbf_plonk_verify_bn254_fs_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                  const uint64_t* d_srs, size_t srs_m, const uint64_t* g2, const uint64_t* proof_pts,
                                  const uint64_t* proof_f, const uint64_t* pub, size_t npub, const uint64_t* k1k2,
                                  int mode, int* ok, void* stream);
int pbf_plonk_verify_bn254_batch_fs(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                    const uint64_t* srs, size_t srs_m, const uint64_t* g2, size_t count,
                                    const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* pub,
                                    size_t npub, const uint64_t* k1k2, int mode, int* ok, int* ok_each);
int pbf_plonk_verify_bn254_batch_fs_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                        const uint64_t* d_srs, size_t srs_m, const uint64_t* g2, size_t count,
                                        const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* pub,
                                        size_t npub, const uint64_t* k1k2, int mode, int* ok, int* ok_each,
                                        void* stream);

/* ---- KZG commitments over BN254 (the scheme inside Plonk::prove / verify, on its own) ------
 * Elements as above: Fr canonical 4 x u64, G1 affine 8 x u64 with (0,0) the identity, G2 16 x u64;
 * srs = [G, sG, s^2 G, ...] as pbf_srs_create_bn254 writes it (G = (1, 2)), g2 = [G2, [s]G2].
 * `batch` polynomials of `len` coefficients each, polynomial b starting at element b * pitch
 * (pitch >= len). Results come back on the host, synchronised on the context's host stream
 * (host forms) or the given stream (_dev forms: device srs and polynomials, everything else on the
 * host), as pbf_msm_g1_bn254_fixed_dev returns its point; the stream contract, the side stream of
 * the fixed-base MSM and its cached window table of the SRS (keyed by the points and srs_m) are
 * that entry point's.
 *
 * pbf_poly_eval_fr256: Poly::eval (poly.rs:71-79) over Fr, the twin of pbf_poly_eval_u64:
 *   ys[i] = sum_j coeffs[j] * xs[i]^j for n >= 1 coefficients and nx >= 1 points (repeats allowed);
 *   coefficients and points are checked canonical.
 * pbf_kzg_commit_bn254*: SRS::eval_at_s (plonk.rs:51-58), out_pts[b] = sum_j p_b[j] * srs[j]: one
 *   fixed-base MSM per polynomial. Needs srs_m >= len.
 * pbf_kzg_open_bn254*: the batched opening at one point (plonk.rs:429-446):
 *     out_y[b] = p_b(z),     out_w = commit( (sum_b weights_b (p_b(x) - out_y[b])) / (x - z) ).
 *   The weights are explicit (the prover's are 1, z^(n+2), z^(2n+4), v, v^2, ..., not pure powers).
 *   The prover's own sequence: chunked Horner evaluations, the weighted sum of the polynomials,
 *   one synthetic division by (x - z), then one fixed-base MSM over the quotient. Needs
 *   srs_m >= len - 1; with len = 1 the quotient is empty and out_w is the identity.
 *   z and the weights may be any canonical values, 0 included; z may be a root of a polynomial or
 *   a point of any NTT domain: synthetic division has no failing case and none is added.
 * pbf_kzg_verify_bn254: `count` openings (C_i, z_i, y_i, W_i), host pointers:
 *     *ok = [ e(sum_i rho_i W_i, [s]G2) * e(-sum_i rho_i (C_i - y_i G + z_i W_i), G2) == 1 ]
 *   as one MSM over count points, one over 2 count + 1 points and one pairing check, whatever
 *   `count` is. count = 1, rho = 1 is the single check of plonk.rs:641-650. A batched opening
 *   enters as one entry: C = sum_b weights_b C_b, y = sum_b weights_b y_b.
 *   Randomness: the library reads none (the contract of pbf_plonk_verify_bn254_batch). Soundness
 *   rests on the caller choosing the weights rho unpredictably and AFTER seeing the openings
 *   (e.g. by hashing all of them); with predictable or equal weights the errors of two bad
 *   entries can cancel (y_0 + d, y_1 - d at one z under rho = 1, 1) and the batch passes.
 *   A point that is not canonical or not on the curve gives *ok = 0 outright ((0,0) is accepted);
 *   there is no per-entry localisation.
 * Errors (PBF_EINVAL, before anything is enqueued; never an abort): NULL pointers; len = 0,
 * batch = 0 or batch > 2^16; count = 0 or count > 2^20; pitch < len; a short SRS; a host scalar
 * (z, a weight, y, rho) >= r; rho_i = 0.                                                       */
int pbf_poly_eval_fr256(pbf_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t* xs, size_t nx, uint64_t* ys);
int pbf_kzg_commit_bn254(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* polys, size_t len,
                         size_t pitch, size_t batch, uint64_t* out_pts);
int pbf_kzg_commit_bn254_dev(pbf_ctx* ctx, const uint64_t* d_srs, size_t srs_m, const uint64_t* d_polys, size_t len,
                             size_t pitch, size_t batch, uint64_t* out_pts, void* stream);
int pbf_kzg_open_bn254(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* polys, size_t len,
                       size_t pitch, size_t batch, const uint64_t* z, const uint64_t* weights, uint64_t* out_y,
                       uint64_t* out_w);
int pbf_kzg_open_bn254_dev(pbf_ctx* ctx, const uint64_t* d_srs, size_t srs_m, const uint64_t* d_polys, size_t len,
                           size_t pitch, size_t batch, const uint64_t* z, const uint64_t* weights, uint64_t* out_y,
                           uint64_t* out_w, void* stream);
int pbf_kzg_verify_bn254(pbf_ctx* ctx, const uint64_t* g2, size_t count, const uint64_t* commits, const uint64_t* z,
                         const uint64_t* y, const uint64_t* w, const uint64_t* rho, int* ok);

/* ---- Multi-point KZG openings: many polynomials, many points, two G1 points -------------------
 * The multi-point opening of Boneh, Drake, Fisch and Gabizon ("Efficient polynomial commitment
 * schemes for multiple points and polynomials", 2020, section 4): `batch` polynomials p_b, each
 * opened on its own non-empty subset S_b of a set T of npts distinct points, are proven by two G1
 * points, W and W', with two MSMs on the prover's side however many points there are, and checked
 * with [s]G2 and one pairing check. srs, srs_m, polys, len, pitch, batch, the elements, the streams
 * and the results are those of "KZG commitments" above (_dev: device srs and polynomials,
 * everything else on the host).
 *   pts    npts x 4 u64, the points t_0 .. t_(npts-1) of T, canonical and distinct, 1 <= npts <= 32
 *   sets   batch u64 masks: bit j of sets[b] says t_j in S_b; no mask is zero or has a bit at npts
 *          or above
 *   gamma, z   the two challenges, one canonical value each. The library derives no challenge:
 *          gamma must be derived AFTER the commitments and the evaluations y, and z AFTER W (e.g.
 *          by hashing them into the caller's transcript); soundness rests on that order.
 * With r_b the interpolation of p_b on S_b and Z_S(x) = prod_{t in S} (x - t):
 * pbf_kzg_open_multi_bn254*: phase 1.
 *     out_y[b][j] = p_b(t_j) for j in S_b, zero words elsewhere (batch x npts x 4),
 *     out_w = W = commit( sum_b gamma^b (p_b - r_b) / Z_{S_b} ).
 *   The polynomials are grouped by equal set, one weighted sum and one division by Z_S per
 *   distinct set; the division is |S| synthetic divisions over one read of the sum (partial
 *   fractions), so there is no failing case and none is added: points may be 0, roots of a
 *   polynomial or points of an NTT domain, gamma may be 0 (0^0 = 1). Needs srs_m >= len - 1; with
 *   len = 1 W is the identity and the SRS is not read.
 * pbf_kzg_open_multi_finish_bn254*: phase 2, after the caller has derived z from W.
 *     out_w2 = W' = commit( (sum_b gamma^b Z_{T \ S_b}(z) (p_b - r_b(z)) - Z_T(z) h) / (x - z) ),
 *   h the polynomial W commits to. The call is stateless: it takes the same polynomials, points,
 *   sets and gamma again and recomputes h (two more sweeps, no MSM). z may be any canonical value,
 *   a point of T and 0 included. Needs srs_m >= len - 1; with len = 1 W' is the identity.
 * pbf_kzg_verify_multi_bn254: `count` multi-openings of one shape (batch, npts, sets), each with
 *   its own commits (count x batch x 8), pts (count x npts x 4), y (count x batch x npts x 4; entries
 *   outside a set are not read), gamma, z, rho (count x 4 each), w, w2 (count x 8 each); host pointers.
 *     F_i = sum_b gamma_i^b Z_{T \ S_b}(z_i) (C_ib - r_ib(z_i) G) - Z_T(z_i) W_i
 *     *ok = [ e(sum_i rho_i W'_i, [s]G2) * e(-sum_i rho_i (F_i + z_i W'_i), G2) == 1 ]
 *   as one MSM over count points, one over count (batch + 2) + 1 points and one pairing check.
 *   r_ib(z_i) is taken in product form; nothing is divided by z_i - t_j, so z_i in T is accepted.
 *   Randomness: the library reads none (the contract of pbf_kzg_verify_bn254). Soundness of the
 *   batch rests on the caller choosing the weights rho unpredictably and AFTER seeing the openings
 *   (e.g. by hashing all of them); with predictable or equal weights the errors of two bad
 *   openings can cancel and the batch passes. count = 1, rho = 1 is the single check.
 *   A point that is not canonical or not on the curve gives *ok = 0 outright ((0,0) is accepted);
 *   there is no per-opening localisation.
 * Errors (PBF_EINVAL, before anything is enqueued or written; never an abort): every error of
 * pbf_kzg_open_bn254*; npts = 0 or npts > 32; two equal points in pts (per opening in the
 * verifier); a mask that is zero or has a bit at npts or above; pts, gamma, z or a y inside its
 * set >= r; rho_i = 0 or >= r; count = 0; count * batch > 2^20.                                 */
int pbf_kzg_open_multi_bn254(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* polys, size_t len,
                             size_t pitch, size_t batch, const uint64_t* pts, size_t npts, const uint64_t* sets,
                             const uint64_t* gamma, uint64_t* out_y, uint64_t* out_w);
int pbf_kzg_open_multi_bn254_dev(pbf_ctx* ctx, const uint64_t* d_srs, size_t srs_m, const uint64_t* d_polys,
                                 size_t len, size_t pitch, size_t batch, const uint64_t* pts, size_t npts,
                                 const uint64_t* sets, const uint64_t* gamma, uint64_t* out_y, uint64_t* out_w,
                                 void* stream);
int pbf_kzg_open_multi_finish_bn254(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* polys, size_t len,
                                    size_t pitch, size_t batch, const uint64_t* pts, size_t npts,
                                    const uint64_t* sets, const uint64_t* gamma, const uint64_t* z,
                                    uint64_t* out_w2);
int pbf_kzg_open_multi_finish_bn254_dev(pbf_ctx* ctx, const uint64_t* d_srs, size_t srs_m, const uint64_t* d_polys,
                                        size_t len, size_t pitch, size_t batch, const uint64_t* pts, size_t npts,
                                        const uint64_t* sets, const uint64_t* gamma, const uint64_t* z,
                                        uint64_t* out_w2, void* stream);
int pbf_kzg_verify_multi_bn254(pbf_ctx* ctx, const uint64_t* g2, size_t count, size_t batch, size_t npts,
                               const uint64_t* sets, const uint64_t* commits, const uint64_t* pts, const uint64_t* y,
                               const uint64_t* gamma, const uint64_t* z, const uint64_t* w, const uint64_t* w2,
                               const uint64_t* rho, int* ok);

/* ---- KZG in evaluation form: G1 NTT, Lagrange-basis SRS, opening from evaluations -----------
 * A polynomial of degree < n given by its values on H = <omega> (evals[i] = p(omega^i), as the
 * NTT entry points leave witness columns, extensions and quotients) is committed and opened as it
 * stands, with no inverse transform, against the SRS in the Lagrange basis
 *     lsrs[i] = [L_i(s)]G,   L_i(x) = (x^n - 1) omega^i / (n (x - omega^i)),   i < n.
 * omega: canonical, of order exactly n; n a power of two, 1 <= n <= 2^28.
 *
 * pbf_ntt_g1_bn254*: the NTT over G1 points, natural order in and out:
 *     inverse = 0:  out[k] = sum_j [omega^(jk)] in[j]
 *     inverse = 1:  out[j] = [n^-1] sum_k [omega^(-jk)] in[k]
 *   Points are canonical affine, 8 x u64, (0,0) the identity. The output is the unique canonical
 *   form, so inverse(forward(x)) == x bit for bit. in == out is allowed. Its main use is the
 *   Lagrange-basis SRS, computed without the trapdoor:
 *     lsrs = the inverse G1 NTT of srs[0 .. n).
 *   The host form checks every point canonical and on the curve (PBF_EINVAL before the
 *   transform is enqueued). The _dev form does not check, like pbf_ntt_u64_batch_dev: input off
 *   the curve gives unspecified points, never a fault. Cost: n/2 (log2 n - 1) products of a point
 *   by a full-width scalar (the inverse: n more), on a 4-bit fixed window. The
 *   context keeps the table of omega's powers per (omega, n) until pbf_ctx_release_caches, and
 *   n x 128 B of scratch plus the window table of option g1ntt.tile_log.
 * pbf_ntt_g1_bn254_batch*: `batch` transforms of size n under the same omega in one call,
 *   transform b at in + 8*b*n and out + 8*b*n (u64 words; the layout is compact); in == out is
 *   allowed. Each transform is, bit for bit, what pbf_ntt_g1_bn254* returns for that slice, and
 *   the single forms are batch = 1 of this one. Limits: 1 <= batch and n * batch <= 2^28, the
 *   scratch of the largest single transform. The host form checks every point of every transform;
 *   the _dev form does not, like its single twin. Cost: batch times the products of the single
 *   transform, in batch times fewer launches: a stage is ceil(batch n/2 / 2^g1ntt.tile_log)
 *   launches, and a launch costs the latency of one window product however few lanes it carries,
 *   so small transforms are far cheaper by the batch than one by one. Scratch:
 *   n * batch x 128 B plus the window table (min(n * batch / 2, 2^tile_log) x 1920 B; the inverse:
 *   n * batch).
 * Commit from evaluations needs no entry point of its own:
 *     pbf_kzg_commit_bn254*(lsrs, n, evals, n, pitch, batch, out) = [p_b(s)]G,
 *   the same points as the commitments of the coefficient forms against srs, and
 *   pbf_kzg_verify_bn254 verifies them unchanged.
 * pbf_kzg_open_evals_bn254*: the batched opening of pbf_kzg_open_bn254 from evaluations;
 *   polynomial b is the n values at evals + b * pitch:
 *     out_y[b] = p_b(z),   out_w = sum_i q_i lsrs[i],
 *     q = the values on H of (sum_b weights_b (p_b(x) - out_y[b])) / (x - z),
 *   the same y and, bit for bit, the same point W as pbf_kzg_open_bn254 returns for the
 *   coefficient forms. With u_i = 1 / (omega^i - z), c = sum_b weights_b p_b, y_c = sum_b
 *   weights_b y_b: y_b = -(z^n - 1) n^-1 sum_i p_b[i] omega^i u_i and q_i = (c_i - y_c) u_i: one
 *   batch inversion, one dot product per polynomial, one pointwise sweep, one fixed-base MSM.
 *   z inside H is no failing case either: for z = omega^k (found on the device) y_b = p_b[k],
 *   q_i as above for i != k, and q_k = -omega^-k sum_{i != k} omega^i q_i; the inversion never
 *   sees the zero denominator. n = 1: y_b = p_b[0], W is the identity and lsrs is not read.
 * One window table per context: the fixed-base MSM caches the window table of ONE point set. A
 *   caller who alternates srs and lsrs on one context rebuilds that table at every switch;
 *   two contexts, one per basis, avoid it.
 * Streams and results as the KZG entry points above (_dev: d_lsrs, d_evals, d_in, d_out on the
 *   device, everything else on the host; caller's stream only).
 * Errors (PBF_EINVAL, before anything is enqueued): those of pbf_kzg_open_bn254* with len read as
 *   n; n = 0, not a power of two or above 2^28; omega >= r or not of order exactly n; NULL
 *   pointers; in the host form of the NTT a coordinate >= q or a point off the curve (of any
 *   transform of a batch); batch = 0 or n * batch > 2^28. Nothing is enqueued or written.       */
int pbf_ntt_g1_bn254(pbf_ctx* ctx, const uint64_t* omega, const uint64_t* in, uint64_t* out, size_t n, int inverse);
int pbf_ntt_g1_bn254_dev(pbf_ctx* ctx, const uint64_t* omega, const uint64_t* d_in, uint64_t* d_out, size_t n,
                         int inverse, void* stream);
int pbf_ntt_g1_bn254_batch(pbf_ctx* ctx, const uint64_t* omega, const uint64_t* in, uint64_t* out, size_t n,
                           size_t batch, int inverse);
int pbf_ntt_g1_bn254_batch_dev(pbf_ctx* ctx, const uint64_t* omega, const uint64_t* d_in, uint64_t* d_out, size_t n,
                               size_t batch, int inverse, void* stream);
int pbf_kzg_open_evals_bn254(pbf_ctx* ctx, const uint64_t* lsrs, size_t n, const uint64_t* omega,
                             const uint64_t* evals, size_t pitch, size_t batch, const uint64_t* z,
                             const uint64_t* weights, uint64_t* out_y, uint64_t* out_w);
int pbf_kzg_open_evals_bn254_dev(pbf_ctx* ctx, const uint64_t* d_lsrs, size_t n, const uint64_t* omega,
                                 const uint64_t* d_evals, size_t pitch, size_t batch, const uint64_t* z,
                                 const uint64_t* weights, uint64_t* out_y, uint64_t* out_w, void* stream);

/* ---- Every opening at once: the pointwise G1 product and FK20 over the G1 NTT ----------------
 * All n openings of a polynomial on its domain, W_i for z = omega^i, i < n (the multiproofs of
 * data-availability sampling and vector-commitment lookups), from two G1 transforms instead of
 * n calls of pbf_kzg_open_bn254* (Feist-Khovratovich). Elements as above.
 *
 * pbf_g1_bn254_mul*: out_i = [scalars_i] points_i, i < n: a different point for every scalar
 *   (pbf_g1_bn254_mul_base_dev multiplies G only; the MSM sums). Points canonical affine, (0,0)
 *   the identity; scalars canonical; the output is the unique canonical affine form. out may be
 *   points. 1 <= n <= 2^32. The host form checks every point canonical and on the curve and every
 *   scalar < r (PBF_EINVAL before the product is enqueued); the _dev form does not check, like
 *   pbf_ntt_g1_bn254_dev: input off the curve gives unspecified points, never a fault. The
 *   window product of the G1 NTT, on its window table (option g1ntt.tile_log).
 *
 * With srs[k] = [s^k]G, p(x) = sum_{j<n} p_j x^j (coefficients past len are zero), omega2 of
 * order exactly 2n and omega = omega2^2:
 *     W_(omega^i) = sum_{m<n} omega^(im) h_m,   h_m = sum_{k=0}^{n-2-m} p_(m+1+k) srs[k],
 *   h_(n-1) the identity: W is the forward G1 NTT of size n of h, and h_m = c_(n-1+m) for the
 *   convolution c = a * b of a_t = srs[n-2-t] (t <= n-2, the identity for n-1 <= t < 2n) with
 *   b_j = p_j (j < n, 0 above), which has degree <= 2n-3 and does not wrap at size 2n.
 * pbf_kzg_fk20_setup_bn254*: once per (SRS, n), into the caller's buffer of 2n points,
 *     xext = the forward G1 NTT of size 2n, root omega2, of a       (canonical affine),
 *   so a caller may also compute or store it. Needs srs_m >= n - 1 (points 0 .. n-2 are read).
 *   n a power of two, 1 <= n <= 2^27; with n = 1 xext is two identities. The host form checks
 *   the points it reads; d_xext must not overlap d_srs.
 * pbf_kzg_open_all_bn254*: polynomials laid out as pbf_kzg_open_bn254* takes them, 1 <= len <= n;
 *   weights on the host, as there:
 *     out_y[b*n + i] = p_b(omega^i)  (batch x n values; out_y may be NULL),
 *     out_w[i] = bit for bit the out_w of pbf_kzg_open_bn254 for the same polynomials and
 *                weights at z = omega^i  (n points).
 *   Per call: c = (2n)^-1 sum_b weights_b p_b formed once on coefficients (the inverse
 *   transform's factor rides on the weights, so the batch costs one transform set whatever its
 *   size), bhat = the Fr NTT of size 2n of c, the products [bhat_i] xext_i written where the
 *   unscaled inverse G1 NTT of size 2n reads them, then the forward one of size n over entries
 *   n-1 .. 2n-2 of its result: 2n + n log2 n + n/2 (log2 n - 1) window products and
 *   one affine conversion per output point, none in between. The values y are Fr NTTs of size n.
 *   xext is trusted as the setup wrote it (not checked). With len = 1 every W is the identity.
 *   Scratch kept by the context: 2n x 128 B of points plus the window table of option
 *   g1ntt.tile_log (min(2n, 2^tile_log) x 1920 B: 30 MiB by default), 2n x 32 B for bhat and
 *   len x 32 B for c; the tables of omega2's and omega's powers stay until pbf_ctx_release_caches.
 * Streams: the caller's stream only. The _dev forms take d_srs, d_xext, d_polys, d_points,
 *   d_scalars and every output on the device, and their results stay there, stream-ordered;
 *   omega2 and the weights are on the host. Outputs must not overlap inputs except where stated.
 * Errors (PBF_EINVAL, before anything is enqueued): those of pbf_kzg_open_bn254* (NULL pointers,
 *   len = 0, batch = 0 or > 2^16, pitch < len, a weight >= r); len > n; n = 0, not a power of
 *   two or above 2^27; omega2 >= r or not of order exactly 2n; a short SRS; for the product n = 0.  */
int pbf_g1_bn254_mul(pbf_ctx* ctx, const uint64_t* points, const uint64_t* scalars, uint64_t* out, size_t n);
int pbf_g1_bn254_mul_dev(pbf_ctx* ctx, const uint64_t* d_points, const uint64_t* d_scalars, uint64_t* d_out, size_t n,
                         void* stream);
int pbf_kzg_fk20_setup_bn254(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* omega2, size_t n,
                             uint64_t* xext);
int pbf_kzg_fk20_setup_bn254_dev(pbf_ctx* ctx, const uint64_t* d_srs, size_t srs_m, const uint64_t* omega2, size_t n,
                                 uint64_t* d_xext, void* stream);
int pbf_kzg_open_all_bn254(pbf_ctx* ctx, const uint64_t* xext, size_t n, const uint64_t* omega2,
                           const uint64_t* polys, size_t len, size_t pitch, size_t batch, const uint64_t* weights,
                           uint64_t* out_y, uint64_t* out_w);
int pbf_kzg_open_all_bn254_dev(pbf_ctx* ctx, const uint64_t* d_xext, size_t n, const uint64_t* omega2,
                               const uint64_t* d_polys, size_t len, size_t pitch, size_t batch,
                               const uint64_t* weights, uint64_t* d_out_y, uint64_t* d_out_w, void* stream);

/* ---- KZG cell proofs: FK20 over cosets, batched cell verification ----------------------------
 * Data-availability sampling samples cells, not points: cell i < k = n / l is the l values of p
 * on the coset {omega^(i + k t) : t < l}, every point of which satisfies x^l = c_i = omega^(i l).
 * A cell has ONE proof, W_i = [q_i(s)]G for p = q_i (x^l - c_i) + I_i with deg I_i < l (I_i
 * interpolates p on the cell), and many cells are verified in one pairing check.
 * n and l are powers of two, 1 <= l <= n <= 2^27; omega2 of order exactly 2n, omega = omega2^2;
 * srs[j] = [s^j]G; p(x) = sum_{j<n} p_j x^j, coefficients past len zero.
 *     W_i = sum_{m<k} c_i^m h_m,   h_m = sum_{j=0}^{n-1-(m+1)l} p_(j+(m+1)l) srs[j],
 *   h_(k-1) the identity: W is the forward G1 NTT of size k, root omega^l, of h. With j = r + l u,
 *   r < l: h_m = sum_{r<l} (a_r * b_r)_(k-1+m) for the l convolutions of
 *     a_r[t] = srs[r + l (k-2-t)]  (t <= k-2, the identity for k-1 <= t < 2k)  with
 *     b_r[u] = p_(r + l u)         (u < k, 0 above),
 *   none of which wraps at size 2k.
 * pbf_kzg_cells_setup_bn254*: once per (SRS, n, l), into the caller's buffer of 2n points,
 *     xext[r*2k + i] = G1-NTT_{2k, omega2^l}(a_r)[i],  r < l, i < 2k   (canonical affine, slab-major),
 *   so a caller may also compute or store it. Needs srs_m >= n - l (points 0 .. n-l-1 are read).
 *   With l = 1 the output equals that of pbf_kzg_fk20_setup_bn254* bit for bit; with l = n every
 *   point is the identity. The l transforms run as one batch of the G1 NTT
 *   (pbf_ntt_g1_bn254_batch_dev: batch = l, size 2k, in place). The host form checks the points it
 *   reads; d_xext must not overlap d_srs.
 * pbf_kzg_open_cells_bn254*: polynomials, pitch, batch and the host weights exactly as
 *   pbf_kzg_open_all_bn254* takes them, 1 <= len <= n:
 *     out_w[i] = W_i of c = sum_b weights_b p_b, i < k   (k points),
 *     out_y[(b*k + i)*l + t] = p_b(omega^(i + k t))      (batch x n values, cell-major: the l
 *                values of a cell are consecutive, in the order the verifier takes them;
 *                out_y may be NULL).
 *   Per call: c = sum_b weights_b p_b, its b_r gathered times (2k)^-1 (the inverse transform's
 *   factor rides on them), bhat_r = the Fr NTT of size 2k, root omega2^l, of b_r, all l in one
 *   batch; the 2n products [bhat_(r,i)] xext_(r,i) as one vector; chat_i = their sum over r < l, written where
 *   the unscaled inverse G1 NTT of size 2k reads it; then the forward one of size k over entries
 *   k-1 .. 2k-2 of its result: 2n + k log2 k + k/2 (log2 k - 1) window products, 2k (l - 1)
 *   additions and one affine conversion per output point, nothing leaving Xyzz in between. The
 *   values y are the batched Fr NTT of size n followed by a transposing store. xext is trusted as
 *   the setup wrote it (not checked). With len <= l every W is the identity. With l = 1 out_w and
 *   out_y equal those of pbf_kzg_open_all_bn254* bit for bit.
 *   Scratch kept by the context: (2n + 2k) x 128 B of points plus the window table of option
 *   g1ntt.tile_log, 2n x 32 B for bhat, n x 32 B for the b_r, len x 32 B for c and, with out_y and
 *   1 < l < n, batch x n x 32 B; the power tables of omega2^l, omega^l and omega stay until
 *   pbf_ctx_release_caches.
 * pbf_kzg_open_cells_each_bn254*: the proofs of EACH polynomial of a batch in one call (a block
 *   builder's rows, or the rows pbf_kzg_recover_cells_bn254_dev has just recovered): xext, n, l,
 *   omega2, polys, len, pitch and the streams exactly as pbf_kzg_open_cells_bn254* takes them, and
 *   no weights:
 *     out_w[b*k + i] = W_i of p_b, i < k, b < batch      (batch x k points, polynomial-major),
 *   for every b bit for bit the out_w of pbf_kzg_open_cells_bn254* called on polynomial b alone
 *   with weight 1; out_y is exactly that entry point's out_y (batch x n values, cell-major; may be
 *   NULL). With l = 1 it is every opening of every polynomial (pbf_kzg_open_all_bn254* per
 *   polynomial); with len <= l every W is the identity. This version supports 1 <= batch <= 2^16
 *   and batch * n <= 2^24 (more: PBF_EINVAL; a caller with more rows loops).
 *   Per call: the steps of pbf_kzg_open_cells_bn254* with every vector batch times as long: one
 *   gather that also applies (2k)^-1, one batched Fr NTT of size 2k over batch x l rows, the
 *   batch x 2n products [bhat_(b,r,i)] xext_(r,i) as ONE vector (a launch takes 2^g1ntt.tile_log
 *   of them whatever 2n is: polynomials share a launch, and a launch may split a polynomial), the
 *   sums over r into batch x 2k slots, and the two transforms as batches of the G1 NTT over
 *   `batch` transforms: batch x (2n + k log2 k + k/2 (log2 k - 1)) window products, one affine
 *   conversion per output point, nothing leaving Xyzz in between. The transforms' 2 log2 k + 1
 *   stages are paid once per call, not once per polynomial.
 *   Scratch kept by the context: batch x (2n + 2k) x 128 B of points (every product is kept until
 *   the sums are formed: 4 GiB at batch * n = 2^24) plus the window table of option
 *   g1ntt.tile_log, batch x 2n x 32 B for bhat, batch x n x 32 B for the b_r and, with out_y and
 *   1 < l < n, batch x n x 32 B.
 * pbf_kzg_verify_cells_bn254: host pointers, like pbf_kzg_verify_bn254. g2 = [G2, [s^l]G2]: the
 *   caller brings the l-th power of s on the twist, not [s]G2 (a trusted setup publishes it; tests
 *   make it from a trapdoor with pbf_g2_bn254_mul). srs = the first l G1 points, srs_m >= l; omega
 *   of order exactly n. Entry j < count is (commits_j, cell_idx_j, ys[j*l .. (j+1)*l), w_j):
 *   cell_idx is uint64_t, each < k; ys is count x l values in the order of out_y. With
 *     I_(j,t) = omega^(-idx_j t) INTT_{l, omega^k}(ys_j)[t]   (the interpolant's coefficients),
 *   *ok = 1 exactly when
 *     e(sum_j rho_j W_j, [s^l]G2) e(-(sum_j rho_j C_j - [sum_j rho_j I_j](s) G
 *                                      + sum_j rho_j c_(idx_j) W_j), G2) == 1:
 *   one batched Fr INTT of size l over the count cells, one sweep, one MSM over count points, one
 *   over 2 count + l points ((C_j, rho_j), (W_j, rho_j c_(idx_j)), (srs[t], -sum_j rho_j I_(j,t))),
 *   one pairing check. Repeated cells and repeated commitments are allowed. count in 1 .. 2^20 and
 *   count * l <= 2^22. The context keeps the power table of (omega, n) (n/2 x 32 B).
 *   Randomness: the library reads none (the contract of pbf_kzg_verify_bn254). Soundness rests on
 *   the caller choosing the weights rho, nonzero and canonical, unpredictably and AFTER seeing the
 *   cells and proofs; with predictable or equal weights the errors of two bad entries can cancel
 *   (the same cell twice with one value raised by d in one copy and lowered by d in the other,
 *   under rho = 1, 1) and the batch passes. A point (of commits, w or srs) that is not canonical
 *   or not on the curve gives *ok = 0 outright ((0,0) is accepted); there is no per-entry
 *   localisation.
 * Streams: as the entry points above; the _dev forms take d_srs, d_xext, d_polys and every output
 *   on the device, omega2 and the weights on the host.
 * Errors (PBF_EINVAL, before anything is enqueued; never an abort): those of
 *   pbf_kzg_open_all_bn254* and pbf_kzg_verify_bn254; l = 0, not a power of two or above n; a short
 *   SRS (srs_m < n - l for the setup, srs_m < l for the verifier); cell_idx >= k; count * l > 2^22;
 *   omega not of order exactly n (omega2: 2n); a value of ys >= r; for
 *   pbf_kzg_open_cells_each_bn254* those of pbf_kzg_open_cells_bn254* without the weights, and
 *   batch * n > 2^24.                                                                           */
int pbf_kzg_cells_setup_bn254(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* omega2, size_t n,
                              size_t l, uint64_t* xext);
int pbf_kzg_cells_setup_bn254_dev(pbf_ctx* ctx, const uint64_t* d_srs, size_t srs_m, const uint64_t* omega2, size_t n,
                                  size_t l, uint64_t* d_xext, void* stream);
int pbf_kzg_open_cells_bn254(pbf_ctx* ctx, const uint64_t* xext, size_t n, size_t l, const uint64_t* omega2,
                             const uint64_t* polys, size_t len, size_t pitch, size_t batch, const uint64_t* weights,
                             uint64_t* out_y, uint64_t* out_w);
int pbf_kzg_open_cells_bn254_dev(pbf_ctx* ctx, const uint64_t* d_xext, size_t n, size_t l, const uint64_t* omega2,
                                 const uint64_t* d_polys, size_t len, size_t pitch, size_t batch,
                                 const uint64_t* weights, uint64_t* d_out_y, uint64_t* d_out_w, void* stream);
int pbf_kzg_open_cells_each_bn254(pbf_ctx* ctx, const uint64_t* xext, size_t n, size_t l, const uint64_t* omega2,
                                  const uint64_t* polys, size_t len, size_t pitch, size_t batch, uint64_t* out_y,
                                  uint64_t* out_w);
int pbf_kzg_open_cells_each_bn254_dev(pbf_ctx* ctx, const uint64_t* d_xext, size_t n, size_t l,
                                      const uint64_t* omega2, const uint64_t* d_polys, size_t len, size_t pitch,
                                      size_t batch, uint64_t* d_out_y, uint64_t* d_out_w, void* stream);
int pbf_kzg_verify_cells_bn254(pbf_ctx* ctx, const uint64_t* g2, const uint64_t* srs, size_t srs_m,
                               const uint64_t* omega, size_t n, size_t l, size_t count, const uint64_t* commits,
                               const uint64_t* cell_idx, const uint64_t* ys, const uint64_t* w, const uint64_t* rho,
                               int* ok);

/* ---- Recovery from cells: polynomials from any sufficient set of their KZG cells --------------
 * What the cells are for: a node that holds only some cells of an extended polynomial (the rest
 * never sampled, or withheld) rebuilds the polynomial, and from it the missing cells and their
 * proofs: the recover_cells_and_kzg_proofs of consensus specifications. A call
 * takes a batch of polynomials that share one pattern of missing cells (the rows of a block that
 * misses the same columns), so the work on the pattern is paid once per call.
 * Geometry as for the cell proofs: n and l powers of two, 1 <= l <= n <= 2^27, k = n / l; omega of
 * order exactly n, as pbf_kzg_verify_cells_bn254 takes it; cell i < k is the l values on
 * {omega^(i + k t) : t < l}. The unknown polynomials have len coefficients, 1 <= len <= n
 * (coefficients past len are zero; the usual case is len = n/2, the 2x extension). This version
 * supports n/l <= 2^16 (more cells: PBF_EINVAL).
 * Input: count known cells, 1 <= count <= k. cell_idx: count distinct values, each < k, in any
 *   order; a host pointer in both forms, like the weights of the other KZG entry points.
 *     cells[(b*count + j)*l + t] = the value of polynomial b at omega^(cell_idx[j] + k t),
 *   cell-major, the order of out_y of pbf_kzg_open_cells_bn254*: that output feeds this input with
 *   the missing cells simply left out. One pattern for all batch polynomials, 1 <= batch <= 2^16.
 *   The call needs count * l >= len (else PBF_EINVAL): below that nothing determines the polynomial.
 * Output: with R_b the unique polynomial of degree < count*l that takes the given values on the
 *   known cells,
 *     out_polys[b*pitch + j], j < len (pitch >= len) = the first len coefficients of R_b, canonical;
 *     consistent[b] = 1 exactly when every coefficient of R_b from len on is zero: the cells are
 *       the cells of a polynomial of len coefficients, and that polynomial is the output. With
 *       count*l == len every input is consistent. With consistent[b] = 0 polynomial b's outputs
 *       hold canonical values with no further meaning; the other polynomials are unaffected;
 *     out_y (may be NULL; else batch x n values) = all k cells of the polynomial written to
 *       out_polys, in the order of out_y of pbf_kzg_open_cells_bn254*: for a consistent input the
 *       known cells come back bit for bit and the missing ones are filled.
 *   Results are exact field elements; there is no tolerance anywhere.
 *   Proofs need no entry point of their own: pbf_kzg_open_cells_bn254_dev on d_out_polys gives every
 *   cell's proof, the missing cells' included.
 * Per call: with M the missing cells, Z(x) = prod_{i in M} (x^l - omega^(i l)) and E_b the known
 *   values with zero on the missing cells, E_b Z = R_b Z on H = <omega> and deg R_b Z < n: one
 *   batched inverse Fr NTT of size n, the forward transform on the coset 5 H, the pointwise
 *   division by Z there, the inverse coset transform (three batched transforms of
 *   pbf_ntt_fr256_batch_dev, the coset's factors 5^j and 5^-j applied by one launch each for the
 *   whole batch). Z depends on x only through x^l: its k values on H and k on the coset are
 *   formed once per call, directly as products over M (k |M| products each: hence n/l <= 2^16),
 *   and the coset's are inverted by the prover's batch inversion. 5^n != 1 for every n <= 2^28,
 *   so Z has no zero on the coset whatever is missing; the results do not depend on the shift.
 *   out_y is one more batched forward transform.
 *   Scratch kept by the context: batch x n x 32 B for the working array (the transforms run in
 *   place on it) beside the transforms' own, 2k x 32 B for Z, k x 32 B for the inversion, 2k x 4 B
 *   for the slot and missing-cell tables; the host form also holds its inputs and outputs. The
 *   powers of the shift, (n + 1) x 32 B per n used, are built at the first call of that n (one
 *   stream synchronisation) and stay with the context. The power table of (omega, n) is shared
 *   with pbf_kzg_verify_cells_bn254 and stays until pbf_ctx_release_caches. Nothing about the
 *   missing set is kept between calls.
 * Streams: the caller's stream only. The _dev form takes d_cells and every output on the device
 *   (d_consistent: batch ints) and leaves them there, stream-ordered; omega and cell_idx are on the
 *   host. The host form returns after its results are on the host, and checks every value of cells
 *   canonical; the _dev form does not check, like the other _dev forms: values >= r give
 *   unspecified values, never a fault. Outputs must not overlap inputs.
 * Errors (PBF_EINVAL, before anything is enqueued or written; never an abort): NULL ctx, omega,
 *   cell_idx, cells, out_polys or consistent; n or l zero, not a power of two, l > n or n > 2^27;
 *   n/l > 2^16; omega >= r or not of order exactly n; len = 0 or len > n; count = 0, count > k or
 *   count * l < len; a cell_idx value >= k or repeated; batch = 0 or batch > 2^16; pitch < len; in
 *   the host form a cell value >= r.                                                           */
int pbf_kzg_recover_cells_bn254(pbf_ctx* ctx, const uint64_t* omega, size_t n, size_t l, size_t len, size_t count,
                                const uint64_t* cell_idx, const uint64_t* cells, size_t batch, uint64_t* out_polys,
                                size_t pitch, uint64_t* out_y, int* consistent);
int pbf_kzg_recover_cells_bn254_dev(pbf_ctx* ctx, const uint64_t* omega, size_t n, size_t l, size_t len, size_t count,
                                    const uint64_t* cell_idx, const uint64_t* d_cells, size_t batch,
                                    uint64_t* d_out_polys, size_t pitch, uint64_t* d_out_y, int* d_consistent,
                                    void* stream);

/* Config 5 across G GPUs ("NTT sharded across 8xMI355X"): one process (or thread) per GPU
 * calls pbf_plonk_prove_bn254_sharded_dev with the same inputs (circuit, SRS, challenges,
 * blinders) and its rank. The library computes nothing collective itself: it calls back
 * into the caller's communicator (RCCL via torch.distributed in multigpu.py, or the library's
 * own in pbf_plonk_prove_bn254_multi), always for buffers it names in `comm` and
 * stream-ordered on `stream`:
 *   all_to_all(user, b, stream):  send[g*b .. (g+1)*b) goes to rank g, recv[g*b ..) comes from g
 *   all_gather(user, b, stream):  send[0 .. b) of rank g lands in recv[g*b .. (g+1)*b)
 * Work split, every witness-dependent step on this rank's share: satisfies and
 * the accumulator's terms / prefix products on rows [r n/G, (r+1) n/G) (the ranks' products
 * all-gathered); interpolation of a b c and of the accumulator as sharded INTTs; every coset NTT
 * of size 4n and the coset INTT of t as stride-sharded transforms; the quotient on this rank's
 * evaluation blocks; commitments, evaluations, r(x) and the opening divisions on this rank's
 * contiguous coefficient range (one all-to-all transposes the NTTs' stride shards into it; the
 * divisions' and evaluations' per-range totals are all-gathered); every commitment is this
 * rank's point range, the partial sums all-gathered once at the end. The circuit's proving key
 * is built once per circuit on every rank. Outputs are identical on every rank and
 * bit-identical to the single-GPU proof. n >= world^2. send / recv: device buffers of
 * `capacity` >= 5 * (4n / world) * 32 bytes each.                                          */
typedef struct pbf_comm {
  uint32_t world, rank;
  void* user;
  void* send;
  void* recv;
  size_t capacity;
  int (*all_to_all)(void* user, size_t bytes_per_peer, void* stream);
  int (*all_gather)(void* user, size_t bytes_per_rank, void* stream);
} pbf_comm;
int pbf_plonk_prove_bn254_sharded_dev(pbf_ctx* ctx, const pbf_comm* comm, size_t n, const uint64_t* d_q,
                                      const uint64_t* d_copies, const uint64_t* d_abc, const uint64_t* chal,
                                      const uint64_t* rnd, const uint64_t* k1k2, const uint64_t* d_srs,
                                      size_t srs_m, int mode, uint64_t* out_pts, uint64_t* out_f, void* stream);

/* ---- multi-GPU from ONE host process (SURVEY.md §8b pbf_ntt_u64_multi) -------------------
 * `ctxs` = G contexts (G = 2, 4, 8), rank g = ctxs[g]. The library owns the exchange: on G
 * distinct devices it uses RCCL (librccl loaded at run time; ncclCommInitAll, grouped
 * ncclSend / ncclRecv for the all-to-all, ncclAllGather), on one shared device (virtual ranks)
 * stream-ordered device copies ordered by events. The communicator and its buffers are kept
 * per context list (pointers and creation order) until a member context is destroyed. Each
 * rank runs in a library-owned host thread; errors name the failing rank. Outputs are
 * bit-identical to the single-GPU entry points.
 *
 * pbf_ntt_u64_multi: CooleyTurkey::fft / fft_inv (fft.rs:66-78) of one host vector of n points
 *   (n = G * nl, nl a power of two >= G), natural order in and out, with the top log2(G) levels of
 *   the recursion (fft.rs:94-96) across the ranks: the stride shards go to the G devices, one
 *   all-to-all, the blocks come back (pbf_ntt_shard_local_dev / _combine_dev, one rank each).
 * _dev: per-rank device buffers and streams: d_in[g] = rank g's stride shards [batch][nl]
 *   (forward) or blocks (inverse), d_out[g] likewise the other way round (streams may be NULL).
 * pbf_mul_ntt_*_multi: mul_ntt (fft.rs:109-132), la + lb = G * nl; out has la + lb entries.
 * pbf_plonk_prove_bn254_multi: Plonk::prove (plonk.rs:191-466) with the work split of
 *   pbf_plonk_prove_bn254_sharded_dev, the host inputs uploaded to every rank's device; _dev
 *   takes per-rank device copies (d_q[g] ... on rank g's device) and streams. The ranks'
 *   proofs are compared (PBF_ECOMM if they differ) and returned once.
 * pbf_multi_backend: *backend = 0 (device copies, one device) or 1 (RCCL).                   */
int pbf_ntt_u64_multi(pbf_ctx* const* ctxs, uint32_t world, uint64_t modulus, uint64_t omega, const uint64_t* in,
                      uint64_t* out, size_t n, int inverse);
int pbf_ntt_u64_multi_dev(pbf_ctx* const* ctxs, uint32_t world, uint64_t modulus, uint64_t omega,
                          const uint64_t* const* d_in, uint64_t* const* d_out, size_t nl, size_t batch, int inverse,
                          void* const* streams);
int pbf_ntt_fr256_multi(pbf_ctx* const* ctxs, uint32_t world, const uint64_t* omega, const uint64_t* in, uint64_t* out,
                        size_t n, int inverse);
int pbf_ntt_fr256_multi_dev(pbf_ctx* const* ctxs, uint32_t world, const uint64_t* omega, const uint64_t* const* d_in,
                            uint64_t* const* d_out, size_t nl, size_t batch, int inverse, void* const* streams);
int pbf_mul_ntt_u64_multi(pbf_ctx* const* ctxs, uint32_t world, uint64_t modulus, uint64_t omega, const uint64_t* a,
                          size_t la, const uint64_t* b, size_t lb, uint64_t* out);
int pbf_mul_ntt_fr256_multi(pbf_ctx* const* ctxs, uint32_t world, const uint64_t* omega, const uint64_t* a, size_t la,
                            const uint64_t* b, size_t lb, uint64_t* out);
int pbf_plonk_prove_bn254_multi(pbf_ctx* const* ctxs, uint32_t world, size_t n, const uint64_t* q, const uint64_t* copies,
                                const uint64_t* abc, const uint64_t* chal, const uint64_t* rnd, const uint64_t* k1k2,
                                const uint64_t* srs, size_t srs_m, int mode, uint64_t* out_pts, uint64_t* out_f);
int pbf_plonk_prove_bn254_multi_dev(pbf_ctx* const* ctxs, uint32_t world, size_t n, const uint64_t* const* d_q,
                                    const uint64_t* const* d_copies, const uint64_t* const* d_abc, const uint64_t* chal,
                                    const uint64_t* rnd, const uint64_t* k1k2, const uint64_t* const* d_srs,
                                    size_t srs_m, int mode, uint64_t* out_pts, uint64_t* out_f, void* const* streams);
int pbf_multi_backend(pbf_ctx* const* ctxs, uint32_t world, int* backend);

/* synthetic config-5 circuit on the device (bench / tests): every gate a*b = c, a, b
 * uniform (splitmix64 of seed), every 4th gate's c copied into the next gate's a       */
int pbf_plonk_synth_circuit_bn254_dev(pbf_ctx* ctx, size_t n, uint64_t seed, uint64_t* d_q, uint64_t* d_copies,
                                      uint64_t* d_abc, void* stream);
/* SRS::create with the output left on the device (n+1 points)                          */
int pbf_srs_create_bn254_dev(pbf_ctx* ctx, const uint64_t* s, size_t n, uint64_t* d_out, void* stream);

/* ---- Plonk-by-hand types (BASELINE config 1; src/pbh/{g1,g2,gt,pairing}.rs) -------------------
 * 32-bit words: G1 [x, y, inf] over F101 (y^2 = x^3 + 3), G2 [a, b] (a + b*u over
 * F101[u]/(u^2+2)), GT [a, b]. Inputs must be on the curve (else PBF_EINVAL, where the
 * reference would panic or compute garbage).                                        */
int pbf_pbh_g1_mul(pbf_ctx* ctx, const uint32_t* pts, const uint32_t* scalars, size_t n, uint32_t* out);
int pbf_pbh_g2_mul(pbf_ctx* ctx, const uint32_t* pts, const uint32_t* scalars, size_t n, uint32_t* out);
int pbf_pbh_gt_pow(pbf_ctx* ctx, const uint32_t* x, const uint32_t* e, size_t n, uint32_t* out);
/* PBHPairing::pairing (pairing.rs:12-47), batched                                    */
int pbf_pbh_pairing(pbf_ctx* ctx, const uint32_t* g1, const uint32_t* g2, size_t n, uint32_t* out);
/* Plonk::prove (+ Plonk::verify when verify_u < 17) over PlonkByHandTypes
 * (plonk.rs:120-650, pbh/mod.rs:18-33). gates: n x [q_l q_r q_o q_m q_c]; copies:
 * 3 columns x n x [kind (0=A,1=B,2=C), 1-based index]; abc: 3 x n witness; chal:
 * [alpha beta gamma z v]; rnd: 9 blinders; s: toxic waste; srs_n: SRS degree;
 * omega_pows: |H|. out_pts: 9 x [x y inf] (a_s b_s c_s z_s t_lo t_mid t_hi w_z w_zw),
 * out_f: [a_z b_z c_z s_sigma_1_z s_sigma_2_z r_z z_omega_z]; *verified = 1/0 (or -1).  */
int pbf_pbh_prove(pbf_ctx* ctx, size_t n, const uint64_t* gates, const uint64_t* copies,
                  const uint64_t* abc, const uint64_t* chal, const uint64_t* rnd, uint64_t s,
                  uint64_t srs_n, uint64_t omega_pows, uint64_t verify_u, uint64_t* out_pts,
                  uint64_t* out_f, int* verified);

/* ---- synthetic inputs (bench / tests) ------------------------------------- */
/* d_out[i] = splitmix64 stream of (seed, i) with rejection of values >= modulus;
 * identical to tests/golden/gen_golden.py:splitmix_field.                     */
int pbf_fill_random_u64_dev(pbf_ctx* ctx, uint64_t modulus, uint64_t seed, uint64_t* d_out,
                            size_t count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PBF_H */
