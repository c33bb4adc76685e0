// What prover.hip exports to the KZG units (through kzg.hpp) and the verifiers (verify.hip,
// verify_batch.hip): the geometry of the blocked synthetic division and host launchers of the
// prover's own kernels (chunked Horner evaluation, linear combination, k_hs1..3, the H powers and
// sigma labels). Plonk::prove goes through the same launchers. Then what g1_ntt.hip, g1_mul.hip
// and verify.hip export to the same users, and two device helpers over Fr.
#pragma once
#include <cstring>
#include <initializer_list>
#include "fr_host.hpp"
#include "msm.hpp"

namespace pbf {

// Synthetic division by (x - z) as a blocked linear recurrence (prover.hip k_hs1..3): HS_T
// threads of HS_PER consecutive steps each per block.
constexpr int HS_T = 256, HS_PER = 16, HS_BLK = HS_T * HS_PER, HS_LOG_T = 8;
// Conversion-free: the recurrence is linear with Montgomery-form multipliers (z, z^k), so
// canonical coefficients give canonical s_k, totals and quotients throughout.
struct HsArgs {
  const uint64_t* p;
  uint64_t L;
  U256 y;                 // subtracted from p_0 (canonical)
  U256 z;                 // Montgomery
  U256 zs[HS_LOG_T];      // z^(HS_PER 2^j)
};

// z and its table zs of a division by (x - z); z in Montgomery form
void hs_set_point(HsArgs& a, const U256& z);
// q = the quotient of (p - y) / (x - z) for p of L >= 2 coefficients (L - 1 coefficients),
// *rem = p(z) - y: k_hs1, k_hs2, k_hs3 (a.p, a.L, a.y set by the caller; a.z, a.zs by hs_set_point)
int hs_div_run(pbf_ctx* ctx, const HsArgs& a, uint64_t* q, uint64_t* rem, hipStream_t s);
// evals[p] = x^off polys[p](x) for np <= 12 device polynomials of lens[p] coefficients, at most
// two distinct points among xs (Montgomery form): k_eval_partial, k_eval_final. off is the global
// index of every poly[p][0]: 0 for whole polynomials, a rank's first coefficient for its range.
int fr_eval_run(const uint64_t* const* polys, const uint64_t* lens, const U256* xs, int np, uint64_t off,
                DevBuf& partial, uint64_t* d_evals, hipStream_t s);
// out[i] = sum_k c[k] in[k][i] (+ c0 at i = 0), i < count, for k <= 10 inputs; in[k] contributes
// 0 from lens[k] on (c, c0 in Montgomery form; an input may be `out` itself): k_lincomb
int fr_lincomb_run(int k, const uint64_t* const* in, const uint64_t* lens, const U256* c, const U256& c0,
                   uint64_t* out, uint64_t count, hipStream_t s);
// hpow[i] = omega^i (i < n) and copy_constraints_to_roots (plonk.rs:181-189) over all n rows:
// sigma[col][i] (3 n values); a label out of range sets *bad: k_powers29, k_sigma
int sigma_table_run(uint64_t n, const U256& omega, const U256& k1, const U256& k2, const uint64_t* d_copies,
                    uint64_t* hpow, uint64_t* sigma, int* bad, hipStream_t s);
// out[i] = start base^i (i < count), canonical; base and start in Montgomery form: k_powers29
int fr_powers_run(uint64_t* out, uint64_t count, const U256& base, const U256& start, hipStream_t s);
// out[i] = the Montgomery form of 1 / den[i] for canonical den (i < count; out may be den): the
// prover's batch inversion k_div_batch_w, one Fermat inverse per chunk of 64 x 32 elements or more.
// A zero denominator sets *bad and leaves its chunk unwritten.
int fr_inv_batch_run(pbf_ctx* ctx, const uint64_t* den, uint64_t* out, uint64_t count, int* bad, hipStream_t s);

// g1_ntt.hip: the evaluation domain H = <omega> of the G1 NTT and of KZG in evaluation form.
// n a power of two in 1 .. 2^28 and omega canonical of order exactly n, else PBF_EINVAL;
// *wm = omega in Montgomery form.
int fr_domain_check(const uint64_t* omega, size_t n, U256* wm);
// The context's device table of (omega, n): omega^i canonical for i < n/2 (omega^(i + n/2) is
// the negation), then n^-1 canonical at entry n/2. Built once per (omega, n) on s by
// fr_powers_run (one stream sync), kept until pbf_ctx_release_caches.
int fr_domain_table(pbf_ctx* ctx, const U256& wm, uint64_t n, hipStream_t s, const uint64_t** tw);
// omega^i from that table, canonical (i < n, n >= 2)
__device__ __forceinline__ U256 fr_domain_at(const uint64_t* tw, uint64_t n, uint64_t i) {
  const uint64_t h = n >> 1;
  const U256 w = u256_from_u64(tw + 4 * (i & (h - 1)));
  return i < h ? w : Fr::sub(u256_zero(), w);
}
// The workgroup's sum of v over its blockDim.x lanes (a power of two; sh: as many values), valid
// on lane 0. The leading barrier lets a kernel call it again on the same sh, as k_ev_dot does.
__device__ __forceinline__ U256 fr_block_sum(U256* sh, const U256& v) {
  const uint32_t t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  __syncthreads();
  for (uint32_t s = blockDim.x / 2; s; s >>= 1) {
    if (t < s) sh[t] = Fr::add(sh[t], sh[t + s]);
    __syncthreads();
  }
  return sh[0];
}

// g1_ntt.hip: the pieces of the G1 NTT that FK20 (kzg_cells.hip) strings together without leaving Xyzz.
// The context's scratch: x, `points` Xyzz (absent with points = 0), and the window table for
// launches of up to min(`products`, 2^g1ntt.tile_log) products, `stride` of them.
struct G1Work {
  Xyzz* x;
  Xyzz* tbl;
  uint64_t stride;
};
int g1_work(pbf_ctx* ctx, uint64_t points, uint64_t products, G1Work* w);
// *bad = some of the n device points (8 x u64) is not canonical or not on the curve; synchronises s
int g1_check_run(pbf_ctx* ctx, const uint64_t* d_pts, uint64_t n, hipStream_t s, int* bad);
// All of these take `batch` transforms of one size n and omega, transform q at w.x + q pitch
// (pitch >= n points); one launch carries butterflies of several transforms.
// The log2 n butterfly stages over w.x[0 .. n), n >= 2: input at bit-reversed indices, output in
// natural order, unscaled: x[k] = sum_j [omega^(jk)] in[j]. With in[j] stored at the bit-reversed
// index of (n - j) mod n it is the inverse transform without its factor n^-1.
// w from g1_work(ctx, ., batch n/2 or more, .).
int g1_ntt_stages(pbf_ctx* ctx, const U256& wm, uint64_t n, uint64_t batch, uint64_t pitch, const G1Work& w,
                  hipStream_t s);
// w.x[0 .. 2n) in natural order -> its entries n - 1 .. 2n - 2 and the identity, as the input of
// the stages of size n, in w.x[0 .. n) (n >= 2). Transform q at w.x + 2 q n before and after: the
// transforms of size n keep the pitch 2n.
int g1_ntt_slice(const G1Work& w, uint64_t n, uint64_t batch, hipStream_t s);
// d_out[q n + i] = (w.x + q pitch)[i] as canonical affine, i < n: d_out is compact
int g1_ntt_store(const G1Work& w, uint64_t* d_out, uint64_t n, uint64_t batch, uint64_t pitch, hipStream_t s);
// pbf_ntt_g1_bn254_batch_dev past its argument checks (wm: omega of order n, Montgomery form)
int g1_ntt_run(pbf_ctx* ctx, const U256& wm, const uint64_t* d_in, uint64_t* d_out, uint64_t n, uint64_t batch,
               int inverse, hipStream_t s);
// g1_mul.hip: (w.x + q n)[bitrev((n - i) mod n)] = [k_(q n + i)]P_i for i < n, q < batch (n >= 2 a
// power of two): the same n canonical affine points times batch x n canonical scalars, left as Xyzz
// where g1_ntt_stages (pitch n) reads the inputs of inverse transforms. The batch x n products are
// one vector: a launch is as wide as the tile whatever n. w from g1_work(ctx, ., batch n, .).
int g1_mul_xyzz_run(const G1Work& w, const uint64_t* d_points, const uint64_t* d_scalars, uint64_t n, uint64_t batch,
                    hipStream_t s);

// verify.hip, then what the single and the batched verifier (and, for pairing_tail, the KZG
// ones) state once, inline. Plonk::verify's preprocessing, shared by the single and the batched verifier:
// pre = the commitments of q_m q_l q_r q_o q_c s_sigma_1..3 (canonical affine), from the
// context's verification key when option verifier.vk allows and q, copies and the SRS equal
// their snapshots, else recomputed. omega = fr_root_of_unity(log2 n), Montgomery form.
int verifier_vk(pbf_ctx* ctx, size_t n, const U256& omega, const uint64_t* d_q, const uint64_t* d_copies,
                const uint64_t* d_srs, size_t srs_m, const uint64_t* k1k2, hipStream_t s, uint64_t pre[8][8]);
// The argument errors both verifiers share, before anything is enqueued: a null among ptrs or ok,
// then (with *ok zeroed) n not a power of two >= 8, then an SRS shorter than n.
inline int verifier_shape(std::initializer_list<const void*> ptrs, size_t n, size_t srs_m, int* ok) {
  for (const void* p : ptrs)
    if (!p) return fail(PBF_EINVAL, "null argument");
  if (!ok) return fail(PBF_EINVAL, "null argument");
  *ok = 0;
  if (n < 8 || (n & (n - 1))) return fail(PBF_EINVAL, "n must be a power of two >= 8");
  if (srs_m < n) return fail(PBF_EINVAL, "SRS too short");
  return 0;
}
// The host forms' circuit and SRS on the device (the context's vf.q, vf.copies, vf.srs), enqueued on s
inline int verifier_upload(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies, const uint64_t* srs,
                           size_t srs_m, hipStream_t s, const uint64_t** d_q, const uint64_t** d_copies,
                           const uint64_t** d_srs) {
  DevBuf &dq = ctx->buf("vf.q"), &dc = ctx->buf("vf.copies"), &dsrs = ctx->buf("vf.srs");
  int rc;
  if ((rc = dq.ensure(5 * n * 32)) || (rc = dc.ensure(3 * n * 16)) || (rc = dsrs.ensure(srs_m * 64))) return rc;
  PBF_HIP(hipMemcpyAsync(dq.p, q, 5 * n * 32, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(dc.p, copies, 3 * n * 16, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(dsrs.p, srs, srs_m * 64, hipMemcpyHostToDevice, s));
  *d_q = (const uint64_t*)dq.p, *d_copies = (const uint64_t*)dc.p, *d_srs = (const uint64_t*)dsrs.p;
  return 0;
}
// The last step of every KZG-based verifier: *ok = [e(E1, g2[1]) == e(E2, g2[0])], as the one
// check e(E1, g2[1]) e(-E2, g2[0]) == 1 (plonk.rs:646-650). e1, e2: affine G1 (8 x u64, host);
// g2 = [G2, [s]G2] (or [s^l]G2 for cells), 2 x 16 u64, host.
inline int pairing_tail(pbf_ctx* ctx, const uint64_t* e1, const uint64_t* e2, const uint64_t* g2, int* ok,
                        hipStream_t s) {
  uint64_t g1s[16], g2s[32];
  memcpy(g1s, e1, 64);
  neg_g1(e2, g1s + 8);
  memcpy(g2s, g2 + 16, 128);
  memcpy(g2s + 16, g2, 128);
  return pairing_check_on_stream(ctx, g1s, g2s, 2, ok, s);
}

// verify_batch.hip: public inputs of the _pi verifiers. pub (host, count x npub canonical values)
// against the contract of pbf.h: PBF_EINVAL for npub > n, a null pub with npub > 0, a value >= r.
int plonk_pub_validate(size_t n, const uint64_t* pub, size_t npub, size_t count);
// d_nd[2 i], d_nd[2 i + 1] = (N_i, D_i), 4 x u64 each in Montgomery form, with
// sum_{j<npub} pub_ij w^j / (z_i - w^j) = N_i / D_i for proof i < count: d_pub count x npub
// canonical values, z_i the fourth challenge of d_chal (count x 5); npub, count >= 1. D_i = 0
// exactly when z_i^n = 1 on some j < npub. PI_i(z_i) = -(z_i^n - 1) n^-1 N_i / D_i:
// k_vb_pi_partial, k_vb_pi_combine.
int plonk_pi_fraction_run(pbf_ctx* ctx, const U256& omega, const uint64_t* d_pub, uint64_t npub,
                          const uint64_t* d_chal, uint64_t count, uint64_t* d_nd, hipStream_t s);

}  // namespace pbf
