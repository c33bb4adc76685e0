// What prover.hip exports to the KZG entry points (kzg.hip) and the verifiers (verify.hip,
// verify_batch.hip): the geometry of the blocked synthetic division and host launchers of the
// prover's own kernels (chunked Horner evaluation, linear combination, k_hs1..3, the H powers and
// sigma labels). Plonk::prove goes through the same launchers.
#pragma once
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

// verify.hip: Plonk::verify's preprocessing, shared by the single and the batched verifier:
// pre = the commitments of q_m q_l q_r q_o q_c s_sigma_1..3 (canonical affine), from the
// context's verification key when option verifier.vk allows and q, copies and the SRS equal
// their snapshots, else recomputed. omega = fr_root_of_unity(log2 n), Montgomery form.
int verifier_vk(pbf_ctx* ctx, size_t n, const U256& omega, const uint64_t* d_q, const uint64_t* d_copies,
                const uint64_t* d_srs, size_t srs_m, const uint64_t* k1k2, hipStream_t s, uint64_t pre[8][8]);

}  // namespace pbf
