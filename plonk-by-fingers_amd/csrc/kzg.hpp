// The prover's opening machinery (prover.hip) as the KZG entry points (kzg.hip) use it: the
// geometry of the blocked synthetic division and host launchers of the prover's own kernels
// (chunked Horner evaluation, linear combination, k_hs1..3). Plonk::prove calls the same kernels
// with the same arguments as before; nothing here changes what it computes.
#pragma once
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
// evals[p] = polys[p](x) for np <= 12 device polynomials of lens[p] coefficients, at most two
// distinct points among xs (Montgomery form): k_eval_partial, k_eval_final
int fr_eval_run(const uint64_t* const* polys, const uint64_t* lens, const U256* xs, int np, DevBuf& partial,
                uint64_t* d_evals, hipStream_t s);
// out[i] = sum_k c[k] in[k][i], i < len, for k <= 10 inputs of len coefficients each (c in
// Montgomery form; an input may be `out` itself): k_lincomb
int fr_lincomb_run(const uint64_t* const* in, const U256* c, int k, uint64_t len, uint64_t* out, hipStream_t s);

}  // namespace pbf
