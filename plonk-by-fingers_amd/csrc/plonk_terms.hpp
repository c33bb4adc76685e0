// The scalar terms of Plonk::prove's rounds 4 and 5 (src/plonk.rs:401-439), stated once for the
// one-GPU and the sharded prover (prover.hip): the coefficients of the linearisation r(x) and of
// the W_z numerator as linear combinations of polynomials. Host only, every value in Montgomery
// form; each prover binds its own pointers and lengths to the coefficients.
#pragma once
#include "fr_host.hpp"

namespace pbf {

struct PlonkChallenges {
  U256 alpha, beta, gamma, z, v, k1, k2;
};
// round 4 (plonk.rs:393-399, 424): a(z) b(z) c(z) s_sigma_1(z) s_sigma_2(z) z(z w) L_1(z) t(z) r(z)
struct PlonkEvals {
  U256 a_z, b_z, c_z, s1_z, s2_z, zw_z, l1_z, t_z, r_z;
};

// r(x) = c[0] q_m + c[1] q_l + c[2] q_r + c[3] q_o + c[4] q_c + c[5] z(x) + c[6] p_7(x)
//      = q_m a_z b_z + q_l a_z + q_r b_z + q_o c_z + q_c + (K2 + K4) z(x) + r_3(x)   (plonk.rs:401-422)
// p_7 = s_sigma_3(x) in mode 1 (the paper: r_3 = -beta z_w(z) K3 s_sigma_3(x)), z(x) s_sigma_3(x)
// in mode 0 (the reference: r_3 = +beta z_w(z) K3 z(x) s_sigma_3(x), plonk.rs:414-416). e.t_z and
// e.r_z are not read.
inline void plonk_r_coeffs(const PlonkChallenges& ch, const PlonkEvals& e, int mode, U256 c[7]) {
  const U256 &alpha = ch.alpha, &beta = ch.beta, &gamma = ch.gamma;
  const U256 K2 = Fr::mul(Fr::mul(Fr::mul(Fr::add(Fr::add(e.a_z, Fr::mul(beta, ch.z)), gamma),
                                          Fr::add(Fr::add(e.b_z, Fr::mul(Fr::mul(beta, ch.k1), ch.z)), gamma)),
                                  Fr::add(Fr::add(e.c_z, Fr::mul(Fr::mul(beta, ch.k2), ch.z)), gamma)),
                          alpha);
  const U256 K3 = Fr::mul(Fr::mul(Fr::add(Fr::add(e.a_z, Fr::mul(beta, e.s1_z)), gamma),
                                  Fr::add(Fr::add(e.b_z, Fr::mul(beta, e.s2_z)), gamma)),
                          alpha);
  const U256 K4 = Fr::mul(e.l1_z, Fr::mul(alpha, alpha));
  const U256 r3 = Fr::mul(Fr::mul(beta, e.zw_z), K3);
  c[0] = Fr::mul(e.a_z, e.b_z);
  c[1] = e.a_z;
  c[2] = e.b_z;
  c[3] = e.c_z;
  c[4] = fr_one_m();
  c[5] = Fr::add(K2, K4);
  c[6] = mode == 1 ? Fr::sub(U256{}, r3) : r3;
}

// W_z (x - z) = c[0] t_lo + c[1] t_mid + c[2] t_hi + c[3] r + c[4] a + c[5] b + c[6] c
//             + c[7] s_sigma_1 + c[8] s_sigma_2 + c0
//   = t_lo + z^(n+2) t_mid + z^(2n+4) t_hi - t_z + v (r - r_z) + v^2 (a - a_z) + v^3 (b - b_z)
//     + v^4 (c - c_z) + v^5 (s1 - s1_z) + v^6 (s2 - s2_z)                         (plonk.rs:430-439)
// for n gates; returns the constant term c0.
inline U256 plonk_wz_coeffs(const PlonkChallenges& ch, const PlonkEvals& e, uint64_t n, U256 c[9]) {
  U256 vp[7];
  vp[0] = fr_one_m();
  for (int i = 1; i < 7; ++i) vp[i] = Fr::mul(vp[i - 1], ch.v);
  c[0] = vp[0];
  c[1] = fr_pow(ch.z, n + 2);
  c[2] = fr_pow(ch.z, 2 * n + 4);
  for (int i = 1; i < 7; ++i) c[2 + i] = vp[i];
  U256 cst = Fr::add(e.t_z, Fr::mul(vp[1], e.r_z));
  cst = Fr::add(cst, Fr::mul(vp[2], e.a_z));
  cst = Fr::add(cst, Fr::mul(vp[3], e.b_z));
  cst = Fr::add(cst, Fr::mul(vp[4], e.c_z));
  cst = Fr::add(cst, Fr::mul(vp[5], e.s1_z));
  cst = Fr::add(cst, Fr::mul(vp[6], e.s2_z));
  return Fr::sub(U256{}, cst);
}

}  // namespace pbf
