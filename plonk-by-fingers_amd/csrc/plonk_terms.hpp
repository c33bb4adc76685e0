// The scalar terms of the protocol, each stated once for the code paths that need it. Every value
// is in Montgomery form.
//   Plonk::prove's rounds 4 and 5 (src/plonk.rs:401-439), for the one-GPU and the sharded prover
//   (prover.hip): the coefficients of the linearisation r(x) and of the W_z numerator as linear
//   combinations of polynomials; each prover binds its own pointers and lengths to them. Host only.
//   Plonk::verify's steps 4-10 (src/plonk.rs:549-634), for the single verifier on the host
//   (verify.hip) and the batched one on the device (verify_batch.hip k_vb_scalars): the 18 MSM
//   scalars and the 2 of E1 from a proof's evaluations and challenges. Host and device.
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

// ---------------------------------------------------------------- Plonk::verify steps 4-10
// The Fr product as a call: the verifier's scalars are ~120 products of straight line, and the
// device keeps one copy of the product's code per kernel.
__host__ __device__ __noinline__ inline U256 fmul(U256 a, U256 b) { return Fr::mul(a, b); }
// a^(r-2): Fermat inverse (a != 0) over fmul
__host__ __device__ inline U256 fmul_inv(const U256& a, const U256& one) {
  U256 r = one;
#pragma unroll 1
  for (int i = 255; i >= 0; --i) {
    r = fmul(r, r);
    const uint32_t e = Bn254FrParams::P[i / 32] - (i < 32 ? 2u : 0u);
    if ((e >> (i % 32)) & 1) r = fmul(r, a);
  }
  return r;
}

// The domain of n = 2^log_n gates: omega = fr_root_of_unity(log_n) of order n, and n^-1
struct PlonkDomain {
  uint32_t log_n;
  U256 omega, n_inv;
};
inline PlonkDomain plonk_domain(uint64_t n) {
  PlonkDomain d{};
  while (((uint64_t)1 << d.log_n) < n) ++d.log_n;
  d.omega = fr_root_of_unity(d.log_n);
  d.n_inv = fr_inv(hm64(n));
  return d;
}

// what the verifier's scalars take besides the challenges and the proof: the verifier's random u
// (plonk.rs:519) and the batching weight rho (1 for a proof on its own)
struct PlonkVerifierArgs {
  U256 u, rho;
  PlonkDomain dom;
  int mode;
};

// Steps 4-10 for one proof as the scalars of one linear combination of points, every one times rho.
// Each is handed to out(j, value) as soon as it is known, j in the order
//   0 .. 8    on the proof's a b c z t_lo t_mid t_hi w_z w_zw:
//             rho (v^2, v^3, v^4, d_2, 1, z^(n+2), z^(2n+4), z, u z omega)
//   9, 10     of E1 = W_z + u W_zw: rho, rho u
//   11 .. 19  on the shared bases q_m q_l q_r q_o q_c s1 s2 s3 G:
//             rho (v a_z b_z, v a_z, v b_z, v c_z, v, v^5, v^6, -d_3, -E)
// so the caller decides where and in which form they are kept, and the device holds none longer
// than its store takes. e.l1_z and e.t_z are not read: L_1(z) = (z^n - 1) / (n (z - 1)) and step 7's
// t_z come from here. pi_nd: null, or the public inputs' fraction (N, D) in Montgomery form as
// plonk_pi_fraction_run stores it (2 x 4 u64), read where it is used:
// sum_j pub_j w^j / (z - w^j) = N / D, D != 0 for z outside H; step 7 then takes r_z + PI(z),
// PI(z) = -Z_H(z) n^-1 N / D. mode 0 keeps the reference's step 7 (plonk.rs:575-581, no alpha on
// the permutation term), mode 1 the paper's.
// Returns false with no output when Z_H(z) = 0, where the reference's .unwrap() would panic
// (plonk.rs:581); z = 1 is such a z, so one inversion of Z_H(z) (z - 1) [D] serves every quotient.
template <class Out>
__host__ __device__ __forceinline__ bool plonk_verifier_scalars(const PlonkChallenges& ch, const PlonkEvals& e,
                                                                const PlonkVerifierArgs& g, const uint64_t* pi_nd,
                                                                Out out) {
  const U256 one = fr_one_m();
  const U256 &alpha = ch.alpha, &beta = ch.beta, &gamma = ch.gamma, &zc = ch.z, &v = ch.v, &u = g.u, &rho = g.rho;
  // Step 4: Z_H(z) = z^n - 1
  U256 zn = zc;
#pragma unroll 1
  for (uint32_t k = 0; k < g.dom.log_n; ++k) zn = fmul(zn, zn);
  const U256 z_h_z = Fr::sub(zn, one);
  if (Fr::is_zero(z_h_z)) return false;
  // Step 5: L_1(z), with 1 / Z_H(z) and 1 / D from the same inversion
  const U256 zm1 = Fr::sub(zc, one);
  const U256 zhm = fmul(z_h_z, zm1);
  U256 tinv, rpi_z = e.r_z;  // r_z + PI(z)
  if (pi_nd) {
    const U256 piN = u256_from_u64(pi_nd), piD = u256_from_u64(pi_nd + 4);
    const U256 all = fmul_inv(fmul(zhm, piD), one);
    tinv = fmul(all, piD);
    rpi_z = Fr::sub(e.r_z, fmul(fmul(fmul(z_h_z, g.dom.n_inv), piN), fmul(all, zhm)));
  } else {
    tinv = fmul_inv(zhm, one);
  }
  const U256 inv_zh = fmul(tinv, zm1);
  const U256 l1 = fmul(fmul(z_h_z, fmul(tinv, z_h_z)), g.dom.n_inv);
  // Step 7: t_z
  const U256 alpha2 = fmul(alpha, alpha);
  const U256 l1a2 = fmul(l1, alpha2);
  const U256 pa = Fr::add(Fr::add(e.a_z, fmul(beta, e.s1_z)), gamma);
  const U256 pb = Fr::add(Fr::add(e.b_z, fmul(beta, e.s2_z)), gamma);
  const U256 pab = fmul(pa, pb);
  U256 perm = fmul(pab, fmul(Fr::add(e.c_z, gamma), e.zw_z));
  if (g.mode == 1) perm = fmul(perm, alpha);
  const U256 t_z = fmul(Fr::sub(Fr::sub(rpi_z, perm), l1a2), inv_zh);
  // Steps 8-10
  U256 vp[7];
  vp[0] = one;
  for (int k = 1; k < 7; ++k) vp[k] = fmul(vp[k - 1], v);
  const U256 bz = fmul(beta, zc);
  const U256 d2 = Fr::add(
      Fr::add(fmul(fmul(fmul(fmul(Fr::add(Fr::add(e.a_z, bz), gamma), Fr::add(Fr::add(e.b_z, fmul(bz, ch.k1)), gamma)),
                             Fr::add(Fr::add(e.c_z, fmul(bz, ch.k2)), gamma)),
                        alpha),
                   v),
              fmul(l1a2, v)),
      u);
  const U256 d3 = fmul(fmul(fmul(fmul(pab, alpha), v), beta), e.zw_z);
  U256 ecoef = Fr::add(t_z, fmul(v, e.r_z));
  ecoef = Fr::add(ecoef, fmul(vp[2], e.a_z));
  ecoef = Fr::add(ecoef, fmul(vp[3], e.b_z));
  ecoef = Fr::add(ecoef, fmul(vp[4], e.c_z));
  ecoef = Fr::add(ecoef, fmul(vp[5], e.s1_z));
  ecoef = Fr::add(ecoef, fmul(vp[6], e.s2_z));
  ecoef = Fr::add(ecoef, fmul(u, e.zw_z));
  const U256 zn2 = fmul(zn, fmul(zc, zc));  // z^(n+2)
  out(0, fmul(rho, vp[2]));                   // a_s
  out(1, fmul(rho, vp[3]));                   // b_s
  out(2, fmul(rho, vp[4]));                   // c_s
  out(3, fmul(rho, d2));                      // z_s
  out(4, rho);                                // t_lo
  out(5, fmul(rho, zn2));                     // t_mid
  out(6, fmul(rho, fmul(zn2, zn2)));          // t_hi: z^(2n+4)
  out(7, fmul(rho, zc));                      // w_z * z
  const U256 ru = fmul(rho, u);
  out(8, fmul(ru, fmul(zc, g.dom.omega)));        // w_zw * u z w
  out(9, rho);
  out(10, ru);
  const U256 rv = fmul(rho, v);
  out(11, fmul(rv, fmul(e.a_z, e.b_z)));      // q_m
  out(12, fmul(rv, e.a_z));                   // q_l
  out(13, fmul(rv, e.b_z));                   // q_r
  out(14, fmul(rv, e.c_z));                   // q_o
  out(15, rv);                                // q_c
  out(16, fmul(rho, vp[5]));                  // s1
  out(17, fmul(rho, vp[6]));                  // s2
  out(18, Fr::sub(U256{}, fmul(rho, d3)));    // - s3 d3
  out(19, Fr::sub(U256{}, fmul(rho, ecoef))); // - E
  return true;
}

}  // namespace pbf
