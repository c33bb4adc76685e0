// One copy of the small BN254 helpers every unit's host code needs: Fr values in and out of
// Montgomery form, powers and the Fermat inverse, the root of unity, the canonical test, and the
// two G1 checks of the verifiers. fr_one_m, fr_pow, fr_inv and hout are also what kernels call
// (the prover's, the batched verifier's). Everything takes and returns Montgomery form unless it
// says canonical.
#pragma once
#include <cstddef>
#include <cstdint>
#include "fp256.hpp"

namespace pbf {

__host__ __device__ __forceinline__ U256 fr_one_m() { return Fr::to_mont(Fr::one_plain()); }

// a^e
__host__ __device__ inline U256 fr_pow(U256 a, uint64_t e) {
  U256 r = fr_one_m();
  while (e) {
    if (e & 1) r = Fr::mul(r, a);
    a = Fr::mul(a, a);
    e >>= 1;
  }
  return r;
}
// a^(r-2): Fermat inverse (a != 0)
__host__ __device__ inline U256 fr_inv(const U256& a) {
  U256 r = fr_one_m();
  for (int i = 255; i >= 0; --i) {
    r = Fr::mul(r, r);
    uint32_t e = Bn254FrParams::P[i / 32] - (i < 32 ? 2u : 0u);
    if ((e >> (i % 32)) & 1) r = Fr::mul(r, a);
  }
  return r;
}
// out of Montgomery form, to 4 little-endian u64 limbs (canonical)
__host__ __device__ __forceinline__ void hout(uint64_t* p, const U256& m) { u256_to_u64(Fr::from_mont(m), p); }

// ---------------------------------------------------------------- host only
// 4 little-endian u64 limbs (any 256-bit value, reduced mod r) / a u64, to Montgomery form
inline U256 hm(const uint64_t* p) { return Fr::to_mont(u256_from_u64(p)); }
inline U256 hm64(uint64_t v) {
  U256 r{};
  r.w[0] = (uint32_t)v;
  r.w[1] = (uint32_t)(v >> 32);
  return Fr::to_mont(r);
}
inline U256 hpowm(U256 a, const U256& e_plain) {  // exponent given as plain U256
  U256 r = fr_one_m();
  for (int i = 255; i >= 0; --i) {
    r = Fr::mul(r, r);
    if ((e_plain.w[i / 32] >> (i % 32)) & 1) r = Fr::mul(r, a);
  }
  return r;
}
inline bool heq1(const U256& m) { return Fr::eq(m, fr_one_m()); }
// primitive 2^k-th root of unity of Fr: 5^((r-1)/2^k)
inline U256 fr_root_of_unity(uint32_t log_n) {
  U256 e;  // (r-1) >> log_n
  for (int i = 0; i < 8; ++i) e.w[i] = Bn254FrParams::P[i];
  e.w[0] -= 1;
  for (uint32_t s = 0; s < log_n; ++s) {
    for (int i = 0; i < 8; ++i) e.w[i] = (e.w[i] >> 1) | (i < 7 ? (e.w[i + 1] << 31) : 0);
  }
  return hpowm(hm64(5), e);
}

// canonical Fr (below r): one value of 4 u64 limbs, or every one of count
inline bool fr_canonical(const uint64_t* p) { return !Fr::geq_p(u256_from_u64(p)); }
inline bool fr_canonical(const uint64_t* p, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (!fr_canonical(p + 4 * i)) return false;
  return true;
}

// y^2 == x^3 + 3 over Fq for an affine canonical point (identity (0,0) accepted: G1P::in_curve)
inline bool on_curve(const uint64_t* p) {
  bool zero = true;
  for (int i = 0; i < 8; ++i) zero = zero && p[i] == 0;
  if (zero) return true;
  const U256 x = u256_from_u64(p), y = u256_from_u64(p + 4);
  if (Fq::geq_p(x) || Fq::geq_p(y)) return false;
  const U256 xm = Fq::to_mont(x), ym = Fq::to_mont(y);
  U256 three{};
  three.w[0] = 3;
  const U256 rhs = Fq::add(Fq::mul(Fq::mul(xm, xm), xm), Fq::to_mont(three));
  return Fq::eq(Fq::mul(ym, ym), rhs);
}
// (x, q - y), the identity unchanged
inline void neg_g1(const uint64_t* p, uint64_t* out) {
  for (int i = 0; i < 8; ++i) out[i] = p[i];
  const U256 y = u256_from_u64(p + 4);
  if (Fq::is_zero(y)) return;
  U256 d;
  uint64_t borrow = 0;
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)Bn254FqParams::P[i] - y.w[i] - borrow;
    d.w[i] = (uint32_t)t;
    borrow = (t >> 63) & 1;
  }
  u256_to_u64(d, out + 4);
}

}  // namespace pbf
