// The fixed-window product [k]Q of the G1 NTT's butterflies (g1_ntt.hip) and of the pointwise
// product (g1_mul.hip), and the 128-bit point loads and stores both use. Device code only.
#pragma once
#include <cstring>
#include "prover.hpp"

namespace pbf {

constexpr int GN_T = 64;          // lanes per workgroup: one wave, one product per lane
constexpr int GN_ENT = 15;        // table entries per product: 1Q .. 15Q

__device__ __forceinline__ Xyzz ld_pt(const Xyzz* p) {
  const uint4* s = (const uint4*)p;
  uint4 v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = s[i];
  Xyzz r;
  memcpy(&r, v, sizeof(Xyzz));
  return r;
}
__device__ __forceinline__ void st_pt(Xyzz* p, const Xyzz& r) {
  uint4 v[8];
  memcpy(v, &r, sizeof(Xyzz));
  uint4* d = (uint4*)p;
#pragma unroll
  for (int i = 0; i < 8; ++i) d[i] = v[i];
}

// [k]Q for the canonical scalar at k (8 x u32 in memory); tbl: this lane's first table entry,
// the others `stride` points apart
__device__ __forceinline__ Xyzz g1_mul_win(const Xyzz& Q, const uint32_t* k, Xyzz* tbl, uint64_t stride) {
  if (G1::is_identity(Q)) return Q;
  st_pt(tbl, Q);
  Xyzz acc = G1::dbl2(Q);
  st_pt(tbl + stride, acc);
#pragma unroll 1
  for (int e = 2; e < GN_ENT; ++e) {
    acc = G1::add2(acc, Q);
    st_pt(tbl + e * stride, acc);
  }
  acc = G1::identity();
#pragma unroll 1
  for (int i = 63; i >= 0; --i) {
#pragma unroll 1
    for (int d = 0; d < 4; ++d) acc = G1::dbl2(acc);  // the identity returns at once
    const uint32_t digit = (k[i >> 3] >> ((i & 7) * 4)) & 15u;
    if (digit) acc = G1::add2(acc, ld_pt(tbl + (digit - 1) * stride));
  }
  return acc;
}

// the canonical affine point at p (8 x u64, (0,0) the identity) as Xyzz
__device__ __forceinline__ Xyzz ld_affine(const uint64_t* p) {
  uint64_t l[8], any = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) any |= (l[k] = p[k]);
  Xyzz r = G1::identity();
  if (any) {
    Affine a;
    a.x = Fq::to_mont(u256_from_u64(l));
    a.y = Fq::to_mont(u256_from_u64(l + 4));
    r = G1::from_affine(a);
  }
  return r;
}
// and back: the unique canonical affine form
__device__ __forceinline__ void st_affine(uint64_t* out, const Xyzz& p) {
  U256 ax, ay;
  G1::to_affine_plain(p, &ax, &ay);
  u256_to_u64(ax, out);
  u256_to_u64(ay, out + 4);
}

}  // namespace pbf
