// Generalised PLONK prover over BN254 on gfx950 — BASELINE config 5 and the §8(f) rows:
// Plonk::prove (src/plonk.rs:191-466) for any power-of-two number of gates n, with every
// O(n^2)/O(n^3) step of the reference replaced by an equivalent O(n log n) one:
//
//   interpolate_at_h (Vandermonde inverse, plonk.rs:177-179)   -> batched INTT
//   round-2 accumulator (per-row s_sigma.eval, plonk.rs:278-299) -> sigma labels +
//        batch inversion + prefix product (the values s_sigma_k(w^j) ARE sigma_k[j])
//   t(x) = (t1 + t2 - t3 + t4) / Z_H (Poly mul/div, plonk.rs:339-370) -> 13 coset NTTs of
//        size 4n, one pointwise quotient kernel (Z_H(x) = x^n - 1 takes 4 values on the
//        coset), one coset INTT; the division's `rem == 0` assert becomes "coefficients
//        3n+6 .. 4n-1 of t are zero" (also the 3-way split's precondition, plonk.rs:376-378
//        generalised to n+2 coefficients per part)
//   evaluations at z (Poly::eval, plonk.rs:393-399)              -> chunked Horner + reduction
//   W_z, W_zw (Poly::div by x - z, plonk.rs:430-442)             -> blocked synthetic division
//        on the coefficients (k_hs1..3); the remainder must be zero
//   SRS::eval_at_s commitments (plonk.rs:51-58)                 -> Pippenger MSM (msm.hip)
//
// Every output is the unique mathematical value the reference's formulas define (the
// same polynomials, evaluations and group elements), so results are bit-identical to a
// literal restatement (oracle/plonk_bn254.py). mode 0 keeps the reference's r_3(x)
// (plonk.rs:414-416: z(x) * s_sigma_3(x) * ..., product computed on the coset); mode 1
// uses the linearisation its verifier checks.
//
// Field elements at rest in HBM: canonical Fr, 4 x u64 little-endian (the ABI layout);
// kernels convert to Montgomery on load and back on store.
//
// Layout: the Fr polynomial kernels and their launchers (prover.hpp exports the ones kzg.hip and
// verify.hip share), the Prover helper struct, then Plonk::prove as prove_setup and its two
// siblings prove_single and prove_sharded, which take the protocol's scalar terms from
// plonk_terms.hpp; the synthetic circuit and the SRS at the end. The verifier is verify.hip.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <vector>
#include "../../include/pbf.h"
#include "prover.hpp"
#include "transcript.hpp"
#include "plonk_terms.hpp"
#include "fr29.hpp"

// ntt256.hip: the coset transforms' batched forward NTT of zero-padded prefixes
int pbf_internal_ntt_fr256_prefix(pbf_ctx* ctx, const uint64_t* omega, uint64_t* d_io, size_t n, size_t batch,
                                  size_t in_len, hipStream_t s);

namespace pbf {

__device__ __forceinline__ U256 ldr(const uint64_t* p) { return Fr::to_mont(u256_from_u64(p)); }
__device__ __forceinline__ void str(uint64_t* p, const U256& m) { u256_to_u64(Fr::from_mont(m), p); }

constexpr int PV_CHUNK = 32;  // elements per thread in the chunked kernels

static uint32_t blocks_for(uint64_t threads) {
  uint64_t b = (threads + 255) / 256;
  return (uint32_t)(b ? b : 1);
}

// Chunked kernels: the wave of thread t owns 64 * PV_CHUNK consecutive elements and lane l
// takes i = first + 64 k (k < PV_CHUNK), so every load and store instruction of the wave
// touches consecutive elements; a running power steps by base^64.
__device__ __forceinline__ uint64_t chunk_first(uint64_t t) { return (t / 64) * 64 * PV_CHUNK + (t % 64); }
__device__ __forceinline__ U256 pow64(U256 b) {
#pragma unroll
  for (int i = 0; i < 6; ++i) b = Fr::mul(b, b);
  return b;
}

// out[m] = (j = in_off + in_stride m) < len ? in[j] * base^(e_off + e_mult m) : 0, m < count
// (coset scaling with zero padding; with in_stride = e_mult = G, in_off = e_off = rank it
// extracts rank's stride shard of the scaled vector). The product of a canonical value and
// a Montgomery-form power is the canonical product (a * xR * R^-1): no conversions.
// c0 (Montgomery form, folded into x0 by the host): an extra constant factor of every output --
// the quotient's circuit slots come out at a chosen R-degree this way, for free (see QuotArgs)
// Round 4: a thread's first power c0 base^(e_off + e_mult i0), i0 = 64 PV_CHUNK v + l (wave v,
// lane l), comes from host-computed tables instead of two square-and-multiply chains per thread
// (~80 dependent products, which were most of the kernel's time at 2^20 gates): x0 = c0
// base^e_off, tl[l] = base^(e_mult l), tv[k] = base^(e_mult 64 PV_CHUNK 2^k) for the set bits k
// of v, step = base^(64 e_mult).
constexpr int SP_WBITS = 27;  // waves < 2^27
struct ScalePow {
  U256 x0, step;
  U256 tl[64];
  U256 tv[SP_WBITS];
};
__global__ void k_scale_pow(const uint64_t* in, uint64_t in_off, uint64_t in_stride, uint64_t len, uint64_t* out,
                            uint64_t count, ScalePow sp) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t i0 = chunk_first(t);
  if (i0 >= count) return;
  if (in_off + in_stride * i0 >= len) {  // the whole chunk is zero padding (j grows with i): no powers
    for (uint64_t i = i0, k = 0; k < PV_CHUNK && i < count; ++k, i += 64)
      for (int q = 0; q < 4; ++q) out[4 * i + q] = 0;
    return;
  }
  U256 x = Fr::mul_tp(sp.x0, sp.tl[t % 64]);
  for (uint64_t v = t / 64, k = 0; v; v >>= 1, ++k)
    if (v & 1) x = Fr::mul_tp(x, sp.tv[k]);
  const U256 step = sp.step;
  for (uint64_t i = i0, k = 0; k < PV_CHUNK && i < count; ++k, i += 64) {
    const uint64_t j = in_off + in_stride * i;
    if (j < len) u256_to_u64(Fr::mul_tp(u256_from_u64(in + 4 * j), x), out + 4 * i);
    else for (int q = 0; q < 4; ++q) out[4 * i + q] = 0;
    x = Fr::mul_tp(x, step);
  }
}

// Evaluation-domain layout of a rank's blocks in the stride-sharded NTT (multigpu, SURVEY.md
// §8e): local position p = q*S + kk holds global index q*nl + rank*S + kk. G = 1: p itself.
struct Blk {
  uint64_t nl, S, rank;
  uint32_t G;
};
__device__ __forceinline__ uint64_t blk_index(const Blk& b, uint64_t p) {
  return b.G == 1 ? p : (p / b.S) * b.nl + b.rank * b.S + (p % b.S);
}
// x_{i(p)} = g w^{i(p)} for the chunked kernels: advance the running point by w^64 inside a
// block, recompute it where p + 64 starts a new block
__device__ __forceinline__ U256 blk_next_x(const Blk& b, uint64_t p, const U256& x, const U256& step, const U256& g,
                                           const U256& w) {
  if (b.G == 1 || (p + 64) / b.S == p / b.S) return Fr::mul_tp(x, step);
  return Fr::mul_tp(g, fr_pow(w, blk_index(b, p + 64)));
}

// the start-power tables of x0 base^(e_off + e_mult i) (k_scale_pow, k_powers29), host products
static ScalePow scale_pow_tab(const U256& x0, const U256& base, uint64_t e_off, uint64_t e_mult) {
  ScalePow sp;
  sp.x0 = Fr::mul(x0, fr_pow(base, e_off));
  sp.step = fr_pow(base, 64 * e_mult);
  const U256 bm = fr_pow(base, e_mult);
  sp.tl[0] = fr_one_m();
  for (int l = 1; l < 64; ++l) sp.tl[l] = Fr::mul(sp.tl[l - 1], bm);
  sp.tv[0] = fr_pow(sp.step, PV_CHUNK);
  for (int k = 1; k < SP_WBITS; ++k) sp.tv[k] = Fr::mul(sp.tv[k - 1], sp.tv[k - 1]);
  return sp;
}
static ScalePow powers_tab(const U256& base, const U256& start) { return scale_pow_tab(start, base, 0, 1); }

// copy_constraints_to_roots (plonk.rs:181-189): sigma[col][i] = {w^j, k1 w^j, k2 w^j}[kind]
// Rows [row0, row0 + rows) of every column; sigma[col][i - row0] (the whole table: 0, n)
__global__ void k_sigma(const uint64_t* copies, const uint64_t* hpow, uint64_t n, uint64_t row0, uint64_t rows, U256 k1,
                        U256 k2, uint64_t* sigma, int* bad) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * rows) return;
  const uint64_t col = t / rows, id = t;
  const uint64_t src = col * n + row0 + t % rows;
  const uint64_t kind = copies[2 * src], idx = copies[2 * src + 1];
  if (kind > 2 || idx < 1 || idx > n) {
    *bad = 1;
    for (int k = 0; k < 4; ++k) sigma[4 * id + k] = 0;
    return;
  }
  U256 h = u256_from_u64(hpow + 4 * (idx - 1));  // canonical; k1, k2 Montgomery: products canonical
  if (kind == 1) h = Fr::mul_tp(h, k1);
  if (kind == 2) h = Fr::mul_tp(h, k2);
  u256_to_u64(h, sigma + 4 * id);
}

// k_sigma for the blocked rows of a sharded NTT's rank r: out[col][q Sn + kk] = sigma of row
// q B + r Sn + kk (B = n / G, Sn = B / G), the evaluation layout pbf_ntt_fr256_shard_* use
__global__ void k_sigma_blk(const uint64_t* copies, const uint64_t* hpow, uint64_t n, uint64_t B, uint64_t Sn,
                            uint64_t r, U256 k1, U256 k2, uint64_t* out, int* bad) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * B) return;
  const uint64_t col = t / B, p = t % B;
  const uint64_t row = (p / Sn) * B + r * Sn + p % Sn;
  const uint64_t kind = copies[2 * (col * n + row)], idx = copies[2 * (col * n + row) + 1];
  if (kind > 2 || idx < 1 || idx > n) {
    *bad = 1;
    for (int k = 0; k < 4; ++k) out[4 * t + k] = 0;
    return;
  }
  U256 h = u256_from_u64(hpow + 4 * (idx - 1));
  if (kind == 1) h = Fr::mul_tp(h, k1);
  if (kind == 2) h = Fr::mul_tp(h, k2);
  u256_to_u64(h, out + 4 * t);
}

// Constrains::satisfies (constraints.rs:198-230, with its q_l * b term): gates and copies.
// PI (pbf_plonk_prove_bn254_pi*): rows i < npub check ... + q_c - pub_i = 0; a pub_i >= r sets bad[1]
// (the _dev form's pub is on the device: this is its canonical check). PI = false is the
// kernel of the plain entries, which pass pub = null and npub = 0.
template <bool PI>
__global__ void k_satisfies(const uint64_t* q, const uint64_t* abc, const uint64_t* copies, uint64_t n, uint64_t row0,
                            uint64_t rows, const uint64_t* pub, uint64_t npub, int* bad) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows) return;
  const uint64_t i = row0 + t;
  // every term at R-degree -1 (the zero test does not depend on the degree): canonical
  // products of two canonical values; q_m lifted to degree 1, q_c lowered to -1
  auto ld = [](const uint64_t* p) { return u256_from_u64(p); };
  const U256 ql = ld(q + 4 * i), qo = ld(q + 4 * (2 * n + i)), qm = Fr::to_mont(ld(q + 4 * (3 * n + i))),
             qc = Fr::from_mont(ld(q + 4 * (4 * n + i)));
  const U256 a = ld(abc + 4 * i), b = ld(abc + 4 * (n + i)), c = ld(abc + 4 * (2 * n + i));
  U256 r = Fr::add(Fr::mul_tp(ql, a), Fr::mul_tp(ql, b));
  r = Fr::add(r, Fr::mul_tp(qo, c));
  r = Fr::add(r, Fr::mul_tp(Fr::mul_tp(qm, a), b));
  r = Fr::add(r, qc);
  if (PI && i < npub) {
    const U256 p = ld(pub + 4 * i);
    if (Fr::geq_p(p)) atomicOr(bad + 1, 1);  // its own word: the plain stores below do not touch it
    else r = Fr::sub(r, Fr::from_mont(p));   // lowered to degree -1, as q_c
  }
  if (!Fr::is_zero(r)) *bad = 1;
  for (int col = 0; col < 3; ++col) {
    const uint64_t kind = copies[2 * (col * n + i)], idx = copies[2 * (col * n + i) + 1];
    if (kind > 2 || idx < 1 || idx > n) { *bad = 1; continue; }
    const uint64_t* v = abc + 4 * (kind * n + idx - 1);
    const uint64_t* w = abc + 4 * (col * n + i);
    if (v[0] != w[0] || v[1] != w[1] || v[2] != w[2] || v[3] != w[3]) *bad = 1;
  }
}

// round 2 terms (plonk.rs:282-297) for row j < n-1: num_j = dend, den_j = dsor.
// Conversion-free (R-degrees as in QuotArgs): canonical a b c w sigma, beta k1 k2 in
// Montgomery form (degree 1), gamma0 canonical: each factor lands at degree 0, each
// three-factor product at degree -2 -- num and den alike, and k_div_batch takes them so.
// Rows j = row0 + t, t < rows (and j < n - 1): num[t], den[t]; sigma as k_sigma wrote it for
// the same rows (column stride `rows`)
__global__ void __launch_bounds__(256) k_perm_terms(const uint64_t* abc, const uint64_t* sigma, const uint64_t* hpow, uint64_t n,
                                                    uint64_t row0, uint64_t rows, U256 beta, U256 gamma0, U256 k1, U256 k2,
                                                    uint64_t* num, uint64_t* den) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t j = row0 + t;
  if (t >= rows || j + 1 >= n) return;
  auto ld = [](const uint64_t* p) { return u256_from_u64(p); };
  const U256 a = ld(abc + 4 * j), b = ld(abc + 4 * (n + j)), c = ld(abc + 4 * (2 * n + j));
  const U256 w = ld(hpow + 4 * j);
  const U256 bw = Fr::mul_tp(beta, w);
  U256 d1 = Fr::add(Fr::add(a, bw), gamma0);
  U256 d2 = Fr::add(Fr::add(b, Fr::mul_tp(bw, k1)), gamma0);
  U256 d3 = Fr::add(Fr::add(c, Fr::mul_tp(bw, k2)), gamma0);
  u256_to_u64(Fr::mul_tp(Fr::mul_tp(d1, d2), d3), num + 4 * t);
  U256 e1 = Fr::add(Fr::add(a, Fr::mul_tp(beta, ld(sigma + 4 * t))), gamma0);
  U256 e2 = Fr::add(Fr::add(b, Fr::mul_tp(beta, ld(sigma + 4 * (rows + t)))), gamma0);
  U256 e3 = Fr::add(Fr::add(c, Fr::mul_tp(beta, ld(sigma + 4 * (2 * rows + t)))), gamma0);
  u256_to_u64(Fr::mul_tp(Fr::mul_tp(e1, e2), e3), den + 4 * t);
}

// out[i] = num[i] / den[i] by Montgomery's trick (one Fermat inverse per chunk); a zero
// denominator sets *bad (the reference's `.unwrap()`, plonk.rs:297). num and den are read as
// stored: with both at R-degree e the quotient comes out at degree 1 (the Montgomery inverse of a
// degree-e value is at degree 2 - e), which the final from_mont turns canonical. num == null:
// 1 / den (den at degree 1).
// The chunk is spread over a wave (round 6): lane l of a wave takes the elements blk + 64 k + l,
// k < chunk (coalesced), and keeps its running prefix products in `pre` (count elements of
// scratch) instead of a per-thread array of 32 (which hipcc had placed in scratch memory); the
// chunk grows with the count (fewer Fermat inversions: 3 + 380 / chunk products per element)
// while leaving >= 2048 waves.
__global__ void __launch_bounds__(256) k_div_batch_w(const uint64_t* num, const uint64_t* den, uint64_t* out,
                                                     uint64_t* pre, uint64_t count, uint32_t chunk, int* bad) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t lane = g & 63, blk = (g >> 6) * 64 * (uint64_t)chunk;
  if (blk >= count) return;
  U256 acc = fr_one_m();
  for (uint32_t k = 0; k < chunk; ++k) {
    const uint64_t i = blk + 64 * (uint64_t)k + lane;
    if (i >= count) break;
    const U256 d = u256_from_u64(den + 4 * i);
    if (Fr::is_zero(d)) { *bad = 1; return; }
    u256_to_u64(acc, pre + 4 * i);
    acc = Fr::mul_tp(acc, d);
  }
  U256 inv = fr_inv(acc);  // 1 / prod (1 for a lane with no element)
  for (int k = (int)chunk - 1; k >= 0; --k) {
    const uint64_t i = blk + 64 * (uint64_t)k + lane;
    if (i >= count) continue;
    const U256 d = u256_from_u64(den + 4 * i);
    const U256 dinv = Fr::mul_tp(inv, u256_from_u64(pre + 4 * i));  // 1 / d_i
    inv = Fr::mul_tp(inv, d);
    str(out + 4 * i, num ? Fr::mul_tp(u256_from_u64(num + 4 * i), dinv) : dinv);
  }
}
// chunk of k_div_batch_w: the largest of 32, 64, 128 that leaves >= 2048 waves (2^24 rows: 64)
static uint32_t div_chunk(uint64_t count) {
  uint32_t c = 32;
  while (c < 128 && (uint64_t)c * 2 * 64 * 2048 <= count) c *= 2;
  return c;
}
static int div_batch(pbf_ctx* ctx, const uint64_t* num, const uint64_t* den, uint64_t* out, uint64_t count, int* bad,
                     hipStream_t s) {
  if (!count) return 0;
  DevBuf& pb = ctx->buf("pv.divpre");
  int rc = pb.ensure(count * 32);
  if (rc) return rc;
  const uint32_t ch = div_chunk(count);
  const uint64_t waves = (count + 64ull * ch - 1) / (64ull * ch);
  hipLaunchKernelGGL(k_div_batch_w, dim3(blocks_for(waves * 64)), dim3(256), 0, s, num, den, out, (uint64_t*)pb.p,
                     count, ch, bad);
  PBF_HIP(hipGetLastError());
  return 0;
}

// ---- exclusive prefix product: out[0] = 1, out[i] = prod_{j<i} in[j]  (i < count)
constexpr int SCAN_T = 256, SCAN_PER = 8, SCAN_BLK = SCAN_T * SCAN_PER;

__device__ void block_scan_mul(U256* sh, int t) {  // inclusive Hillis-Steele over SCAN_T
  for (int off = 1; off < SCAN_T; off <<= 1) {
    U256 v = sh[t];
    if (t >= off) v = Fr::mul_tp(sh[t - off], v);
    __syncthreads();
    sh[t] = v;
    __syncthreads();
  }
}

// phase 1: block-local inclusive products (in place into out), block totals
__global__ void __launch_bounds__(SCAN_T) k_scan1(const uint64_t* in, uint64_t* out, uint64_t count, uint64_t* totals) {
  __shared__ U256 sh[SCAN_T];
  const int t = threadIdx.x;
  const uint64_t base = (uint64_t)blockIdx.x * SCAN_BLK + (uint64_t)t * SCAN_PER;
  U256 v[SCAN_PER];
  U256 acc = fr_one_m();
  for (int k = 0; k < SCAN_PER; ++k) {
    const uint64_t i = base + k;
    const U256 x = i < count ? ldr(in + 4 * i) : fr_one_m();
    acc = Fr::mul_tp(acc, x);
    v[k] = acc;
  }
  sh[t] = acc;
  __syncthreads();
  block_scan_mul(sh, t);
  // canonical prefix times a Montgomery-form product: the canonical output in one product
  const U256 pre = Fr::from_mont(t ? sh[t - 1] : fr_one_m());
  for (int k = 0; k < SCAN_PER; ++k) {
    const uint64_t i = base + k;
    if (i < count) u256_to_u64(Fr::mul_tp(pre, v[k]), out + 4 * i);
  }
  if (t == SCAN_T - 1) str(totals + 4 * blockIdx.x, sh[t]);
}

// phase 2: exclusive scan of the block totals in one block (any number of totals)
__global__ void __launch_bounds__(SCAN_T) k_scan2(uint64_t* totals, uint64_t nb) {
  __shared__ U256 sh[SCAN_T];
  const int t = threadIdx.x;
  const uint64_t per = (nb + SCAN_T - 1) / SCAN_T;
  const uint64_t b0 = (uint64_t)t * per;
  U256 acc = fr_one_m();
  for (uint64_t k = 0; k < per; ++k)
    if (b0 + k < nb) acc = Fr::mul_tp(acc, ldr(totals + 4 * (b0 + k)));
  sh[t] = acc;
  __syncthreads();
  block_scan_mul(sh, t);
  U256 run = t ? sh[t - 1] : fr_one_m();  // exclusive prefix of this thread's range
  for (uint64_t k = 0; k < per; ++k) {
    if (b0 + k >= nb) break;
    const U256 x = ldr(totals + 4 * (b0 + k));
    str(totals + 4 * (b0 + k), run);
    run = Fr::mul_tp(run, x);
  }
}

// phase 3: out[i] = (inclusive product up to i-1) = block exclusive prefix * local
// inclusive[i-1]; reads the phase-1 inclusive values from incl, writes exclusive into out
__global__ void k_scan3(const uint64_t* incl, uint64_t* out, uint64_t count, const uint64_t* totals) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  if (i == 0) { str(out, fr_one_m()); return; }
  const uint64_t j = i - 1;
  const uint64_t blk = j / SCAN_BLK;
  // Montgomery-form total times the canonical inclusive product: canonical (2 products, not 4)
  u256_to_u64(Fr::mul_tp(ldr(totals + 4 * blk), u256_from_u64(incl + 4 * j)), out + 4 * i);
}

// coeff[idx] += delta (blinding: (b_lo + b_hi x [+ b x^2]) * (x^n - 1), plonk.rs:250-252, 304)
struct Blind {
  uint64_t idx[6];
  U256 delta[6];
  int count;
};
__global__ void k_blind(uint64_t* coeff, Blind b) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int k = 0; k < b.count; ++k) str(coeff + 4 * b.idx[k], Fr::add(ldr(coeff + 4 * b.idx[k]), b.delta[k]));
}

// out[i] = sum_k c_k * in_k[i] (+ c0 at i = 0); in_k shorter than i contributes 0
struct LinComb {
  const uint64_t* in[10];
  uint64_t len[10];
  U256 c[10];
  int k;
  U256 c0;
};
__global__ void k_lincomb(LinComb L, uint64_t* out, uint64_t count) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  // conversion-free: canonical inputs times Montgomery-form constants are canonical products
  U256 acc = i == 0 ? Fr::from_mont(L.c0) : u256_zero();
  for (int k = 0; k < L.k; ++k)
    if (i < L.len[k]) acc = Fr::add(acc, Fr::mul_tp(L.c[k], u256_from_u64(L.in[k] + 4 * i)));
  u256_to_u64(acc, out + 4 * i);
}

// out = a b for canonical a and b held at R-degree 1 (b R: mont(a, b R) = a b, canonical)
__global__ void k_mul(const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t count) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) u256_to_u64(Fr::mul_tp(u256_from_u64(a + 4 * i), u256_from_u64(b + 4 * i)), out + 4 * i);
}

// Public inputs (pbf_plonk_prove_bn254_pi*): u[i] = q_c[i] - pub[i] for i < npub, q_c[i] from there
// on (i < n), canonical: the values on H of q_c(x) + PI(x), the quotient's per-proof q_c operand
__global__ void k_qc_minus_pub(const uint64_t* qc, const uint64_t* pub, uint64_t npub, uint64_t* u, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  U256 v = u256_from_u64(qc + 4 * i);
  if (i < npub) v = Fr::sub(v, u256_from_u64(pub + 4 * i));
  u256_to_u64(v, u + 4 * i);
}

// t(x_i) for x_i = g w_N^i on the coset (N = 4n): the numerator of plonk.rs:358-368
// divided by Z_H(x_i) = g^n w_4^(i mod 4) - 1 (inverses zh_inv[0..3] from the host)
// No Montgomery conversions (late round 2): a stored value u "has R-degree d" for the field
// value v when u = v R^d (mod p); mont(u1, u2) = u1 u2 / R adds degrees minus one and adds
// need equal degrees. The coset slots come out of coset_ntt_batch at the degrees
// QUOT_DEG gives (a b c z z(wx) qc raw; ql qr qo s1 s2 s3 l1 at 1; qm at 2) and the host
// passes every constant at the degree its use needs, so every term below lands at degree 0
// and the output is canonical with no to_mont / from_mont (14 products per point fewer).
constexpr int QUOT_DEG[14] = {0, 0, 0, 0, 1, 1, 1, 2, 0, 1, 1, 1, 1, 0};
struct QuotArgs {
  const uint64_t *a, *b, *c, *z, *ql, *qr, *qo, *qm, *qc, *s1, *s2, *s3, *l1;
  const uint64_t* zw;  // z(w x) evaluations (sharded layout), or null: z at index i + 4
  uint64_t N;          // evaluations held here (N, or nl on a rank of a sharded prove)
  uint64_t N_all;      // 4n
  Blk blk;
  U256 beta0, gamma0;  // degree 0
  U256 alpha4;         // degree 4
  U256 k1, k2, alpha2, g, wN;  // degree 1 (Montgomery form)
  U256 zh_inv[4];      // degree 1
};
// ch: points per thread (lane l of a wave takes first + 64 k, k < ch); a chunk's first x
// costs one fr_pow, so ch trades that against the resident waves of a 4n-point grid
__global__ void __launch_bounds__(256) k_quotient(QuotArgs q, uint64_t* out, uint32_t ch) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t i0 = (t / 64) * 64 * ch + (t % 64);
  if (i0 >= q.N) return;
  U256 x = Fr::mul_tp(q.g, fr_pow(q.wN, blk_index(q.blk, i0)));
  const U256 step = pow64(q.wN);
  for (uint64_t p = i0, k = 0; k < ch && p < q.N; ++k, x = blk_next_x(q.blk, p, x, step, q.g, q.wN), p += 64) {
    const uint64_t o = 4 * p;
    const uint64_t i = blk_index(q.blk, p);
    auto ld = [](const uint64_t* p) { return u256_from_u64(p); };  // as stored (its slot's degree)
    const U256 a = ld(q.a + o), b = ld(q.b + o), c = ld(q.c + o), z = ld(q.z + o);
    const U256 zw = q.zw ? ld(q.zw + o) : ld(q.z + 4 * ((i + 4) % q.N_all));  // z(w x_i): w = w_N^4
    // t1: a b q_m + a q_l + b q_r + c q_o + q_c                   (degrees -1+2, 0+1, 0)
    U256 t1 = Fr::mul_tp(Fr::mul_tp(a, b), ld(q.qm + o));
    t1 = Fr::add(t1, Fr::mul_tp(a, ld(q.ql + o)));
    t1 = Fr::add(t1, Fr::mul_tp(b, ld(q.qr + o)));
    t1 = Fr::add(t1, Fr::mul_tp(c, ld(q.qo + o)));
    t1 = Fr::add(t1, ld(q.qc + o));
    // t2 - t3 = (a + beta x + gamma)(b + beta k1 x + gamma)(c + beta k2 x + gamma) z
    //         - (a + beta s1 + gamma)(b + beta s2 + gamma)(c + beta s3 + gamma) z(w x)   (degree -3),
    // times alpha once (alpha at degree 4)
    const U256 bx = Fr::mul_tp(q.beta0, x);  // x at degree 1
    U256 t2 = Fr::mul_tp(Fr::add(Fr::add(a, bx), q.gamma0), Fr::add(Fr::add(b, Fr::mul_tp(bx, q.k1)), q.gamma0));
    t2 = Fr::mul_tp(t2, Fr::add(Fr::add(c, Fr::mul_tp(bx, q.k2)), q.gamma0));
    t2 = Fr::mul_tp(t2, z);
    U256 t3 = Fr::mul_tp(Fr::add(Fr::add(a, Fr::mul_tp(q.beta0, ld(q.s1 + o))), q.gamma0),
                      Fr::add(Fr::add(b, Fr::mul_tp(q.beta0, ld(q.s2 + o))), q.gamma0));
    t3 = Fr::mul_tp(t3, Fr::add(Fr::add(c, Fr::mul_tp(q.beta0, ld(q.s3 + o))), q.gamma0));
    t3 = Fr::mul_tp(t3, zw);
    const U256 t23 = Fr::mul_tp(Fr::sub(t2, t3), q.alpha4);
    // t4: alpha^2 (z - 1) L1                                        (0+1-1, then +1-1)
    const U256 t4 = Fr::mul_tp(Fr::mul_tp(Fr::sub(z, Fr::one_plain()), ld(q.l1 + o)), q.alpha2);
    const U256 num = Fr::add(Fr::add(t1, t23), t4);
    u256_to_u64(Fr::mul_tp(num, q.zh_inv[i & 3]), out + o);
  }
}

// k_quotient on nine 29-bit limbs (round 6, fr29.hpp; option ntt256.l29 = 0 keeps k_quotient).
// fr29::mul(u, v) = u v / 2^261 = (u v / R) / 32: every product carries one more factor 1/32 than
// the 32-bit kernel's, on top of the same R-degree bookkeeping. The host scales the constants so
// that every term of the numerator ends with exactly one such factor -- beta, k1 beta, k2 beta by
// 32 (their products enter sums with raw data), alpha^4 by 32^3, alpha^2 by 32, zh_inv by 32^2 --
// and two constant products align the q_m term (x 32) and q_c (x 1/32); so the output is the
// 32-bit kernel's canonical integer. Lazy sums as in the Fr NTT passes; one operand of every
// product is normalised (reduce() where both would be sums), so its 64-bit columns hold.
using l29::L29;
struct Quot29Args {
  const uint64_t *a, *b, *c, *z, *ql, *qr, *qo, *qm, *qc, *s1, *s2, *s3, *l1, *zw;
  uint64_t N, N_all;
  Blk blk;
  U256 g, wN;                       // x = g wN^i at degree 1, as k_quotient
  L29 beta, gamma, k1b, k2b;        // beta 32, gamma (degree 0), k1 beta 32, k2 beta 32 (degree 1 x)
  L29 alpha4, alpha2, c_qm, c_qc;   // alpha^4 32^3, alpha^2 32, R 32^2, R
  L29 zh[4];                        // zh_inv 32^2
};
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) k_quotient29(Quot29Args q, uint64_t* out, uint32_t ch) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t i0 = (t / 64) * 64 * ch + (t % 64);
  if (i0 >= q.N) return;
  U256 x = Fr::mul_tp(q.g, fr_pow(q.wN, blk_index(q.blk, i0)));
  const U256 step = pow64(q.wN);
  L29 one{};
  one.l[0] = 1;
  for (uint64_t p = i0, k = 0; k < ch && p < q.N; ++k, x = blk_next_x(q.blk, p, x, step, q.g, q.wN), p += 64) {
    const uint64_t o = 4 * p;
    const uint64_t i = blk_index(q.blk, p);
    auto ld = [](const uint64_t* p) { return l29::from_u256(u256_from_u64(p)); };
    const L29 a = ld(q.a + o), b = ld(q.b + o), c = ld(q.c + o), z = ld(q.z + o);
    const L29 zw = q.zw ? ld(q.zw + o) : ld(q.z + 4 * ((i + 4) % q.N_all));
    // t1 (one factor 1/32 per term)
    const L29 ab = fr29::mul(a, b);
    L29 t1 = fr29::mul(fr29::mul(ab, ld(q.qm + o)), q.c_qm);
    t1 = fr29::add(t1, fr29::mul(a, ld(q.ql + o)));
    t1 = fr29::add(t1, fr29::mul(b, ld(q.qr + o)));
    t1 = fr29::add(t1, fr29::mul(c, ld(q.qo + o)));
    t1 = fr29::add(t1, fr29::mul(ld(q.qc + o), q.c_qc));
    // t2 - t3 (three factors 1/32 each side)
    const L29 xl = l29::from_u256(x);
    const L29 bx = fr29::mul(q.beta, xl);
    const L29 A = fr29::add(fr29::add(a, bx), q.gamma);
    const L29 Bn = fr29::reduce(fr29::add(fr29::add(b, fr29::mul(q.k1b, xl)), q.gamma));
    const L29 Cs = fr29::add(fr29::add(c, fr29::mul(q.k2b, xl)), q.gamma);
    const L29 t2 = fr29::mul(fr29::mul(fr29::mul(A, Bn), Cs), z);
    const L29 D = fr29::add(fr29::add(a, fr29::mul(q.beta, ld(q.s1 + o))), q.gamma);
    const L29 En = fr29::reduce(fr29::add(fr29::add(b, fr29::mul(q.beta, ld(q.s2 + o))), q.gamma));
    const L29 Fs = fr29::add(fr29::add(c, fr29::mul(q.beta, ld(q.s3 + o))), q.gamma);
    const L29 t3 = fr29::mul(fr29::mul(fr29::mul(D, En), Fs), zw);
    const L29 t23 = fr29::mul(fr29::sub(t2, t3, fr29::B4R), q.alpha4);
    // t4 = alpha^2 (z - 1) L1
    const L29 t4 = fr29::mul(fr29::mul(fr29::sub(z, one, fr29::B2R), ld(q.l1 + o)), q.alpha2);
    const L29 num = fr29::reduce(fr29::add(fr29::add(t1, t23), t4));
    u256_to_u64(fr29::canon(fr29::mul(num, q.zh[i & 3])), out + o);
  }
}

// host: the 29-bit kernel's constants from k_quotient's (QuotArgs)
static L29 h_relimb(const U256& a) {
  L29 r;
  for (int i = 0; i < 9; ++i) {
    const int bit = 29 * i;
    uint64_t v = 0;
    for (int k = 0; k < 29; ++k) {
      const int bb = bit + k;
      if (bb < 256 && ((a.w[bb / 32] >> (bb % 32)) & 1)) v |= 1ull << k;
    }
    r.l[i] = (uint32_t)v;
  }
  return r;
}
// a 32^e (mod r) for a canonical integer a (32 in Montgomery form: Fr::mul(a, 32 R) = 32 a)
static U256 h_times32(U256 a, int e) {
  U256 c32 = Fr::one_plain();
  c32.w[0] = 32;
  const U256 c32m = Fr::to_mont(c32);
  for (int k = 0; k < e; ++k) a = Fr::mul(a, c32m);
  return a;
}
// Round 6: the coset scaling and power kernels on 29-bit limbs (fr29.hpp: the product ~1.39x
// cheaper than the 32-bit one; both kernels are product-bound). The tables hold the 32-bit
// kernels' numbers times 32 (x 2^261 where those hold x 2^256), so every output is the same
// canonical integer. Bounds: tables canonical; the running power stays below 1.01 r (a product
// is below a b / 2^261 + r); an input below 2^256 times it is below 1.04 r, canon() takes it to
// [0, r).
struct ScalePow29 {
  L29 x0, step;
  L29 tl[64];
  L29 tv[SP_WBITS];
};
static_assert(sizeof(ScalePow29) + 64 <= 4096, "kernel argument limit");
static ScalePow29 to29(const ScalePow& sp) {
  auto c = [](const U256& a) { return h_relimb(h_times32(a, 1)); };
  ScalePow29 r;
  r.x0 = c(sp.x0);
  r.step = c(sp.step);
  for (int l = 0; l < 64; ++l) r.tl[l] = c(sp.tl[l]);
  for (int k = 0; k < SP_WBITS; ++k) r.tv[k] = c(sp.tv[k]);
  return r;
}
static ScalePow29 powers_tab29(const U256& base, const U256& start) { return to29(powers_tab(base, start)); }
__device__ __forceinline__ L29 sp29_first(const ScalePow29& sp, uint64_t t) {
  L29 x = fr29::mul(sp.x0, sp.tl[t % 64]);
  for (uint64_t v = t / 64, k = 0; v; v >>= 1, ++k)
    if (v & 1) x = fr29::mul(x, sp.tv[k]);
  return x;
}
// k_scale_pow on 29-bit limbs
__global__ void k_scale_pow29(const uint64_t* in, uint64_t in_off, uint64_t in_stride, uint64_t len, uint64_t* out,
                              uint64_t count, ScalePow29 sp) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t i0 = chunk_first(t);
  if (i0 >= count) return;
  if (in_off + in_stride * i0 >= len) {
    for (uint64_t i = i0, k = 0; k < PV_CHUNK && i < count; ++k, i += 64)
      for (int q = 0; q < 4; ++q) out[4 * i + q] = 0;
    return;
  }
  L29 x = sp29_first(sp, t);
  const L29 step = sp.step;
  for (uint64_t i = i0, k = 0; k < PV_CHUNK && i < count; ++k, i += 64) {
    const uint64_t j = in_off + in_stride * i;
    if (j < len) u256_to_u64(fr29::canon(fr29::mul(l29::from_u256(u256_from_u64(in + 4 * j)), x)), out + 4 * i);
    else for (int q = 0; q < 4; ++q) out[4 * i + q] = 0;
    x = fr29::mul(x, step);
  }
}
// k_powers on 29-bit limbs: out[i] = start base^i (canonical: the running power times 1)
__global__ void k_powers29(uint64_t* out, uint64_t count, ScalePow29 sp) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t i0 = chunk_first(t);
  if (i0 >= count) return;
  L29 one{};
  one.l[0] = 1;
  L29 x = sp29_first(sp, t);
  const L29 step = sp.step;
  for (uint64_t i = i0, k = 0; k < PV_CHUNK && i < count; ++k, i += 64) {
    u256_to_u64(fr29::canon(fr29::mul(x, one)), out + 4 * i);
    x = fr29::mul(x, step);
  }
}

// The coset scaling for the public Fr coset transforms (ntt256.hip pbf_ntt_fr256_coset*):
// out[b*out_pitch + i] = in[b*len + i] * base^i, i < len, for `batch` polynomials (base in
// Montgomery form, elements 4 x u64; in may equal out when out_pitch == len). The prover's own
// calls (Prover::scale) do not come through here.
int fr256_scale_pow(bool l29, const uint64_t* in, uint64_t len, uint64_t* out, uint64_t out_pitch, uint64_t batch,
                    const U256& base, hipStream_t s) {
  const ScalePow sp = scale_pow_tab(fr_one_m(), base, 0, 1);
  const ScalePow29 sp29 = to29(sp);
  const dim3 grid(blocks_for((len + PV_CHUNK - 1) / PV_CHUNK));
  for (uint64_t b = 0; b < batch; ++b) {
    if (l29)
      hipLaunchKernelGGL(k_scale_pow29, grid, dim3(256), 0, s, in + 4 * len * b, (uint64_t)0, (uint64_t)1, len,
                         out + 4 * out_pitch * b, len, sp29);
    else
      hipLaunchKernelGGL(k_scale_pow, grid, dim3(256), 0, s, in + 4 * len * b, (uint64_t)0, (uint64_t)1, len,
                         out + 4 * out_pitch * b, len, sp);
  }
  PBF_HIP(hipGetLastError());
  return 0;
}

static void launch_quotient(const QuotArgs& qa, uint64_t* out, bool l29, hipStream_t s) {
  constexpr uint32_t qch = 32;  // points per thread
  const uint32_t blocks = blocks_for((qa.N + qch - 1) / qch);
  if (!l29) {
    hipLaunchKernelGGL(k_quotient, dim3(blocks), dim3(256), 0, s, qa, out, qch);
    return;
  }
  Quot29Args q;
  q.a = qa.a; q.b = qa.b; q.c = qa.c; q.z = qa.z; q.ql = qa.ql; q.qr = qa.qr; q.qo = qa.qo; q.qm = qa.qm;
  q.qc = qa.qc; q.s1 = qa.s1; q.s2 = qa.s2; q.s3 = qa.s3; q.l1 = qa.l1; q.zw = qa.zw;
  q.N = qa.N; q.N_all = qa.N_all; q.blk = qa.blk; q.g = qa.g; q.wN = qa.wN;
  q.beta = h_relimb(h_times32(qa.beta0, 1));
  q.gamma = h_relimb(qa.gamma0);
  // k_quotient forms beta x k1 as mont(mont(beta0, x), k1): here beta0 k1 / R once on the host
  q.k1b = h_relimb(h_times32(Fr::mul(qa.beta0, qa.k1), 1));
  q.k2b = h_relimb(h_times32(Fr::mul(qa.beta0, qa.k2), 1));
  q.alpha4 = h_relimb(h_times32(qa.alpha4, 3));
  q.alpha2 = h_relimb(h_times32(qa.alpha2, 1));
  const U256 rm = Fr::to_mont(Fr::one_plain());  // R mod r: "1 at degree 1"
  q.c_qm = h_relimb(h_times32(rm, 2));
  q.c_qc = h_relimb(rm);
  for (int j = 0; j < 4; ++j) q.zh[j] = h_relimb(h_times32(qa.zh_inv[j], 2));
  hipLaunchKernelGGL(k_quotient29, dim3(blocks), dim3(256), 0, s, q, out, qch);
}

// Synthetic division by (x - z), the quotients of the openings (plonk.rs:430-442):
// q = (p - y) / (x - z) for p of L coefficients (y subtracted from p_0), q_(L-2-k) = s_k with
//   s_k = p_(L-1-k) + z s_(k-1)   (Horner from the top coefficient, s_(-1) = 0)
// and s_(L-1) = p(z) - y, the remainder, which must be zero (the reference's `rem == 0`
// asserts). O(L) work on the coefficients instead of a coset NTT, a pointwise division by
// (x_i - z) and a coset INTT of 4n points -- and no failure when z happens to lie on the
// evaluation coset (the reference's long division has no such case).
// Blocked linear recurrence with the constant multiplier z: (1) every block of HS_BLK
// consecutive k runs its recurrence from 0 (per thread, then a Hillis-Steele pass over the
// threads with multipliers z^(HS_PER 2^j)) and leaves its total; (2) one block turns the
// totals into each block's incoming s (multiplier z^HS_BLK); (3) s_k += z^(k - k_b + 1) s_in.
// (HS_T, HS_PER, HS_BLK, HS_LOG_T and HsArgs: prover.hpp, shared with the KZG opening)
// q[L-2-k] <- block-local s_k (k < L-1); the block-local remainder candidate in rem[block]
// (v[] lives in scratch here (528 B per lane); compile-time indices keep it in 213 VGPRs at two
// waves per SIMD, which measured 4 % slower: 1.74 against 1.68 ms for the two 2^24 divisions)
__global__ void __launch_bounds__(HS_T) k_hs1(HsArgs a, uint64_t* q, uint64_t* totals, uint64_t* rem) {
  __shared__ U256 sh[HS_T];
  const int t = threadIdx.x;
  const uint64_t k0 = (uint64_t)blockIdx.x * HS_BLK + (uint64_t)t * HS_PER;
  U256 v[HS_PER];
  U256 acc = u256_zero();
#pragma unroll
  for (int m = 0; m < HS_PER; ++m) {
    const uint64_t k = k0 + m;
    U256 u = u256_zero();
    if (k < a.L) {
      u = u256_from_u64(a.p + 4 * (a.L - 1 - k));
      if (k == a.L - 1) u = Fr::sub(u, a.y);
    }
    acc = Fr::add(u, Fr::mul_tp(a.z, acc));
    v[m] = acc;
  }
  sh[t] = acc;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < HS_LOG_T; ++j) {
    const int off = 1 << j;
    U256 x = sh[t];
    if (t >= off) x = Fr::add(x, Fr::mul_tp(a.zs[j], sh[t - off]));
    __syncthreads();
    sh[t] = x;
    __syncthreads();
  }
  const U256 carry = t ? sh[t - 1] : u256_zero();
  U256 zk = a.z;
#pragma unroll
  for (int m = 0; m < HS_PER; ++m) {
    const uint64_t k = k0 + m;
    const U256 sk = Fr::add(v[m], Fr::mul_tp(zk, carry));
    zk = Fr::mul_tp(zk, a.z);
    if (k + 1 < a.L) u256_to_u64(sk, q + 4 * (a.L - 2 - k));
    else if (k + 1 == a.L) u256_to_u64(sk, rem);
  }
  if (t == HS_T - 1) u256_to_u64(sh[t], totals + 4 * blockIdx.x);
}
// totals[b] <- s_(b HS_BLK - 1), the s entering block b (0 for b = 0); one block
__global__ void __launch_bounds__(HS_T) k_hs2(uint64_t* totals, uint64_t nb, U256 zb, U256 zb_per) {
  __shared__ U256 sh[HS_T];
  const int t = threadIdx.x;
  const uint64_t per = (nb + HS_T - 1) / HS_T;
  const uint64_t b0 = (uint64_t)t * per;
  U256 acc = u256_zero();
  for (uint64_t k = 0; k < per; ++k)
    if (b0 + k < nb) acc = Fr::add(u256_from_u64(totals + 4 * (b0 + k)), Fr::mul_tp(zb, acc));
  sh[t] = acc;
  __syncthreads();
  U256 m = zb_per;  // zb^per: the multiplier across one thread's range (from the host, round 6)
  for (int off = 1; off < HS_T; off <<= 1) {
    U256 x = sh[t];
    if (t >= off) x = Fr::add(x, Fr::mul_tp(m, sh[t - off]));
    __syncthreads();
    sh[t] = x;
    __syncthreads();
    m = Fr::mul_tp(m, m);
  }
  U256 c = t ? sh[t - 1] : u256_zero();
  for (uint64_t k = 0; k < per; ++k) {
    if (b0 + k >= nb) break;
    const U256 x = u256_from_u64(totals + 4 * (b0 + k));
    u256_to_u64(c, totals + 4 * (b0 + k));
    c = Fr::add(x, Fr::mul_tp(zb, c));
  }
}
// s_k += z^(k - k_b + 1) s_in(b); the remainder likewise
__global__ void __launch_bounds__(HS_T) k_hs3(uint64_t* q, uint64_t L, HsArgs a, const uint64_t* totals,
                                              uint64_t* rem) {
  const uint64_t b = blockIdx.x;
  if (b == 0) return;  // block 0 enters with s = 0
  const U256 cin = u256_from_u64(totals + 4 * b);
  const uint64_t k0 = b * HS_BLK + (uint64_t)threadIdx.x * HS_PER;
  if (k0 >= L) return;
  const U256 z = a.z;
  // z^(t HS_PER + 1) from the table z^(HS_PER 2^j) over t's bits (round 6: at most 9 products
  // instead of a Fermat-length fr_pow per thread; the two 2^24 divisions 1.04 -> 0.91 ms)
  U256 zk = z;
#pragma unroll
  for (int j = 0; j < HS_LOG_T; ++j)
    if ((threadIdx.x >> j) & 1) zk = Fr::mul_tp(zk, a.zs[j]);
  for (int m = 0; m < HS_PER; ++m) {
    const uint64_t k = k0 + m;
    if (k >= L) break;
    uint64_t* dst = k + 1 < L ? q + 4 * (L - 2 - k) : rem;
    u256_to_u64(Fr::add(u256_from_u64(dst), Fr::mul_tp(zk, cin)), dst);
    zk = Fr::mul_tp(zk, z);
  }
}

// any nonzero element in [from, to) sets *bad
__global__ void k_nonzero(const uint64_t* a, uint64_t from, uint64_t to, int* bad) {
  const uint64_t i = from + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < to && (a[4 * i] | a[4 * i + 1] | a[4 * i + 2] | a[4 * i + 3])) *bad = 1;
}

// ---------------------------------------------------------------- sharded layouts (G > 1)
// Coefficient vectors of a sharded prove live in one of two layouts:
//  SS (stride shard): slot m of rank r holds global coefficient j = r + G m -- what the
//     stride-sharded (I)NTT produces and consumes;
//  CR (contiguous range): rank r holds j in [r Bc, r Bc + Bc) at slot j - r Bc, and the last
//     rank also the tail [Ls, Ls + TAILC) at slots Bc.. (Ls = G Bc: n, or 2n in mode 0) -- what
//     the commitments (point ranges of the SRS), evaluations, linear combinations and
//     synthetic divisions use.
// SS -> CR is one all-to-all: k_xpose_pack writes, for each destination rank d and part k, the
// Bc / G + TF elements of d's range with j = (r - off_k) mod G (mod G), k_xpose_unpack places
// what arrived. A "part" is a slice [off_k, off_k + len_k) of the source vector that becomes its
// own CR vector (t(x) -> t_lo, t_mid, t_hi); Bc and Ls are multiples of G.
constexpr uint64_t TAILC = 8;  // tail slots of a CR vector (the last rank), and of an SS vector
struct XPose {
  const uint64_t* ss[3];  // source SS vector of each part
  uint64_t* cr[3];        // destination CR vector of each part (zeroed by the caller)
  uint64_t off[3], len[3];
  uint64_t ss_slots;      // source slots of this rank
  uint64_t Ls, Bc, cap;   // cap = Bc / G + TF per (destination, part)
  uint32_t G, rank, P;
};
__global__ void k_xpose_pack(XPose x, uint64_t* send) {
  const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= x.ss_slots) return;
  const uint64_t i = x.rank + (uint64_t)x.G * m;
  for (uint32_t k = 0; k < x.P; ++k) {
    if (i < x.off[k] || i >= x.off[k] + x.len[k]) continue;
    const uint64_t j = i - x.off[k];
    uint64_t d, e;
    if (j < x.Ls) {
      d = j / x.Bc;
      e = (j - d * x.Bc) / x.G;
    } else {
      d = x.G - 1;
      e = x.Bc / x.G + (j - x.Ls) / x.G;
    }
    const uint64_t* src = x.ss[k] + 4 * m;
    uint64_t* dst = send + 4 * ((d * x.P + k) * x.cap + e);
    for (int q = 0; q < 4; ++q) dst[q] = src[q];
  }
}
__global__ void k_xpose_unpack(XPose x, const uint64_t* recv) {
  const uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (uint64_t)x.G * x.P * x.cap) return;
  const uint64_t e = id % x.cap, k = (id / x.cap) % x.P, src = id / (x.cap * x.P);
  const uint64_t c = (src + x.G - x.off[k] % x.G) % x.G;  // j = i - off_k with i = src (mod G)
  uint64_t j;
  if (e < x.Bc / x.G) {
    j = x.rank * x.Bc + c + x.G * e;
    if (j >= x.Ls) return;
  } else {
    if (x.rank != x.G - 1) return;
    j = x.Ls + c + x.G * (e - x.Bc / x.G);
    if (j >= x.Ls + TAILC) return;
  }
  if (j >= x.len[k]) return;
  const uint64_t* sp = recv + 4 * id;
  uint64_t* dp = x.cr[k] + 4 * (j - x.rank * x.Bc);
  for (int q = 0; q < 4; ++q) dp[q] = sp[q];
}

// coeff[slot(idx)] += delta for the blinding indices this rank holds (plonk.rs:250-252, 304):
// ss: SS layout (slot idx / G on rank idx mod G), else CR
struct BlindMap {
  Blind b;
  uint32_t ss, G, rank;
  uint64_t Ls, Bc;
};
__global__ void k_blind_map(uint64_t* coeff, BlindMap m) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int k = 0; k < m.b.count; ++k) {
    const uint64_t j = m.b.idx[k];
    uint64_t slot;
    if (m.ss) {
      if (j % m.G != m.rank) continue;
      slot = j / m.G;
    } else if (j < m.Ls) {
      if (j / m.Bc != m.rank) continue;
      slot = j % m.Bc;
    } else {
      if (m.rank != m.G - 1) continue;
      slot = m.Bc + (j - m.Ls);
    }
    str(coeff + 4 * slot, Fr::add(ldr(coeff + 4 * slot), m.b.delta[k]));
  }
}

// q[e] += z^(cnt - 1 - e) V for e < cnt, q[cnt - 1] starting from 0: a rank's part of a synthetic
// division (k_hs*) completed by the contribution V of the coefficients above its range
__global__ void k_hs_carry(uint64_t* q, uint64_t cnt, U256 z, U256 V) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t k0 = chunk_first(t);  // k = cnt - 1 - e: the power of z
  if (k0 >= cnt) return;
  U256 x = Fr::mul_tp(V, fr_pow(z, k0));
  const U256 step = pow64(z);
  for (uint64_t k = k0, c = 0; c < PV_CHUNK && k < cnt; ++c, k += 64) {
    const uint64_t e = cnt - 1 - k;
    const U256 base = k == 0 ? u256_zero() : u256_from_u64(q + 4 * e);
    u256_to_u64(Fr::add(base, x), q + 4 * e);
    x = Fr::mul_tp(x, step);
  }
}

// out[0] = a[0] * b[0] (a rank's row-product total: last exclusive prefix times last term)
__global__ void k_mul1(const uint64_t* a, const uint64_t* b, uint64_t* out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) u256_to_u64(Fr::from_mont(Fr::mul(ldr(a), ldr(b))), out);
}

// batched Horner: partial[p][chunk] = x^(off + chunk start) * sum of the chunk's terms.
// Round 6: a thread's Horner value h_t enters the block sum as h_t x^(64 t) through the LDS tree
// (level s adds sh[t + s] x^(64 s)), and the block's x^(off + 16384 ch) is a product over the set
// bits of ch; the powers are host products in the arguments (one table per distinct (x, off): the
// prover evaluates at z and z w), not a square-and-multiply chain per thread (~36 dependent
// products next to the 64 Horner steps)
constexpr int EV_T = 256, EV_PER = 64, EV_PW = 26, EV_XS = 2;  // chunks < 2^(EV_PW - 8)
struct EvalArgs {
  const uint64_t* poly[12];
  uint64_t len[12];
  U256 x[12];
  uint64_t off[12];  // global index of poly[p][0] (a rank's coefficient range; 0 on one GPU)
  uint64_t chunks;   // per polynomial
  // filled by launch_eval: pw[xi[p]][k] = x^(64 2^k), xoff[xi[p]] = x^off (Montgomery form)
  U256 pw[EV_XS][EV_PW];
  U256 xoff[EV_XS];
  uint8_t xi[12];
};
static_assert(sizeof(EvalArgs) <= 4096, "kernel argument limit");
__global__ void __launch_bounds__(EV_T) k_eval_partial(EvalArgs e, uint64_t* partial) {
  __shared__ U256 sh[EV_T];
  const uint64_t p = blockIdx.x / e.chunks, ch = blockIdx.x % e.chunks;
  const int t = threadIdx.x;
  const uint64_t start = (ch * EV_T + t) * EV_PER;
  const U256 x = e.x[p];
  const int xi = e.xi[p];
  U256 acc = u256_zero();
  if (start < e.len[p]) {
    uint64_t end = start + EV_PER;
    if (end > e.len[p]) end = e.len[p];
    // conversion-free Horner: canonical acc times Montgomery-form x stays canonical
    for (uint64_t j = end; j-- > start;) acc = Fr::add(Fr::mul_tp(acc, x), u256_from_u64(e.poly[p] + 4 * j));
  }
  sh[t] = acc;
  __syncthreads();
  for (int s = EV_T / 2, k = 7; s > 0; s >>= 1, --k) {  // EV_T = 2^8: x^(64 s) = pw[k]
    if (t < s) sh[t] = Fr::add(sh[t], Fr::mul_tp(sh[t + s], e.pw[xi][k]));
    __syncthreads();
  }
  if (t == 0) {
    U256 f = e.xoff[xi];
    for (uint64_t c = ch, k = 8; c; c >>= 1, ++k)  // 16384 ch = 64 2^8 ch
      if (c & 1) f = Fr::mul_tp(f, e.pw[xi][k]);
    u256_to_u64(Fr::mul_tp(sh[0], f), partial + 4 * blockIdx.x);
  }
}
// out[p] = sum of the chunks' partials (one block per polynomial; round 6: the serial loop of one
// thread per polynomial had taken 1.6 ms over the 1024 chunks of a 2^24-row evaluation)
__global__ void __launch_bounds__(256) k_eval_final(const uint64_t* partial, uint64_t chunks, uint64_t* out) {
  __shared__ U256 sh[256];
  const uint64_t p = blockIdx.x;
  const int t = threadIdx.x;
  U256 acc = u256_zero();
  for (uint64_t i = t; i < chunks; i += 256) acc = Fr::add(acc, u256_from_u64(partial + 4 * (p * chunks + i)));
  sh[t] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sh[t] = Fr::add(sh[t], sh[t + s]);
    __syncthreads();
  }
  if (t == 0) u256_to_u64(sh[0], out + 4 * p);
}

// the power tables, the partial sums, then the totals of np polynomials into evals
static int launch_eval(EvalArgs& e, int np, DevBuf& partial, uint64_t* evals, hipStream_t s) {
  if (e.chunks >= (1ull << (EV_PW - 8))) return fail(PBF_EINVAL, "evaluation longer than its power tables");
  U256 kx[EV_XS];
  uint64_t koff[EV_XS];
  int nx = 0;
  for (int p = 0; p < np; ++p) {
    int j = 0;
    while (j < nx && !(Fr::eq(kx[j], e.x[p]) && koff[j] == e.off[p])) ++j;
    if (j == nx) {
      if (nx == EV_XS) return fail(PBF_EINVAL, "more distinct evaluation points than power tables");
      kx[j] = e.x[p]; koff[j] = e.off[p];
      e.xoff[j] = fr_pow(e.x[p], e.off[p]);
      e.pw[j][0] = fr_pow(e.x[p], EV_PER);
      for (int k = 1; k < EV_PW; ++k) e.pw[j][k] = Fr::mul(e.pw[j][k - 1], e.pw[j][k - 1]);
      ++nx;
    }
    e.xi[p] = (uint8_t)j;
  }
  const uint64_t pn = np * e.chunks;
  int rc = partial.ensure(pn * 32);
  if (rc) return rc;
  uint64_t* part = (uint64_t*)partial.p;
  hipLaunchKernelGGL(k_eval_partial, dim3((uint32_t)pn), dim3(EV_T), 0, s, e, part);
  hipLaunchKernelGGL(k_eval_final, dim3(np), dim3(256), 0, s, (const uint64_t*)part, e.chunks, evals);
  return 0;
}

struct ProverBufs {
  DevBuf &hpow, &sigma, &coef, &acc, &tmp0, &tmp1, &tmp2, &coset, &t, &work, &flag, &evals, &partial;
  explicit ProverBufs(pbf_ctx* c)
      : hpow(c->buf("pv.hpow")), sigma(c->buf("pv.sigma")), coef(c->buf("pv.coef")), acc(c->buf("pv.acc")),
        tmp0(c->buf("pv.tmp0")), tmp1(c->buf("pv.tmp1")), tmp2(c->buf("pv.tmp2")), coset(c->buf("pv.coset")),
        t(c->buf("pv.t")), work(c->buf("pv.work")), flag(c->buf("pv.flag")), evals(c->buf("pv.evals")),
        partial(c->buf("pv.partial")) {}
};

// ---------------------------------------------------------------- prover.hpp: the launchers shared
// with the KZG entry points and the verifiers
void hs_set_point(HsArgs& a, const U256& z) {
  a.z = z;
  for (int j = 0; j < HS_LOG_T; ++j) a.zs[j] = fr_pow(z, (uint64_t)HS_PER << j);
}
int hs_div_run(pbf_ctx* ctx, const HsArgs& a, uint64_t* q, uint64_t* rem, hipStream_t s) {
  const uint64_t nb = (a.L + HS_BLK - 1) / HS_BLK;
  DevBuf& hb = ctx->buf("pv.hs");
  int rc = hb.ensure(nb * 32);
  if (rc) return rc;
  uint64_t* totals = (uint64_t*)hb.p;
  hipLaunchKernelGGL(k_hs1, dim3((uint32_t)nb), dim3(HS_T), 0, s, a, q, totals, rem);
  const U256 zb = fr_pow(a.z, HS_BLK);
  hipLaunchKernelGGL(k_hs2, dim3(1), dim3(HS_T), 0, s, totals, nb, zb, fr_pow(zb, (nb + HS_T - 1) / HS_T));
  hipLaunchKernelGGL(k_hs3, dim3((uint32_t)nb), dim3(HS_T), 0, s, q, a.L, a, (const uint64_t*)totals, rem);
  PBF_HIP(hipGetLastError());
  return 0;
}
int fr_eval_run(const uint64_t* const* polys, const uint64_t* lens, const U256* xs, int np, uint64_t off,
                DevBuf& partial, uint64_t* d_evals, hipStream_t s) {
  if (np < 1 || np > 12) return fail(PBF_EINVAL, "1 .. 12 polynomials per evaluation launch");
  EvalArgs e;
  uint64_t longest = 1;  // one chunk at least: a rank may hold no coefficient of any polynomial
  for (int p = 0; p < np; ++p) {
    e.poly[p] = polys[p];
    e.len[p] = lens[p];
    e.x[p] = xs[p];
    e.off[p] = off;
    longest = std::max(longest, lens[p]);
  }
  e.chunks = (longest + (uint64_t)EV_T * EV_PER - 1) / ((uint64_t)EV_T * EV_PER);
  int rc = launch_eval(e, np, partial, d_evals, s);
  if (rc) return rc;
  PBF_HIP(hipGetLastError());
  return 0;
}
int fr_lincomb_run(int k, const uint64_t* const* in, const uint64_t* lens, const U256* c, const U256& c0,
                   uint64_t* out, uint64_t count, hipStream_t s) {
  if (k < 1 || k > 10) return fail(PBF_EINVAL, "1 .. 10 inputs per linear combination");
  LinComb L;
  for (int i = 0; i < k; ++i) {
    L.in[i] = in[i];
    L.len[i] = lens[i];
    L.c[i] = c[i];
  }
  L.k = k;
  L.c0 = c0;
  hipLaunchKernelGGL(k_lincomb, dim3(blocks_for(count)), dim3(256), 0, s, L, out, count);
  PBF_HIP(hipGetLastError());
  return 0;
}
int sigma_table_run(uint64_t n, const U256& omega, const U256& k1, const U256& k2, const uint64_t* d_copies,
                    uint64_t* hpow, uint64_t* sigma, int* bad, hipStream_t s) {
  hipLaunchKernelGGL(k_powers29, dim3(blocks_for((n + PV_CHUNK - 1) / PV_CHUNK)), dim3(256), 0, s, hpow, n,
                     powers_tab29(omega, fr_one_m()));
  hipLaunchKernelGGL(k_sigma, dim3(blocks_for(3 * n)), dim3(256), 0, s, d_copies, (const uint64_t*)hpow, n, (uint64_t)0,
                     n, k1, k2, sigma, bad);
  PBF_HIP(hipGetLastError());
  return 0;
}
int fr_powers_run(uint64_t* out, uint64_t count, const U256& base, const U256& start, hipStream_t s) {
  if (!count) return 0;
  hipLaunchKernelGGL(k_powers29, dim3(blocks_for((count + PV_CHUNK - 1) / PV_CHUNK)), dim3(256), 0, s, out, count,
                     powers_tab29(base, start));
  PBF_HIP(hipGetLastError());
  return 0;
}
int fr_inv_batch_run(pbf_ctx* ctx, const uint64_t* den, uint64_t* out, uint64_t count, int* bad, hipStream_t s) {
  return div_batch(ctx, nullptr, den, out, count, bad, s);
}

}  // namespace pbf

using namespace pbf;

namespace {

struct Prover {
  pbf_ctx* ctx;
  hipStream_t s;
  uint64_t n, N;
  U256 omega, omegaN, g, g_inv;
  uint64_t w_plain[4], wN_plain[4];
  int* d_bad;
  bool timing = false;
  double t_last = 0;
  // option prover.timing = 1: per-round wall times on stderr (stream synchronised at each mark)
  void mark(const char* what) {
    if (!timing) return;
    (void)hipStreamSynchronize(s);
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    const double t = ts.tv_sec * 1e3 + ts.tv_nsec / 1e6;
    if (t_last > 0) fprintf(stderr, "[pbf prover] %-28s %9.3f ms\n", what, t - t_last);
    t_last = t;
  }

  int check_bad(const char* what) {
    int bad = 0;
    PBF_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    PBF_HIP(hipStreamSynchronize(s));
    if (bad) return fail(PBF_EINVAL, what);
    return 0;
  }
  int ntt(const uint64_t* w, const uint64_t* in, uint64_t* out, uint64_t size, uint64_t batch, int inverse) {
    return pbf_ntt_fr256_batch_dev(ctx, w, in, out, size, batch, inverse, s);
  }

  // ---- multi-GPU split (pbf_plonk_prove_bn254_sharded_dev; G = 1: the single-GPU prover)
  const pbf_comm* comm = nullptr;
  uint32_t G = 1, rank = 0;
  uint64_t nl = 0, S = 0;    // 4n / G evaluations per rank, in G blocks of S
  DevBuf* shard = nullptr;   // stride-shard staging (16 nl elements)
  uint64_t count() const { return G > 1 ? nl : N; }  // coset evaluations held by this rank
  Blk blk() const {
    Blk b;
    b.nl = nl; b.S = S; b.rank = rank; b.G = G;
    return b;
  }
  int a2a(size_t bytes) {
    if (comm->all_to_all(comm->user, bytes, (void*)s)) return fail(PBF_ECOMM, "all_to_all callback failed");
    return 0;
  }
  int ag(size_t bytes) {
    if (comm->all_gather(comm->user, bytes, (void*)s)) return fail(PBF_ECOMM, "all_gather callback failed");
    return 0;
  }
  void scale(const uint64_t* in, uint64_t in_off, uint64_t in_stride, uint64_t len, uint64_t* out, uint64_t cnt,
             const U256& base, uint64_t e_off, uint64_t e_mult, int deg = 0) {
    // outputs at R-degree deg: the constant R^deg in Montgomery form is R^(deg + 1)
    U256 c0 = Fr::one_plain();
    for (int d = 0; d <= deg; ++d) c0 = Fr::to_mont(c0);
    const ScalePow sp = scale_pow_tab(deg != 0 ? c0 : fr_one_m(), base, e_off, e_mult);
    if (ctx->options.num("ntt256.l29", 1) != 0)
      hipLaunchKernelGGL(k_scale_pow29, dim3(blocks_for((cnt + PV_CHUNK - 1) / PV_CHUNK)), dim3(256), 0, s, in, in_off,
                         in_stride, len, out, cnt, to29(sp));
    else
      hipLaunchKernelGGL(k_scale_pow, dim3(blocks_for((cnt + PV_CHUNK - 1) / PV_CHUNK)), dim3(256), 0, s, in, in_off,
                         in_stride, len, out, cnt, sp);
  }
  // k coset NTTs of size N on one GPU: slot i = evaluations of sum_j srcs[i][j] (bases[i] x)^j at
  // g w_N^e, slots N apart in `out`, at R-degree degs[i] (null: canonical). Sharded: coset_ntt_ss.
  int coset_ntt_batch(int k, const uint64_t* const* srcs, const uint64_t* lens, const U256* bases, uint64_t* out,
                      const int* degs = nullptr) {
    // only the scaled coefficients are written (the longest length of the batch; round 6): the
    // transform's first pass reads nothing past them (pbf_internal_ntt_fr256_prefix), so the
    // 3/4 of every 4n slot that is zero padding is neither stored nor loaded
    uint64_t mx = 0;
    for (int i = 0; i < k; ++i) mx = lens[i] > mx ? lens[i] : mx;
    if (mx > N) mx = N;
    for (int i = 0; i < k; ++i)
      scale(srcs[i], 0, 1, lens[i], out + 4 * N * i, mx, bases[i], 0, 1, degs ? degs[i] : 0);
    PBF_HIP(hipGetLastError());
    return pbf_internal_ntt_fr256_prefix(ctx, wN_plain, out, N, k, mx, s);  // one batched NTT
  }
  // coefficients of the polynomial whose N coset evaluations are `ev` (one GPU)
  int coset_intt(uint64_t* ev, uint64_t* out) {
    int rc = ntt(wN_plain, ev, ev, N, 1, 1);
    if (rc) return rc;
    scale(ev, 0, 1, N, out, N, g_inv, 0, 1);
    PBF_HIP(hipGetLastError());
    return 0;
  }
  // SRS::eval_at_s (plonk.rs:51-58) as a fixed-base MSM against the SRS window table
  // (msm.hpp), its XYZZ result left in device slot `slot` (finish_commits collects all of
  // them with one copy: the challenges are inputs, nothing waits on a commitment; the _fs
  // entries, whose challenges are derived, collect round by round). Sharded:
  // commit_cr (below), this rank's point range.
  const Affine* srs_tbl = nullptr;
  uint64_t srs_n = 0;
  Xyzz* slots = nullptr;  // 9 (this rank's partial sums when sharded)
  int commit(const uint64_t* coeff, uint64_t len, int slot) {
    return msm_fixed_device(ctx, srs_tbl, srs_n, 0, coeff, len, s, slots + slot);
  }
  // Horner from the top coefficient over p of L >= 2 coefficients (k_hs1..3): q = the quotient
  // of (p - y) / (x - z) (L - 1 coefficients), *rem = p(z) - y
  int synth_div_run(const uint64_t* p, uint64_t L, const U256& z, const U256& y, uint64_t* q, uint64_t* rem) {
    HsArgs a;
    a.p = p;
    a.L = L;
    a.y = Fr::from_mont(y);
    hs_set_point(a, z);
    return hs_div_run(ctx, a, q, rem, s);
  }
  // q = (p - y) / (x - z) for p of L coefficients; a nonzero remainder fails with `err`
  int synth_div(const uint64_t* p, uint64_t L, const U256& z, const U256& y, uint64_t* q, const char* err) {
    if (L < 2) return fail(PBF_EINVAL, "synthetic division of a constant");
    DevBuf& rb = ctx->buf("pv.hs_rem");
    int rc = rb.ensure(32);
    if (!rc) rc = synth_div_run(p, L, z, y, q, (uint64_t*)rb.p);
    if (rc) return rc;
    hipLaunchKernelGGL(k_nonzero, dim3(1), dim3(64), 0, s, (const uint64_t*)rb.p, 0, 1, d_bad);
    PBF_HIP(hipGetLastError());
    return check_bad(err);
  }

  // ---- sharded layouts (G > 1): rows, SS and CR vectors (see XPose)
  uint64_t B = 0;        // rows per rank: n / G
  uint64_t Ls = 0, Bc = 0;  // CR span (n; 2n in mode 0, whose r(x) has 2n + 2 coefficients), Ls / G
  uint64_t crlo() const { return (uint64_t)rank * Bc; }
  uint64_t crlen() const { return Bc + (rank == G - 1 ? TAILC : 0); }
  uint64_t CRS() const { return Bc + TAILC; }  // CR vector stride in the rank's buffers
  uint64_t SSS() const { return B + TAILC; }   // SS vector (of <= n + TAILC coefficients) stride
  uint64_t cr_count(uint64_t L) const {        // coefficients j < L in this rank's range
    const uint64_t lo = crlo();
    return L <= lo ? 0 : std::min<uint64_t>(L - lo, crlen());
  }
  uint64_t ss_count(uint64_t L) const { return L <= rank ? 0 : (L - rank + G - 1) / G; }  // slots with j < L
  BlindMap bmap(const Blind& b, bool ss) const {
    BlindMap m;
    m.b = b; m.ss = ss ? 1u : 0u; m.G = G; m.rank = rank; m.Ls = Ls; m.Bc = Bc;
    return m;
  }
  // Every rank's *d_bad, all-gathered: any set fails every rank with `err` (so no rank waits in
  // a collective the failed one never reaches)
  int agree(const char* err) {
    PBF_HIP(hipMemsetAsync(comm->send, 0, 8, s));
    PBF_HIP(hipMemcpyAsync(comm->send, d_bad, sizeof(int), hipMemcpyDeviceToDevice, s));
    int rc = ag(8);
    if (rc) return rc;
    std::vector<int> h(2 * G);
    PBF_HIP(hipMemcpyAsync(h.data(), comm->recv, 8 * G, hipMemcpyDeviceToHost, s));
    PBF_HIP(hipStreamSynchronize(s));
    for (uint32_t g = 0; g < G; ++g)
      if (h[2 * g]) return fail(PBF_EINVAL, err);
    return 0;
  }
  // cnt canonical field elements at d_vals from every rank: out[g * cnt + i] (Montgomery)
  int gather(const uint64_t* d_vals, int cnt, std::vector<U256>& out) {
    PBF_HIP(hipMemcpyAsync(comm->send, d_vals, (size_t)cnt * 32, hipMemcpyDeviceToDevice, s));
    int rc = ag((size_t)cnt * 32);
    if (rc) return rc;
    std::vector<uint64_t> h((size_t)4 * cnt * G);
    PBF_HIP(hipMemcpyAsync(h.data(), comm->recv, h.size() * 8, hipMemcpyDeviceToHost, s));
    PBF_HIP(hipStreamSynchronize(s));
    out.resize((size_t)cnt * G);
    for (size_t i = 0; i < out.size(); ++i) out[i] = hm(h.data() + 4 * i);
    return 0;
  }
  // SS -> CR (one all-to-all): part k of the source vectors becomes cr[k] (CRS slots, zeroed here)
  int xpose(int P, const uint64_t* const* ss, uint64_t ss_slots, const uint64_t* off, const uint64_t* len,
            uint64_t* const* cr) {
    XPose x;
    for (int k = 0; k < P; ++k) {
      x.ss[k] = ss[k]; x.cr[k] = cr[k]; x.off[k] = off[k]; x.len[k] = len[k];
      PBF_HIP(hipMemsetAsync(cr[k], 0, CRS() * 32, s));
    }
    x.ss_slots = ss_slots; x.Ls = Ls; x.Bc = Bc; x.cap = Bc / G + (TAILC + G - 1) / G;
    x.G = G; x.rank = rank; x.P = (uint32_t)P;
    if ((uint64_t)G * P * x.cap * 32 > comm->capacity) return fail(PBF_EINVAL, "comm buffers too small for a transpose");
    hipLaunchKernelGGL(k_xpose_pack, dim3(blocks_for(ss_slots)), dim3(256), 0, s, x, (uint64_t*)comm->send);
    PBF_HIP(hipGetLastError());
    int rc = a2a((size_t)P * x.cap * 32);
    if (rc) return rc;
    hipLaunchKernelGGL(k_xpose_unpack, dim3(blocks_for((uint64_t)G * P * x.cap)), dim3(256), 0, s, x,
                       (const uint64_t*)comm->recv);
    PBF_HIP(hipGetLastError());
    return 0;
  }
  // k coset NTTs (this rank's blocks) of SS coefficient vectors of lens[i] coefficients
  int coset_ntt_ss(int k, const uint64_t* const* ss, const uint64_t* lens, const U256* bases, uint64_t* out,
                   const int* degs = nullptr) {
    uint64_t* sh = (uint64_t*)shard->p;
    for (int i = 0; i < k; ++i)
      scale(ss[i], 0, 1, ss_count(lens[i]), sh + 4 * nl * i, nl, bases[i], rank, G, degs ? degs[i] : 0);
    PBF_HIP(hipGetLastError());
    // the sharded forward NTT of the k stride shards in the staging buffer into this rank's blocks
    int rc = pbf_ntt_fr256_shard_local_dev(ctx, wN_plain, G, sh, (uint64_t*)comm->send, nl, k, 0, s);
    if (!rc) rc = a2a((size_t)k * S * 32);
    if (!rc) rc = pbf_ntt_fr256_shard_combine_dev(ctx, wN_plain, G, rank, (const uint64_t*)comm->recv, out, nl, k, 0, s);
    return rc;
  }
  // the SS coefficients (nl slots, j = rank + G m < N) of the polynomial whose coset
  // evaluations are this rank's blocks `ev`
  int coset_intt_ss(const uint64_t* ev, uint64_t* ss_out) {
    uint64_t* sh = (uint64_t*)shard->p;
    int rc = pbf_ntt_fr256_shard_combine_dev(ctx, wN_plain, G, rank, ev, (uint64_t*)comm->send, nl, 1, 1, s);
    if (!rc) rc = a2a(S * 32);
    if (!rc) rc = pbf_ntt_fr256_shard_local_dev(ctx, wN_plain, G, (const uint64_t*)comm->recv, sh, nl, 1, 1, s);
    if (rc) return rc;
    scale(sh, 0, 1, nl, ss_out, nl, g_inv, rank, G);  // u_j g^-j, j = rank + G m
    PBF_HIP(hipGetLastError());
    return 0;
  }
  // commitment of a CR vector of L coefficients: this rank's point range of the SRS (its window
  // table covers exactly SRS[crlo, crlo + crlen)), the partial sum left in `slot`
  int commit_cr(const uint64_t* cr, uint64_t L, int slot) {
    const uint64_t cnt = cr_count(L);
    if (cnt > srs_n) return fail(PBF_EINVAL, "SRS too short for a sharded commitment");
    if (cnt) return msm_fixed_device(ctx, srs_tbl, srs_n, 0, cr, cnt, s, slots + slot);
    PBF_HIP(hipMemsetAsync(slots + slot, 0, sizeof(Xyzz), s));  // ZZ = 0: the identity
    return 0;
  }
  // q = (p - y) / (x - z) for the CR vector p of L coefficients (global): every rank divides its
  // range (T_r = its value at z relative to its first index), the T_r are all-gathered, the
  // remainder sum_r T_r z^lo_r - y must be zero (checked on every rank), and each rank adds the
  // contribution of the coefficients above its range (k_hs_carry)
  int synth_div_cr(const uint64_t* p, uint64_t L, const U256& z, const U256& y, uint64_t* q, const char* err) {
    const uint64_t cnt = cr_count(L);
    DevBuf& rb = ctx->buf("pv.hs_rem");
    int rc = rb.ensure(32);
    if (rc) return rc;
    uint64_t* rem = (uint64_t*)rb.p;
    PBF_HIP(hipMemsetAsync(q, 0, CRS() * 32, s));
    if (cnt >= 2) {
      if ((rc = synth_div_run(p, cnt, z, u256_zero(), q, rem))) return rc;
    } else if (cnt == 1) {
      PBF_HIP(hipMemcpyAsync(rem, p, 32, hipMemcpyDeviceToDevice, s));
    } else {
      PBF_HIP(hipMemsetAsync(rem, 0, 32, s));
    }
    std::vector<U256> T;
    if ((rc = gather(rem, 1, T))) return rc;
    U256 value = u256_zero(), V = u256_zero();
    const uint64_t hi = crlo() + cnt;
    for (uint32_t g = 0; g < G; ++g) {
      const uint64_t lo_g = (uint64_t)g * Bc;
      value = Fr::add(value, Fr::mul(T[g], fr_pow(z, lo_g)));
      if (g > rank) V = Fr::add(V, Fr::mul(T[g], fr_pow(z, lo_g - hi)));  // nonzero only above a full range
    }
    if (!Fr::is_zero(Fr::sub(value, y))) return fail(PBF_EINVAL, err);
    if (cnt)
      hipLaunchKernelGGL(k_hs_carry, dim3(blocks_for((cnt + PV_CHUNK - 1) / PV_CHUNK)), dim3(256), 0, s, q, cnt, z,
                         Fr::from_mont(V));
    PBF_HIP(hipGetLastError());
    return 0;
  }
  // commitments lo .. hi - 1 as canonical affine points, on one GPU: a round's share of what
  // finish_commits collects at the end (the _fs entries: the next challenge waits on them)
  int collect(int lo, int hi, uint64_t (*out)[8]) {
    Xyzz h[9];
    int rc = msm_fixed_wait(ctx, s);
    if (rc) return rc;
    PBF_HIP(hipMemcpyAsync(h, slots + lo, (size_t)(hi - lo) * sizeof(Xyzz), hipMemcpyDeviceToHost, s));
    PBF_HIP(hipStreamSynchronize(s));
    for (int k = lo; k < hi; ++k) xyzz_to_affine_u64(h[k - lo], out[k]);
    return 0;
  }
  int finish_commits(int count, uint64_t (*out)[8]) {
    std::vector<Xyzz> h((size_t)count * G);  // [rank][commitment]
    int rc = msm_fixed_wait(ctx, s);
    if (rc) return rc;
    if (G == 1) {
      PBF_HIP(hipMemcpyAsync(h.data(), slots, h.size() * sizeof(Xyzz), hipMemcpyDeviceToHost, s));
    } else {
      // the partial sums of every commitment in as few all-gathers as the comm buffers allow
      // (one for any n >= 64; capacity >= 16 (4n / G) 32 B always holds G of them)
      const int per = (int)std::min<size_t>((size_t)count, comm->capacity / ((size_t)G * sizeof(Xyzz)));
      if (per < 1) return fail(PBF_EINVAL, "comm buffers too small for the commitment all-gather");
      for (int k0 = 0; k0 < count; k0 += per) {
        const int m = std::min(per, count - k0);
        PBF_HIP(hipMemcpyAsync(comm->send, slots + k0, (size_t)m * sizeof(Xyzz), hipMemcpyDeviceToDevice, s));
        if ((rc = ag((size_t)m * sizeof(Xyzz)))) return rc;
        for (uint32_t r = 0; r < G; ++r)
          PBF_HIP(hipMemcpyAsync(h.data() + (size_t)r * count + k0, (const Xyzz*)comm->recv + (size_t)r * m,
                                 (size_t)m * sizeof(Xyzz), hipMemcpyDeviceToHost, s));
      }
    }
    PBF_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < count; ++k) {
      Xyzz acc = h[k];
      for (uint32_t r = 1; r < G; ++r) acc = G1::add(acc, h[(size_t)r * count + k]);
      xyzz_to_affine_u64(acc, out[k]);
    }
    return 0;
  }
};

// What prove_setup leaves for prove_single / prove_sharded: the validated inputs in Montgomery
// form, the initialised Prover, the scratch buffers and the slot tables.
struct ProveState {
  Prover P;
  ProverBufs B;  // context-owned scratch (one ctx per host thread, pbf.h)
  int mode = 0;
  const uint64_t *d_q = nullptr, *d_copies = nullptr, *d_abc = nullptr;
  const uint64_t* d_pub = nullptr;  // public inputs (one GPU; npub = 0: none)
  uint64_t npub = 0;
  PlonkChallenges ch;
  // Fiat-Shamir (pbf_plonk_prove_bn254_fs*, one GPU): the circuit digest h0 in place of challenges;
  // ch is then filled round by round. out_chal: null, or alpha beta gamma z v u as derived
  bool fs = false;
  uint64_t fs_h0[4];
  uint64_t* out_chal = nullptr;
  U256 bl[9];  // the blinders b1..b9
  // proving key: on (option prover.pk), found valid in the context, and the key to store once built
  bool pk_on = false, pk_hit = false;
  std::vector<uint64_t> pk_key;
  uint64_t* pkcoef = nullptr;
  // coefficient slots: 0 a, 1 b, 2 c, 3 q_l, 4 q_r, 5 q_o, 6 q_m, 7 q_c, 8 s1, 9 s2, 10 s3 (3.. in
  // the proving key); coset slots: 0 a 1 b 2 c 3 z 4 ql 5 qr 6 qo 7 qm 8 qc 9 s1 10 s2 11 s3 12 l1
  // [13 z(w x), sharded]
  uint64_t *cslot[11], *ceslot[14];
  uint64_t *out_pts = nullptr, *out_f = nullptr;
  explicit ProveState(pbf_ctx* ctx) : B(ctx) {}
};

// a(x) = (b2 + b1 x)(x^n - 1) + f_a(x), likewise b, c (plonk.rs:250-252): lo = b2, hi = b1
Blind blind_abc(uint64_t n, const U256& lo, const U256& hi) {
  Blind b;
  b.count = 4;
  b.idx[0] = 0; b.delta[0] = Fr::sub(u256_zero(), lo);
  b.idx[1] = 1; b.delta[1] = Fr::sub(u256_zero(), hi);
  b.idx[2] = n; b.delta[2] = lo;
  b.idx[3] = n + 1; b.delta[3] = hi;
  return b;
}
// z(x) = (b9 + b8 x + b7 x^2)(x^n - 1) + acc(x)   (plonk.rs:309)
Blind blind_z(uint64_t n, const U256* bl) {
  Blind b;
  b.count = 6;
  const U256 c0 = bl[8], c1 = bl[7], c2 = bl[6];
  b.idx[0] = 0; b.delta[0] = Fr::sub(u256_zero(), c0);
  b.idx[1] = 1; b.delta[1] = Fr::sub(u256_zero(), c1);
  b.idx[2] = 2; b.delta[2] = Fr::sub(u256_zero(), c2);
  b.idx[3] = n; b.delta[3] = c0;
  b.idx[4] = n + 1; b.delta[4] = c1;
  b.idx[5] = n + 2; b.delta[5] = c2;
  return b;
}
// the quotient kernel's arguments over the coset slots CE(0..12) and z(w x) at `zw` (null: read
// from z at index i + 4), with the constants at the R-degrees the quotient's terms need
// (QuotArgs): Montgomery form is degree 1
int quot_args(const ProveState& S, const uint64_t* zw, QuotArgs& qa) {
  const Prover& P = S.P;
  uint64_t* const* CE = S.ceslot;
  qa.a = CE[0]; qa.b = CE[1]; qa.c = CE[2]; qa.z = CE[3]; qa.ql = CE[4]; qa.qr = CE[5]; qa.qo = CE[6];
  qa.qm = CE[7]; qa.qc = CE[8]; qa.s1 = CE[9]; qa.s2 = CE[10]; qa.s3 = CE[11]; qa.l1 = CE[12];
  qa.zw = zw;
  qa.N = P.count();
  qa.N_all = P.N;
  qa.blk = P.blk();
  qa.beta0 = Fr::from_mont(S.ch.beta);
  qa.gamma0 = Fr::from_mont(S.ch.gamma);
  qa.alpha4 = Fr::to_mont(Fr::to_mont(Fr::to_mont(S.ch.alpha)));
  qa.k1 = S.ch.k1; qa.k2 = S.ch.k2;
  qa.alpha2 = Fr::mul(S.ch.alpha, S.ch.alpha);
  qa.g = P.g; qa.wN = P.omegaN;
  // Z_H(g w_N^i) = g^n w_4^(i mod 4) - 1
  const U256 w4 = fr_pow(P.omegaN, P.n);
  U256 x = fr_pow(P.g, P.n);
  for (int j = 0; j < 4; ++j) {
    const U256 d = Fr::sub(x, fr_one_m());
    if (Fr::is_zero(d)) return fail(PBF_EINVAL, "coset meets H");
    qa.zh_inv[j] = fr_inv(d);
    x = Fr::mul(x, w4);
  }
  return 0;
}
// a_z b_z c_z s1_z s2_z r_z zw_z, canonical: the proof's field elements
void write_proof_fields(uint64_t* out_f, const PlonkEvals& e) {
  const U256 fo[7] = {e.a_z, e.b_z, e.c_z, e.s1_z, e.s2_z, e.r_z, e.zw_z};
  for (int i = 0; i < 7; ++i) hout(out_f + 4 * i, fo[i]);
}

}  // namespace

// ---- Plonk::prove across G ranks (pbf_plonk_prove_bn254_sharded_dev). Every
// witness-dependent step runs on this rank's share, with the layouts of XPose: rows
// [r B, (r + 1) B) of H; stride shards (SS) out of and into the sharded NTTs; contiguous ranges
// (CR) for commitments, evaluations, linear combinations and the opening divisions. Collectives
// (comm callbacks, stream-ordered on P.s): the NTTs' all-to-alls, SS -> CR transposes, and
// all-gathers of a few field elements (flags, scan totals, evaluation partials, division
// totals) and of the commitments' partial sums. The proving key (circuit polynomials) is built
// once per circuit with full-length coefficient slots on every rank and this rank's coset blocks.
static int prove_sharded(ProveState& S) {
  Prover& P = S.P;
  ProverBufs& B = S.B;
  pbf_ctx* ctx = P.ctx;
  const hipStream_t s = P.s;
  const int mode = S.mode;
  const uint64_t *d_q = S.d_q, *d_copies = S.d_copies, *d_abc = S.d_abc;
  const U256 &k1 = S.ch.k1, &k2 = S.ch.k2, &beta = S.ch.beta, &gamma = S.ch.gamma, &zc = S.ch.z;
  const uint64_t n = P.n, G = P.G, r = P.rank, Bn = P.B, Sn = Bn / G, NE = P.nl;
  const uint64_t E = 32, CRS = P.CRS(), SSS = P.SSS();
  const U256 one = fr_one_m();
  auto C = [&](int k) { return S.cslot[k]; };
  auto CE = [&](int k) { return S.ceslot[k]; };
  int rc;
  // ---- this rank's pieces
  DevBuf& shb = ctx->buf("pv.sh");
  const uint64_t sh_elems = 3 * Bn + 3 * SSS + 3 * CRS   // abc: blocked evaluations / INTT out, SS, CR
                            + 3 * Bn + 3 * Bn + Bn        // sigma rows, num / den, acc rows
                            + SSS + CRS                   // z: SS, CR
                            + NE + 3 * CRS                // t: SS over 4n, parts CR
                            + 4 * CRS + 2 * NE            // r, numerator, W_z, W_zw; quotient, mode-0 r_3 evaluations
                            + (mode == 0 ? NE + CRS : 0) + (Bn / SCAN_BLK + 2) + 4;
  if ((rc = shb.ensure(sh_elems * E))) return rc;
  uint64_t* cur = (uint64_t*)shb.p;
  auto take = [&](uint64_t elems) { uint64_t* p = cur; cur += 4 * elems; return p; };
  uint64_t* X = take(3 * Bn);
  uint64_t *abc_ss = take(3 * SSS), *abc_cr = take(3 * CRS);
  uint64_t *sig = take(3 * Bn), *num = take(Bn), *den = take(Bn), *accr = take(Bn);
  take(Bn);  // spare row buffer (scan input padding)
  uint64_t *z_ss = take(SSS), *z_cr = take(CRS);
  uint64_t *t_ss = take(NE), *t_cr = take(3 * CRS);
  uint64_t *rx = take(CRS), *numer = take(CRS), *wz = take(CRS), *wzw = take(CRS);
  uint64_t *Wq = take(NE), *W2 = take(NE);
  uint64_t* r3_ss = mode == 0 ? take(NE) : nullptr;
  uint64_t* r3_cr = mode == 0 ? take(CRS) : nullptr;
  uint64_t* totals = take(Bn / SCAN_BLK + 2);
  uint64_t* tot = take(1);
  uint64_t* hpow = (uint64_t*)B.hpow.p;
  uint64_t* l1 = (uint64_t*)B.tmp0.p;
  uint64_t* send = (uint64_t*)P.comm->send;
  uint64_t* recv = (uint64_t*)P.comm->recv;

  // ---- satisfies (constraints.rs:198-230) on this rank's rows, agreed by every rank
  hipLaunchKernelGGL(k_satisfies<false>, dim3(blocks_for(Bn)), dim3(256), 0, s, d_q, d_abc, d_copies, n, r * Bn, Bn,
                     (const uint64_t*)nullptr, (uint64_t)0, P.d_bad);
  PBF_HIP(hipGetLastError());
  if ((rc = P.agree("constraints not satisfied by the assignment (constraints.rs:198)"))) return rc;
  P.mark("satisfies (rows)");
  // ---- h = w^i (all of H: copy labels point anywhere)
  hipLaunchKernelGGL(k_powers29, dim3(blocks_for((n + PV_CHUNK - 1) / PV_CHUNK)), dim3(256), 0, s, hpow, n, powers_tab29(P.omega, one));
  PBF_HIP(hipGetLastError());
  const U256 ninv = fr_inv(hm64(n));
  // ---- proving key, sharded like the witness (once per circuit; every proof without the key):
  // the 8 circuit polynomials by one sharded INTT of their blocked evaluations (q columns, sigma
  // labels of the blocked rows), their coset blocks from the SS coefficients, their CR ranges by
  // transposes; l1 = n^-1 (1 + x + ... + x^(n-1)) is n^-1 in every slot of both layouts
  if (!S.pk_hit) {
    DevBuf& pkb = ctx->buf("pv.pkb");
    if ((rc = pkb.ensure(2 * 8 * Bn * E))) return rc;
    uint64_t* Xk = (uint64_t*)pkb.p;
    uint64_t* Yk = Xk + 4 * 8 * Bn;
    for (int k = 0; k < 5; ++k)
      PBF_HIP(hipMemcpy2DAsync(Xk + 4 * Bn * k, Sn * E, d_q + 4 * (n * k + r * Sn), Bn * E, Sn * E, G,
                               hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_sigma_blk, dim3(blocks_for(3 * Bn)), dim3(256), 0, s, d_copies, (const uint64_t*)hpow, n, Bn,
                       Sn, r, k1, k2, Xk + 4 * Bn * 5, P.d_bad);
    PBF_HIP(hipGetLastError());
    if ((rc = P.agree("copy constraint label out of range (plonk.rs:181-189)"))) return rc;
    if ((rc = pbf_ntt_fr256_shard_combine_dev(ctx, P.w_plain, (uint32_t)G, (uint32_t)r, Xk, send, Bn, 8, 1, s))) return rc;
    if ((rc = P.a2a(8 * Sn * E))) return rc;
    if ((rc = pbf_ntt_fr256_shard_local_dev(ctx, P.w_plain, (uint32_t)G, recv, Yk, Bn, 8, 1, s))) return rc;
    uint64_t* l1_ss = Xk;  // the blocked evaluations are consumed
    hipLaunchKernelGGL(k_powers29, dim3(blocks_for((Bn + PV_CHUNK - 1) / PV_CHUNK)), dim3(256), 0, s, l1_ss, Bn,
                       powers_tab29(one, ninv));
    PBF_HIP(hipGetLastError());
    const uint64_t lens[5] = {n, n, n, n, n};
    const U256 bases[5] = {P.g, P.g, P.g, P.g, P.g};
    const uint64_t* ss1[5] = {Yk, Yk + 4 * Bn, Yk + 8 * Bn, Yk + 12 * Bn, Yk + 16 * Bn};  // q_l q_r q_o q_m q_c
    if ((rc = P.coset_ntt_ss(5, ss1, lens, bases, CE(4), QUOT_DEG + 4))) return rc;
    const uint64_t* ss2[4] = {Yk + 20 * Bn, Yk + 24 * Bn, Yk + 28 * Bn, l1_ss};  // s1 s2 s3 l1
    if ((rc = P.coset_ntt_ss(4, ss2, lens, bases, CE(9), QUOT_DEG + 9))) return rc;
    for (int k0 = 0; k0 < 8; k0 += 3) {
      const int np = std::min(3, 8 - k0);
      const uint64_t* ss[3];
      uint64_t* cr[3];
      uint64_t off[3], len[3];
      for (int i = 0; i < np; ++i) {
        ss[i] = Yk + 4 * Bn * (k0 + i); cr[i] = C(3 + k0 + i); off[i] = 0; len[i] = n;
      }
      if ((rc = P.xpose(np, ss, Bn, off, len, cr))) return rc;
    }
    pkb.release();
    if (S.pk_on) ctx->pk_key = S.pk_key;
  }
  {  // l1's CR range: n^-1 for j < n
    PBF_HIP(hipMemsetAsync(l1, 0, CRS * E, s));
    const uint64_t cnt = P.cr_count(n);
    if (cnt)
      hipLaunchKernelGGL(k_powers29, dim3(blocks_for((cnt + PV_CHUNK - 1) / PV_CHUNK)), dim3(256), 0, s, l1, cnt,
                         powers_tab29(one, ninv));
    PBF_HIP(hipGetLastError());
  }
  P.mark(S.pk_hit ? "proving key (cached)" : "proving key (built)");

  // ---- round 1: interpolate_at_h of a b c (plonk.rs:233-243) = one sharded INTT of their
  // blocked evaluations: blocked slot q Sn + kk <- row q B + r Sn + kk of every column
  for (int col = 0; col < 3; ++col)
    PBF_HIP(hipMemcpy2DAsync(X + 4 * Bn * col, Sn * E, d_abc + 4 * (n * col + r * Sn), Bn * E, Sn * E, G,
                             hipMemcpyDeviceToDevice, s));
  if ((rc = pbf_ntt_fr256_shard_combine_dev(ctx, P.w_plain, (uint32_t)G, (uint32_t)r, X, send, Bn, 3, 1, s))) return rc;
  if ((rc = P.a2a(3 * Sn * E))) return rc;
  if ((rc = pbf_ntt_fr256_shard_local_dev(ctx, P.w_plain, (uint32_t)G, recv, X, Bn, 3, 1, s))) return rc;
  PBF_HIP(hipMemsetAsync(abc_ss, 0, 3 * SSS * E, s));
  PBF_HIP(hipMemcpy2DAsync(abc_ss, SSS * E, X, Bn * E, Bn * E, 3, hipMemcpyDeviceToDevice, s));
  // a(x) = (b2 + b1 x)(x^n - 1) + f_a(x), likewise b, c (plonk.rs:250-252), on the SS pieces
  for (int k = 0; k < 3; ++k)
    hipLaunchKernelGGL(k_blind_map, dim3(1), dim3(64), 0, s, abc_ss + 4 * SSS * k,
                       P.bmap(blind_abc(n, S.bl[2 * k + 1], S.bl[2 * k]), true));
  PBF_HIP(hipGetLastError());
  {
    const uint64_t* ss[3] = {abc_ss, abc_ss + 4 * SSS, abc_ss + 8 * SSS};
    uint64_t* cr[3] = {abc_cr, abc_cr + 4 * CRS, abc_cr + 8 * CRS};
    const uint64_t off[3] = {0, 0, 0}, len[3] = {n + 2, n + 2, n + 2};
    if ((rc = P.xpose(3, ss, SSS, off, len, cr))) return rc;
  }
  for (int k = 0; k < 3; ++k)
    if ((rc = P.commit_cr(abc_cr + 4 * CRS * k, n + 2, k))) return rc;
  P.mark("round 1 (sharded INTT, 3 MSM)");

  // ---- round 2: accumulator (plonk.rs:278-313) over this rank's rows: terms, batch division,
  // local exclusive prefix products, the ranks' totals all-gathered
  hipLaunchKernelGGL(k_sigma, dim3(blocks_for(3 * Bn)), dim3(256), 0, s, d_copies, (const uint64_t*)hpow, n, r * Bn, Bn,
                     k1, k2, sig, P.d_bad);
  hipLaunchKernelGGL(k_perm_terms, dim3(blocks_for(Bn)), dim3(256), 0, s, d_abc, (const uint64_t*)sig,
                     (const uint64_t*)hpow, n, r * Bn, Bn, beta, Fr::from_mont(gamma), k1, k2, num, den);
  const uint64_t terms = r + 1 == G ? Bn - 1 : Bn;  // ratios j < n - 1
  if ((rc = div_batch(ctx, (const uint64_t*)num, (const uint64_t*)den, num, terms, P.d_bad, s))) return rc;
  if (terms < Bn) {  // the last row's slot: 1 (canonical), so the local total is defined
    const uint64_t one_c[4] = {1, 0, 0, 0};
    PBF_HIP(hipMemcpyAsync(num + 4 * (Bn - 1), one_c, E, hipMemcpyHostToDevice, s));
  }
  if ((rc = P.agree("zero permutation denominator (plonk.rs:297 unwrap)"))) return rc;
  {
    const uint64_t nb = (Bn + SCAN_BLK - 1) / SCAN_BLK;
    hipLaunchKernelGGL(k_scan1, dim3((uint32_t)nb), dim3(SCAN_T), 0, s, (const uint64_t*)num, den, Bn, totals);
    hipLaunchKernelGGL(k_scan2, dim3(1), dim3(SCAN_T), 0, s, totals, nb);
    hipLaunchKernelGGL(k_scan3, dim3(blocks_for(Bn)), dim3(256), 0, s, (const uint64_t*)den, accr, Bn,
                       (const uint64_t*)totals);
    hipLaunchKernelGGL(k_mul1, dim3(1), dim3(64), 0, s, (const uint64_t*)(accr + 4 * (Bn - 1)),
                       (const uint64_t*)(num + 4 * (Bn - 1)), tot);
    PBF_HIP(hipGetLastError());
  }
  {
    std::vector<U256> T;
    if ((rc = P.gather(tot, 1, T))) return rc;
    U256 Ep = one;  // product of the ratios of the rows before this rank's
    for (uint64_t g = 0; g < r; ++g) Ep = Fr::mul(Ep, T[g]);
    // acc rows times Ep, straight into the all-to-all's send buffer: rows [r B, (r + 1) B) in
    // order are the [dst][Sn] send layout that lands as the blocked layout of the INTT below
    const uint64_t* in[1] = {accr};
    if ((rc = fr_lincomb_run(1, in, &Bn, &Ep, u256_zero(), send, Bn, s))) return rc;
  }
  if ((rc = P.a2a(Sn * E))) return rc;  // recv: this rank's blocked rows
  if ((rc = pbf_ntt_fr256_shard_combine_dev(ctx, P.w_plain, (uint32_t)G, (uint32_t)r, recv, send, Bn, 1, 1, s))) return rc;
  if ((rc = P.a2a(Sn * E))) return rc;
  if ((rc = pbf_ntt_fr256_shard_local_dev(ctx, P.w_plain, (uint32_t)G, recv, X, Bn, 1, 1, s))) return rc;
  PBF_HIP(hipMemsetAsync(z_ss, 0, SSS * E, s));
  PBF_HIP(hipMemcpyAsync(z_ss, X, Bn * E, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(k_blind_map, dim3(1), dim3(64), 0, s, z_ss, P.bmap(blind_z(n, S.bl), true));
  PBF_HIP(hipGetLastError());
  {
    const uint64_t* ss[1] = {z_ss};
    uint64_t* cr[1] = {z_cr};
    const uint64_t off[1] = {0}, len[1] = {n + 3};
    if ((rc = P.xpose(1, ss, SSS, off, len, cr))) return rc;
  }
  if ((rc = P.commit_cr(z_cr, n + 3, 3))) return rc;
  P.mark("round 2 (rows, sharded INTT, MSM)");

  // ---- round 3: a b c z z(w x) on this rank's coset blocks, from their SS pieces
  {
    const uint64_t* ss[5] = {abc_ss, abc_ss + 4 * SSS, abc_ss + 8 * SSS, z_ss, z_ss};
    const uint64_t lens[5] = {n + 2, n + 2, n + 2, n + 3, n + 3};
    const U256 bases[5] = {P.g, P.g, P.g, P.g, Fr::mul(P.g, P.omega)};
    if ((rc = P.coset_ntt_ss(5, ss, lens, bases, CE(0)))) return rc;  // slots 0 1 2 3 and 13 (after 3)
  }
  QuotArgs qa;
  if ((rc = quot_args(S, CE(13), qa))) return rc;
  launch_quotient(qa, Wq, ctx->options.num("ntt256.l29", 1) != 0, s);
  PBF_HIP(hipGetLastError());
  if ((rc = P.coset_intt_ss(Wq, t_ss))) return rc;
  const uint64_t m = n + 2;  // coefficients per t part
  hipLaunchKernelGGL(k_nonzero, dim3(blocks_for(NE)), dim3(256), 0, s, (const uint64_t*)t_ss, P.ss_count(3 * m), NE,
                     P.d_bad);
  PBF_HIP(hipGetLastError());
  if ((rc = P.agree("t(x) = numerator / Z_H is not a polynomial of 3(n+2) coefficients (plonk.rs:370)"))) return rc;
  {
    const uint64_t* ss[3] = {t_ss, t_ss, t_ss};
    uint64_t* cr[3] = {t_cr, t_cr + 4 * CRS, t_cr + 8 * CRS};
    const uint64_t off[3] = {0, m, 2 * m}, len[3] = {m, m, m};
    if ((rc = P.xpose(3, ss, NE, off, len, cr))) return rc;
  }
  for (int k = 0; k < 3; ++k)
    if ((rc = P.commit_cr(t_cr + 4 * CRS * k, m, 4 + k))) return rc;
  P.mark("round 3 (sharded coset NTTs, quotient, 3 MSM)");

  // ---- round 4: evaluations at z (plonk.rs:393-399) as per-rank partial sums over the CR
  // ranges, all-gathered
  auto eval = [&](int np, const uint64_t* const* polys, const uint64_t* lens, const U256* xs, U256* res) -> int {
    uint64_t cnt[12];
    for (int i = 0; i < np; ++i) cnt[i] = P.cr_count(lens[i]);
    int rc2 = fr_eval_run(polys, cnt, xs, np, P.crlo(), B.partial, (uint64_t*)B.evals.p, s);
    if (rc2) return rc2;
    std::vector<U256> parts;
    if ((rc2 = P.gather((const uint64_t*)B.evals.p, np, parts))) return rc2;
    for (int i = 0; i < np; ++i) {
      res[i] = u256_zero();
      for (uint64_t g = 0; g < G; ++g) res[i] = Fr::add(res[i], parts[g * np + i]);
    }
    return 0;
  };
  // linear combinations over this rank's CR range
  auto lincomb = [&](int k, const uint64_t* const* in, const uint64_t* lens, const U256* c, const U256& c0,
                     uint64_t* out) -> int {
    uint64_t cnt[10];
    for (int i = 0; i < k; ++i) cnt[i] = P.cr_count(lens[i]);
    // the constant term is coefficient 0: rank 0's
    return fr_lincomb_run(k, in, cnt, c, r == 0 ? c0 : u256_zero(), out, CRS, s);
  };
  const U256 zw = Fr::mul(zc, P.omega);
  PlonkEvals e;
  {
    U256 ev[10];
    const uint64_t* polys[10] = {abc_cr, abc_cr + 4 * CRS, abc_cr + 8 * CRS, C(8), C(9), t_cr, t_cr + 4 * CRS,
                                 t_cr + 8 * CRS, z_cr, l1};
    const uint64_t lens[10] = {n + 2, n + 2, n + 2, n, n, m, m, m, n + 3, n};
    const U256 xs[10] = {zc, zc, zc, zc, zc, zc, zc, zc, zw, zc};
    if ((rc = eval(10, polys, lens, xs, ev))) return rc;
    e.a_z = ev[0]; e.b_z = ev[1]; e.c_z = ev[2]; e.s1_z = ev[3]; e.s2_z = ev[4]; e.zw_z = ev[8]; e.l1_z = ev[9];
    e.t_z = Fr::add(Fr::add(ev[5], Fr::mul(fr_pow(zc, m), ev[6])), Fr::mul(fr_pow(zc, 2 * m), ev[7]));
  }
  const uint64_t rlen = mode == 0 ? 2 * n + 2 : n + 3;
  if (mode == 0) {  // z(x) s_sigma_3(x), the polynomial of r_3 (plonk.rs:414-416): on the coset
    hipLaunchKernelGGL(k_mul, dim3(blocks_for(NE)), dim3(256), 0, s, (const uint64_t*)CE(3), (const uint64_t*)CE(11), W2,
                       NE);
    PBF_HIP(hipGetLastError());
    if ((rc = P.coset_intt_ss(W2, r3_ss))) return rc;
    const uint64_t* ss[1] = {r3_ss};
    uint64_t* cr[1] = {r3_cr};
    const uint64_t off[1] = {0}, len[1] = {2 * n + 2};
    if ((rc = P.xpose(1, ss, NE, off, len, cr))) return rc;
  }
  {  // r(x), all seven terms in one combination
    const uint64_t* in[7] = {C(6), C(3), C(4), C(5), C(7), z_cr, mode == 1 ? C(10) : r3_cr};
    const uint64_t lens[7] = {n, n, n, n, n, n + 3, mode == 1 ? n : 2 * n + 2};
    U256 c[7];
    plonk_r_coeffs(S.ch, e, mode, c);
    if ((rc = lincomb(7, in, lens, c, u256_zero(), rx))) return rc;
  }
  {
    const uint64_t* polys[1] = {rx};
    if ((rc = eval(1, polys, &rlen, &zc, &e.r_z))) return rc;
  }
  P.mark("round 4 (evaluation partials, r(x))");

  // ---- round 5: the opening quotients (plonk.rs:430-442) on the CR ranges
  {
    const uint64_t* in[9] = {t_cr, t_cr + 4 * CRS, t_cr + 8 * CRS, rx, abc_cr, abc_cr + 4 * CRS, abc_cr + 8 * CRS,
                             C(8), C(9)};
    const uint64_t lens[9] = {m, m, m, rlen, n + 2, n + 2, n + 2, n, n};
    U256 c[9];
    const U256 c0 = plonk_wz_coeffs(S.ch, e, n, c);
    if ((rc = lincomb(9, in, lens, c, c0, numer))) return rc;
  }
  const uint64_t lnum = rlen > m ? rlen : m;
  const uint64_t wlen = lnum - 1;
  if ((rc = P.synth_div_cr(numer, lnum, zc, u256_zero(), wz, "W_z division left a remainder (plonk.rs:438)"))) return rc;
  if ((rc = P.commit_cr(wz, wlen, 7))) return rc;
  if ((rc = P.synth_div_cr(z_cr, n + 3, zw, e.zw_z, wzw, "W_zw division left a remainder (plonk.rs:442)"))) return rc;
  if ((rc = P.commit_cr(wzw, n + 2, 8))) return rc;
  if ((rc = P.finish_commits(9, (uint64_t(*)[8])S.out_pts))) return rc;
  P.mark("round 5 (sharded divisions, 2 MSM)");
  write_proof_fields(S.out_f, e);
  return 0;
}

// What both provers need before their rounds: the arguments validated, the Prover initialised
// (comm == null or world 1: one GPU; else this rank's layouts), the proving-key state, the
// scratch buffers sized and the slot tables. S.mode, the device inputs and the outputs are set by
// the caller.
static int prove_setup(ProveState& S, pbf_ctx* ctx, const pbf_comm* comm, size_t n, const uint64_t* chal,
                       const uint64_t* rnd, const uint64_t* k1k2, const uint64_t* d_srs, size_t srs_m, void* stream) {
  const int mode = S.mode;
  const uint64_t *d_q = S.d_q, *d_copies = S.d_copies;
  if (n < 8 || (n & (n - 1))) return fail(PBF_EINVAL, "n must be a power of two >= 8");
  if (mode != 0 && mode != 1) return fail(PBF_EINVAL, "mode must be 0 (reference r_3) or 1 (paper)");
  PBF_HIP(hipSetDevice(ctx->device));
  uint32_t log_n = 0;
  while ((1ull << log_n) < n) ++log_n;
  if (log_n + 2 > 28) return fail(PBF_EINVAL, "4n exceeds the 2-adicity of Fr");
  const uint64_t need_srs = mode == 0 ? 2 * n + 2 : n + 3;  // longest committed polynomial
  if (srs_m < need_srs) return fail(PBF_EINVAL, "SRS too short for this n and mode");
  for (int i = 0; chal && i < 5; ++i)
    if (Fr::geq_p(u256_from_u64(chal + 4 * i))) return fail(PBF_EINVAL, "challenge not canonical");
  for (int i = 0; i < 9; ++i)
    if (Fr::geq_p(u256_from_u64(rnd + 4 * i))) return fail(PBF_EINVAL, "blinder not canonical");

  Prover& P = S.P;
  P.ctx = ctx;
  P.s = (hipStream_t)stream;
  P.timing = ctx->options.num("prover.timing", 0) != 0;
  P.mark("start");
  P.n = n;
  P.N = 4 * n;
  P.omega = fr_root_of_unity(log_n);
  P.omegaN = fr_root_of_unity(log_n + 2);
  P.g = hm64(5);  // coset shift: a quadratic non-residue, outside every 2^k subgroup
  P.g_inv = fr_inv(P.g);
  hout(P.w_plain, P.omega);
  hout(P.wN_plain, P.omegaN);
  if (comm && comm->world > 1) {
    const uint32_t G = comm->world;
    if (G != 2 && G != 4 && G != 8) return fail(PBF_EINVAL, "world size must be 2, 4 or 8");
    if (comm->rank >= G) return fail(PBF_EINVAL, "rank out of range");
    if (!comm->send || !comm->recv || !comm->all_to_all || !comm->all_gather) return fail(PBF_EINVAL, "incomplete comm");
    if ((uint64_t)n < (uint64_t)G * G) return fail(PBF_EINVAL, "n must be at least world^2 (sharded layouts)");
    P.comm = comm;
    P.G = G;
    P.rank = comm->rank;
    P.nl = 4 * (uint64_t)n / G;
    P.S = P.nl / G;
    P.B = n / G;
    P.Ls = mode == 0 ? 2 * (uint64_t)n : (uint64_t)n;  // mode 0's r(x) and W_z reach x^(2n+1)
    P.Bc = P.Ls / G;
    // the largest exchange: 5 coset NTTs of 4n / world points per rank (a b c z z(w x); the key's
    // 9 go as 5 + 4)
    if (comm->capacity < 5 * P.nl * 32) return fail(PBF_EINVAL, "comm buffers below 5 * (4n / world) * 32 bytes");
    P.shard = &ctx->buf("pv.shard");
    int rc0 = P.shard->ensure(5 * P.nl * 32);
    if (rc0) return rc0;
  }
  const hipStream_t s = P.s;
  const uint64_t N = P.N;
  const U256 k1 = hm(k1k2), k2 = hm(k1k2 + 4);
  // Plonk::new asserts (plonk.rs:133-138): k1, k2 not in H, k2 not in k1 H
  if (heq1(fr_pow(k1, n)) || heq1(fr_pow(k2, n)) || heq1(fr_pow(Fr::mul(k2, fr_inv(k1)), n)) || Fr::is_zero(k1) ||
      Fr::is_zero(k2))
    return fail(PBF_EINVAL, "k1/k2 do not give disjoint cosets of H");
  if (chal) {  // null: the _fs entries, whose rounds derive them
    S.ch.alpha = hm(chal); S.ch.beta = hm(chal + 4); S.ch.gamma = hm(chal + 8); S.ch.z = hm(chal + 12);
    S.ch.v = hm(chal + 16);
  }
  S.ch.k1 = k1; S.ch.k2 = k2;
  for (int i = 0; i < 9; ++i) S.bl[i] = hm(rnd + 4 * i);

  ProverBufs& B = S.B;
  const uint64_t E = 32;           // bytes per element
  const uint64_t CS = n + 8;       // coefficient slot (room for blinding terms up to x^(n+2))
  int rc;
  // ---- proving key (one GPU): q_l q_r q_o q_m q_c s1 s2 s3 and l1 depend only on the circuit
  // (d_q, d_copies, k1, k2) and n. Their coefficients (8 slots) and coset evaluations (9
  // slots) are kept in the context and reused while the circuit is the same -- what a
  // PLONK proving key holds -- validated on every call by comparing d_q and d_copies with the
  // context's device copies of the gates and copies the key was built from (exact content).
  // Option prover.pk = 0 recomputes them per proof, as the reference does (plonk.rs:233-243,
  // 339-370).
  const bool pk_on = ctx->options.num("prover.pk", 1) != 0;  // sharded too: this rank's coset blocks
  S.pk_on = pk_on;
  uint64_t* pkcoset = nullptr;
  std::vector<uint64_t>& pk_key = S.pk_key;
  if (pk_on) {
    const SnapItem items[2] = {{"q", d_q, 20 * (uint64_t)n}, {"copies", d_copies, 6 * (uint64_t)n}};
    bool same = false;
    if ((rc = snapshot_check(ctx, "pk", items, 2, s, &same))) return rc;
    if (!same) ctx->pk_key.clear();
    // sharded: the key's CR ranges follow Ls (2n in mode 0, n in mode 1), so the layout is part of the key
    pk_key = {(uint64_t)n, (uint64_t)P.G, (uint64_t)P.rank, P.G > 1 ? P.Ls : 0};
    for (int i = 0; i < 8; ++i) pk_key.push_back(k1k2[i]);
    DevBuf& kc = ctx->buf("pk.coef");
    DevBuf& ks = ctx->buf("pk.coset");
    if ((rc = kc.ensure(8 * (P.G > 1 ? P.CRS() : CS) * E)) || (rc = ks.ensure(9 * P.count() * E))) return rc;
    S.pkcoef = (uint64_t*)kc.p;
    pkcoset = (uint64_t*)ks.p;
    S.pk_hit = ctx->pk_key == pk_key;
    if (!S.pk_hit) ctx->pk_key.clear();  // the slots are rewritten below; valid again once complete
  }
  // sharded: full-length scratch only where the proving key is built (the circuit's polynomials
  // on every rank); the witness-dependent vectors live in this rank's SS / CR pieces ("pv.sh")
  const bool sharded = P.G > 1;
  const uint64_t n_full = sharded ? 0 : n;
  if ((rc = B.hpow.ensure(n * E)) || (rc = B.sigma.ensure((sharded ? 0 : 3 * n) * E)) ||
      (rc = B.coef.ensure(sharded ? (pk_on ? 0 : 11 * P.CRS() * E) : 11 * (n + 8) * E)) ||
      (rc = B.acc.ensure((n_full + 8) * E)) || (rc = B.tmp0.ensure((sharded ? P.CRS() : n) * E)) ||
      (rc = B.tmp1.ensure((n_full + 8) * E)) ||
      (rc = B.tmp2.ensure((n / SCAN_BLK + 2) * E)) || (rc = B.coset.ensure((pk_on ? 5 : 14) * P.count() * E)) ||
      (rc = B.t.ensure((sharded ? 8 : N) * E)) || (rc = B.work.ensure((sharded ? 8 : 3 * N) * E)) ||
      (rc = B.flag.ensure(64)) || (rc = B.evals.ensure(16 * E)))
    return rc;
  P.d_bad = (int*)B.flag.p;
  PBF_HIP(hipMemsetAsync(P.d_bad, 0, sizeof(int), s));
  {
    DevBuf& sl = ctx->buf("pv.commits");
    if ((rc = sl.ensure(9 * sizeof(Xyzz)))) return rc;
    P.slots = (Xyzz*)sl.p;
    if (!sharded) {
      P.srs_n = srs_m;
      if ((rc = msm_fixed_table(ctx, d_srs, srs_m, s, &P.srs_tbl))) return rc;  // built once per SRS
    } else {
      // this rank's point range SRS[crlo, crlo + crlen) (contiguous: the CR ranges)
      if (P.crlo() >= srs_m) return fail(PBF_EINVAL, "SRS too short for this n, mode and world size");
      P.srs_n = std::min<uint64_t>(P.crlen(), srs_m - P.crlo());
      if ((rc = msm_fixed_table(ctx, d_srs + 8 * P.crlo(), P.srs_n, s, &P.srs_tbl))) return rc;
    }
  }
  // the slot tables (ProveState)
  uint64_t* coef = (uint64_t*)B.coef.p;
  const uint64_t cstride = sharded ? P.CRS() : CS;  // sharded: the circuit polynomials' CR ranges
  for (int k = 0; k < 11; ++k)
    S.cslot[k] = (pk_on && k >= 3) ? S.pkcoef + 4 * cstride * (k - 3) : coef + 4 * cstride * k;
  uint64_t* coset = (uint64_t*)B.coset.p;
  const uint64_t NE = P.count();  // coset evaluations held here (N; nl = N / G when sharded)
  for (int k = 0; k < 14; ++k)
    S.ceslot[k] = (pk_on && k >= 4 && k <= 12)  ? pkcoset + 4 * NE * (k - 4)
                  : ((pk_on || sharded) && k == 13) ? coset + 4 * NE * 4        // z(w x) after a b c z
                  : (sharded && k >= 4 && k <= 12)  ? coset + 4 * NE * (k + 1)  // no key: circuit slots after
                                                    : coset + 4 * NE * k;
  return 0;
}

// ---- Plonk::prove on one GPU: the reference's rounds on whole polynomials
static int prove_single(ProveState& S) {
  Prover& P = S.P;
  ProverBufs& B = S.B;
  pbf_ctx* ctx = P.ctx;
  const hipStream_t s = P.s;
  const int mode = S.mode;
  const bool pk_on = S.pk_on, pk_hit = S.pk_hit;
  const uint64_t *d_q = S.d_q, *d_copies = S.d_copies, *d_abc = S.d_abc;
  const U256 &k1 = S.ch.k1, &k2 = S.ch.k2, &beta = S.ch.beta, &gamma = S.ch.gamma, &zc = S.ch.z;
  const uint64_t n = P.n, N = P.N, NE = N, E = 32, CS = n + 8;
  const U256 one = fr_one_m();
  uint64_t *hpow = (uint64_t*)B.hpow.p, *sigma = (uint64_t*)B.sigma.p, *coef = (uint64_t*)B.coef.p;
  uint64_t* pkcoef = S.pkcoef;
  auto C = [&](int k) { return S.cslot[k]; };
  auto CE = [&](int k) { return S.ceslot[k]; };
  int rc;
  uint64_t* work = (uint64_t*)B.work.p;
  uint64_t* W0 = work;
  uint64_t* W1 = work + 4 * N;
  uint64_t* W2 = work + 8 * N;
  // Fiat-Shamir (S.fs): a round's commitments are collected when the round ends and its challenge
  // derived on the host before the next round is enqueued (transcript.hpp; fs_t the running digest)
  uint64_t(*const opts)[8] = (uint64_t(*)[8])S.out_pts;
  uint64_t fs_t[4];
  const auto fs_take = [&](U256& c, const uint64_t* t, int at) {  // c = t mod r, reported at out_chal[at]
    uint64_t l[4];
    fs_challenge(t, l);
    c = hm(l);
    if (S.out_chal) memcpy(S.out_chal + 4 * at, l, 32);
    memcpy(fs_t, t, 32);
  };

  // ---- satisfies (constraints.rs:198-230)
  const uint64_t* d_pub = S.d_pub;
  const uint64_t npub = S.npub;  // 0: the plain entries, and every launch below is theirs
  if (npub) {
    PBF_HIP(hipMemsetAsync(P.d_bad + 1, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_satisfies<true>, dim3(blocks_for(n)), dim3(256), 0, s, d_q, d_abc, d_copies, (uint64_t)n,
                       (uint64_t)0, (uint64_t)n, d_pub, npub, P.d_bad);
    PBF_HIP(hipGetLastError());
    int bad[2] = {0, 0};
    PBF_HIP(hipMemcpyAsync(bad, P.d_bad, sizeof(bad), hipMemcpyDeviceToHost, s));
    PBF_HIP(hipStreamSynchronize(s));
    if (bad[1]) return fail(PBF_EINVAL, "public input not canonical");
    if (bad[0]) return fail(PBF_EINVAL, "constraints not satisfied by the assignment (constraints.rs:198)");
  } else {
    hipLaunchKernelGGL(k_satisfies<false>, dim3(blocks_for(n)), dim3(256), 0, s, d_q, d_abc, d_copies, (uint64_t)n,
                       (uint64_t)0, (uint64_t)n, (const uint64_t*)nullptr, (uint64_t)0, P.d_bad);
    PBF_HIP(hipGetLastError());
    if ((rc = P.check_bad("constraints not satisfied by the assignment (constraints.rs:198)"))) return rc;
  }
  P.mark("satisfies");

  // ---- h = w^i, sigma labels (plonk.rs:124, 181-189, 222-224)
  if ((rc = sigma_table_run(n, P.omega, k1, k2, d_copies, hpow, sigma, P.d_bad, s))) return rc;
  // ---- interpolate_at_h of a b c q_l q_r q_o q_m q_c s1 s2 s3 = INTT (plonk.rs:233-243)
  // every slot's first n coefficients are written below (INTT outputs): only the tails [n, CS)
  // are cleared (round 6: the whole slots were, 1.5 GB at 2^24 rows)
  PBF_HIP(hipMemset2DAsync(coef + 4 * n, CS * E, 0, (CS - n) * E, pk_on ? 3 : 11, s));
  if (pk_on && !pk_hit) PBF_HIP(hipMemset2DAsync(pkcoef + 4 * n, CS * E, 0, (CS - n) * E, 8, s));
  // a b c: INTTs of the witness columns straight into their padded coefficient slots (round 6:
  // one batched INTT into the work buffer and three n-element copies before)
  for (int k = 0; k < 3; ++k)
    if ((rc = P.ntt(P.w_plain, d_abc + 4 * n * k, C(k), n, 1, 1))) return rc;
  if (!pk_hit) {
    for (int k = 0; k < 5; ++k)
      PBF_HIP(hipMemcpyAsync(C(3 + k), d_q + 4 * n * k, n * E, hipMemcpyDeviceToDevice, s));
    for (int k = 0; k < 3; ++k)
      PBF_HIP(hipMemcpyAsync(C(8 + k), sigma + 4 * n * k, n * E, hipMemcpyDeviceToDevice, s));
    for (int k = 3; k < 11; ++k)
      if ((rc = P.ntt(P.w_plain, C(k), C(k), n, 1, 1))) return rc;
  }
  P.mark(pk_hit ? "interpolate (3 INTT, key)" : "interpolate (11 INTT)");
  // ---- round 1: a(x) = (b2 + b1 x)(x^n - 1) + f_a(x), likewise b, c (plonk.rs:250-252)
  for (int k = 0; k < 3; ++k)  // (b2, b1), (b4, b3), (b6, b5)
    hipLaunchKernelGGL(k_blind, dim3(1), dim3(64), 0, s, C(k), blind_abc(n, S.bl[2 * k + 1], S.bl[2 * k]));
  PBF_HIP(hipGetLastError());
  for (int k = 0; k < 3; ++k)
    if ((rc = P.commit(C(k), n + 2, k))) return rc;
  P.mark("round 1 commits (3 MSM)");
  if (S.fs) {
    uint64_t root[4] = {0, 0, 0, 0}, Pd[4], t[4];
    if (npub) {  // P: the tree digest of pub, its levels on the device where pub is
      DevBuf& rb = ctx->buf("fs.roots");
      if ((rc = rb.ensure(32)) || (rc = fs_tree_run(ctx, d_pub, 1, npub, true, (uint64_t*)rb.p, s))) return rc;
      PBF_HIP(hipMemcpyAsync(root, rb.p, 32, hipMemcpyDeviceToHost, s));
    }
    if ((rc = P.collect(0, 3, opts))) return rc;  // synchronises s
    fs_tree_close(FS_TAG_PUB, npub, root, Pd);
    fs_round1(S.fs_h0, Pd, opts[0], t);
    fs_take(S.ch.beta, t, 1);
    fs_round<0, 0>(fs_t, 2, nullptr, nullptr, t);
    fs_take(S.ch.gamma, t, 2);
    P.mark("fs: a_s b_s c_s collected, beta gamma");
  }

  // ---- round 2: accumulator (plonk.rs:278-313)
  uint64_t* acc = (uint64_t*)B.acc.p;
  uint64_t* num = (uint64_t*)B.tmp0.p;
  uint64_t* den = (uint64_t*)B.tmp1.p;
  PBF_HIP(hipMemsetAsync(acc + 4 * n, 0, (CS - n) * E, s));  // k_scan3 writes the first n
  hipLaunchKernelGGL(k_perm_terms, dim3(blocks_for(n)), dim3(256), 0, s, d_abc, (const uint64_t*)sigma,
                     (const uint64_t*)hpow, (uint64_t)n, (uint64_t)0, (uint64_t)n, beta, Fr::from_mont(gamma), k1, k2, num,
                     den);
  if ((rc = div_batch(ctx, (const uint64_t*)num, (const uint64_t*)den, num, (uint64_t)(n - 1), P.d_bad, s))) return rc;
  if ((rc = P.check_bad("zero permutation denominator (plonk.rs:297 unwrap)"))) return rc;
  {
    const uint64_t nb = (n - 1 + SCAN_BLK - 1) / SCAN_BLK;
    uint64_t* totals = (uint64_t*)B.tmp2.p;
    hipLaunchKernelGGL(k_scan1, dim3((uint32_t)nb), dim3(SCAN_T), 0, s, (const uint64_t*)num, den, (uint64_t)(n - 1),
                       totals);
    hipLaunchKernelGGL(k_scan2, dim3(1), dim3(SCAN_T), 0, s, totals, nb);
    hipLaunchKernelGGL(k_scan3, dim3(blocks_for(n)), dim3(256), 0, s, (const uint64_t*)den, acc, (uint64_t)n,
                       (const uint64_t*)totals);
    PBF_HIP(hipGetLastError());
  }
  if ((rc = P.ntt(P.w_plain, acc, acc, n, 1, 1))) return rc;  // acc_x
  hipLaunchKernelGGL(k_blind, dim3(1), dim3(64), 0, s, acc, blind_z(n, S.bl));
  PBF_HIP(hipGetLastError());
  uint64_t* zx = acc;  // length n+3
  P.mark("round 2 accumulator");
  if ((rc = P.commit(zx, n + 3, 3))) return rc;
  P.mark("round 2 commit (MSM)");
  if (S.fs) {
    uint64_t t[4];
    if ((rc = P.collect(3, 4, opts))) return rc;
    fs_round<1, 0>(fs_t, 3, opts[3], nullptr, t);
    fs_take(S.ch.alpha, t, 0);
    P.mark("fs: z_s collected, alpha");
  }

  // ---- round 3: quotient on the coset g H_4n (plonk.rs:326-382)
  const int cmap[13] = {0, 1, 2, -1, 3, 4, 5, 6, 7, 8, 9, 10, -2};  // coef slot per coset slot
  // l_1(x) = interpolate([1, 0, ..., 0]) = n^-1 (1 + x + ... + x^(n-1)) (plonk.rs:328-332)
  const U256 ninv = fr_inv(hm64(n));
  {
    uint64_t* l1 = (uint64_t*)B.tmp0.p;
    hipLaunchKernelGGL(k_powers29, dim3(blocks_for((n + PV_CHUNK - 1) / PV_CHUNK)), dim3(256), 0, s, l1, (uint64_t)n,
                       powers_tab29(one, ninv));
    PBF_HIP(hipGetLastError());
  }
  {
    const uint64_t* srcs[13];
    uint64_t lens[13];
    U256 bases[13];
    for (int k = 0; k < 13; ++k) {
      if (cmap[k] == -1) { srcs[k] = zx; lens[k] = n + 3; }
      else if (cmap[k] == -2) { srcs[k] = (const uint64_t*)B.tmp0.p; lens[k] = n; }
      else { srcs[k] = C(cmap[k]); lens[k] = cmap[k] < 3 ? n + 2 : n; }
      bases[k] = P.g;
    }
    if (pk_on) {  // a b c z per proof, all canonical; the 9 circuit slots once per proving key
      if ((rc = P.coset_ntt_batch(4, srcs, lens, bases, CE(0)))) return rc;
      if (!pk_hit) {
        if ((rc = P.coset_ntt_batch(9, srcs + 4, lens + 4, bases + 4, CE(4), QUOT_DEG + 4))) return rc;
        ctx->pk_key = S.pk_key;
      }
    } else if ((rc = P.coset_ntt_batch(13, srcs, lens, bases, CE(0), QUOT_DEG))) {
      return rc;
    }
  }
  P.mark(pk_hit ? "round 3 coset NTTs (4, key)" : "round 3 coset NTTs (13)");
  QuotArgs qa;
  if ((rc = quot_args(S, nullptr, qa))) return rc;  // z(w x): z at index i + 4
  if (npub) {
    // t_1 gains PI(x) (plonk.rs:339-344 with public inputs): the quotient reads q_c(x) + PI(x) where
    // it read q_c(x), from a per-proof slot -- the key's q_c slot is left as it is. Its values on H
    // are q_c[i] - pub[i]; one INTT and one coset NTT make the 4n coset values, raw like the q_c
    // slot (QUOT_DEG[8]). W1 and W2 are free here: the round's transforms run in the context's NTT
    // scratch, the quotient writes W0, and r(x) takes W1 only in round 4.
    hipLaunchKernelGGL(k_qc_minus_pub, dim3(blocks_for(n)), dim3(256), 0, s, d_q + 16 * n, d_pub, npub, W1, (uint64_t)n);
    PBF_HIP(hipGetLastError());
    if ((rc = P.ntt(P.w_plain, W1, W1, n, 1, 1))) return rc;
    const uint64_t* src = W1;
    const uint64_t len = n;
    if ((rc = P.coset_ntt_batch(1, &src, &len, &P.g, W2, QUOT_DEG + 8))) return rc;
    qa.qc = W2;
    P.mark("round 3 public inputs (INTT + coset NTT)");
  }
  uint64_t* tq = (uint64_t*)B.t.p;
  launch_quotient(qa, W0, ctx->options.num("ntt256.l29", 1) != 0, s);
  PBF_HIP(hipGetLastError());
  if ((rc = P.coset_intt(W0, tq))) return rc;
  const uint64_t m = n + 2;  // coefficients per t part
  hipLaunchKernelGGL(k_nonzero, dim3(blocks_for(N - 3 * m)), dim3(256), 0, s, (const uint64_t*)tq, 3 * m, N, P.d_bad);
  PBF_HIP(hipGetLastError());
  if ((rc = P.check_bad("t(x) = numerator / Z_H is not a polynomial of 3(n+2) coefficients (plonk.rs:370)")))
    return rc;
  // (round 6: the mark now precedes the t_lo commitment, which rounds 4-5 counted here)
  P.mark("round 3 quotient + INTT");
  {
    if ((rc = P.commit(tq, m, 4))) return rc;            // t_lo
    if ((rc = P.commit(tq + 4 * m, m, 5))) return rc;    // t_mid
    if ((rc = P.commit(tq + 8 * m, m, 6))) return rc;    // t_hi
  }
  P.mark("round 3 commits (3 MSM)");
  if (S.fs) {
    uint64_t t[4];
    if ((rc = P.collect(4, 7, opts))) return rc;
    fs_round<3, 0>(fs_t, 4, opts[4], nullptr, t);
    fs_take(S.ch.z, t, 3);
    P.mark("fs: t_lo t_mid t_hi collected, z");
  }

  // ---- round 4: evaluations at z (plonk.rs:393-399), linearisation r(x) (:401-422)
  const U256 zw = Fr::mul(zc, P.omega);
  auto eval = [&](int np, const uint64_t* const* polys, const uint64_t* lens, const U256* xs, U256* res) -> int {
    int rc2 = fr_eval_run(polys, lens, xs, np, 0, B.partial, (uint64_t*)B.evals.p, s);
    if (rc2) return rc2;
    std::vector<uint64_t> h(4 * np);
    PBF_HIP(hipMemcpyAsync(h.data(), B.evals.p, 4 * np * 8, hipMemcpyDeviceToHost, s));
    PBF_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < np; ++i) res[i] = hm(h.data() + 4 * i);
    return 0;
  };
  PlonkEvals e;
  {
    U256 ev[8];  // t(z) from t as one polynomial of 3m coefficients
    const uint64_t* polys[8] = {C(0), C(1), C(2), C(8), C(9), tq, zx, (const uint64_t*)B.tmp0.p};
    const uint64_t lens[8] = {n + 2, n + 2, n + 2, n, n, 3 * m, n + 3, n};
    const U256 xs[8] = {zc, zc, zc, zc, zc, zc, zw, zc};
    if ((rc = eval(8, polys, lens, xs, ev))) return rc;
    e.a_z = ev[0]; e.b_z = ev[1]; e.c_z = ev[2]; e.s1_z = ev[3]; e.s2_z = ev[4]; e.t_z = ev[5]; e.zw_z = ev[6];
    e.l1_z = ev[7];
  }
  const uint64_t rlen = mode == 0 ? 2 * n + 2 : n + 3;
  uint64_t* rx = W1;  // r(x) coefficients (length rlen, N slot)
  {
    U256 c[7];
    plonk_r_coeffs(S.ch, e, mode, c);
    const uint64_t* in[7] = {C(6), C(3), C(4), C(5), C(7), zx, C(10)};
    const uint64_t lens[7] = {n, n, n, n, n, n + 3, n};
    // mode 1: all seven terms; mode 0: the first six, r_3 below. Only the rlen coefficients r(x)
    // has are written (round 6; the N-long tail of zeros was never read: the evaluation, the r_3
    // sum and the W_z numerator stop at rlen)
    if ((rc = fr_lincomb_run(mode == 1 ? 7 : 6, in, lens, c, u256_zero(), rx, rlen, s))) return rc;
    if (mode == 0) {
      // r_3(x) = z(x) s_sigma_3(x) (beta z_w(z)) K3 (plonk.rs:414-416): the product on the coset
      hipLaunchKernelGGL(k_mul, dim3(blocks_for(NE)), dim3(256), 0, s, (const uint64_t*)CE(3), (const uint64_t*)CE(11),
                         W2, NE);
      PBF_HIP(hipGetLastError());
      if ((rc = P.coset_intt(W2, W0))) return rc;
      const uint64_t* in2[2] = {rx, W0};
      const uint64_t lens2[2] = {rlen, rlen};  // z s_sigma_3 has rlen = 2n + 2 coefficients
      const U256 c2[2] = {one, c[6]};
      if ((rc = fr_lincomb_run(2, in2, lens2, c2, u256_zero(), W2, rlen, s))) return rc;
      PBF_HIP(hipMemcpyAsync(rx, W2, rlen * E, hipMemcpyDeviceToDevice, s));
    }
  }
  {
    const uint64_t* polys[1] = {rx};
    if ((rc = eval(1, polys, &rlen, &zc, &e.r_z))) return rc;
  }
  P.mark("round 4 evals + r(x)");
  if (S.fs) {
    uint64_t t[4];
    write_proof_fields(S.out_f, e);
    fs_round<0, 7>(fs_t, 5, nullptr, S.out_f, t);
    fs_take(S.ch.v, t, 4);
  }

  // ---- round 5: W_z = numerator / (x - z), W_zw = (z(x) - z_w(z)) / (x - z w) (plonk.rs:430-442)
  // by synthetic division on the coefficients
  const uint64_t lnum = rlen > m ? rlen : m;  // numerator coefficients (t parts m, r rlen, a/b/c n+2)
  {
    U256 c[9];
    const U256 c0 = plonk_wz_coeffs(S.ch, e, n, c);  // the constant term folded: vanishes at z
    const uint64_t* in[9] = {tq, tq + 4 * m, tq + 8 * m, rx, C(0), C(1), C(2), C(8), C(9)};
    const uint64_t lens[9] = {m, m, m, rlen, n + 2, n + 2, n + 2, n, n};
    if ((rc = fr_lincomb_run(9, in, lens, c, c0, W2, lnum, s))) return rc;  // what the division reads
  }
  const uint64_t wlen = lnum - 1;  // = max(rlen - 1, m)
  if ((rc = P.synth_div(W2, lnum, zc, u256_zero(), W1, "W_z division left a remainder (plonk.rs:438)"))) return rc;
  uint64_t* W3 = W0;  // W1 still feeds the W_z commitment's MSM
  if ((rc = P.synth_div(zx, n + 3, zw, e.zw_z, W3, "W_zw division left a remainder (plonk.rs:442)"))) return rc;
  if ((rc = P.commit(W1, wlen, 7))) return rc;
  if ((rc = P.commit(W3, n + 2, 8))) return rc;
  if (S.fs) {
    uint64_t t[4];
    U256 u;  // for out_chal only: the prover has no use for it
    if ((rc = P.collect(7, 9, opts))) return rc;
    fs_round<2, 0>(fs_t, 6, opts[7], nullptr, t);
    fs_take(u, t, 5);
  } else if ((rc = P.finish_commits(9, opts))) {
    return rc;
  }
  P.mark("round 5 openings + 2 MSM");
  write_proof_fields(S.out_f, e);
  return 0;
}

// Plonk::prove; comm == null (or world 1): one GPU; else this rank's part of the multi-GPU
// split (pbf.h pbf_plonk_prove_bn254_sharded_dev)
static int prove_impl(pbf_ctx* ctx, const pbf_comm* comm, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                      const uint64_t* d_abc, const uint64_t* chal, const uint64_t* rnd, const uint64_t* k1k2,
                      const uint64_t* d_srs, size_t srs_m, int mode, uint64_t* out_pts, uint64_t* out_f,
                      void* stream, const uint64_t* d_pub = nullptr, size_t npub = 0, const uint8_t* fs_digest = nullptr,
                      uint64_t* out_chal = nullptr) {
  if (!ctx || !d_q || !d_copies || !d_abc || (!chal && !fs_digest) || !rnd || !k1k2 || !d_srs || !out_pts || !out_f)
    return fail(PBF_EINVAL, "null argument");
  if (npub && !d_pub) return fail(PBF_EINVAL, "null pub with npub > 0");
  if (npub > n) return fail(PBF_EINVAL, "more public inputs than gates");
  ProveState S(ctx);
  S.mode = mode;
  S.d_q = d_q; S.d_copies = d_copies; S.d_abc = d_abc;
  S.d_pub = npub ? d_pub : nullptr; S.npub = npub;
  S.out_pts = out_pts; S.out_f = out_f;
  if (fs_digest) {
    S.fs = true;
    S.out_chal = out_chal;
    memcpy(S.fs_h0, fs_digest, 32);
  }
  int rc = prove_setup(S, ctx, comm, n, chal, rnd, k1k2, d_srs, srs_m, stream);
  if (rc) return rc;
  return S.P.G > 1 ? prove_sharded(S) : prove_single(S);
}

extern "C" int pbf_plonk_prove_bn254_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                         const uint64_t* d_abc, const uint64_t* chal, const uint64_t* rnd,
                                         const uint64_t* k1k2, const uint64_t* d_srs, size_t srs_m, int mode,
                                         uint64_t* out_pts, uint64_t* out_f, void* stream) {
  return prove_impl(ctx, nullptr, n, d_q, d_copies, d_abc, chal, rnd, k1k2, d_srs, srs_m, mode, out_pts, out_f, stream);
}

extern "C" int pbf_plonk_prove_bn254_sharded_dev(pbf_ctx* ctx, const pbf_comm* comm, size_t n, const uint64_t* d_q,
                                                 const uint64_t* d_copies, const uint64_t* d_abc, const uint64_t* chal,
                                                 const uint64_t* rnd, const uint64_t* k1k2, const uint64_t* d_srs,
                                                 size_t srs_m, int mode, uint64_t* out_pts, uint64_t* out_f,
                                                 void* stream) {
  if (!comm) return fail(PBF_EINVAL, "null comm");
  return prove_impl(ctx, comm, n, d_q, d_copies, d_abc, chal, rnd, k1k2, d_srs, srs_m, mode, out_pts, out_f, stream);
}

// host-pointer wrapper: uploads q / copies / abc / SRS, proves, returns (pts, fields)
extern "C" int pbf_plonk_prove_bn254(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                     const uint64_t* abc, const uint64_t* chal, const uint64_t* rnd, const uint64_t* k1k2,
                                     const uint64_t* srs, size_t srs_m, int mode, uint64_t* out_pts, uint64_t* out_f) {
  if (!ctx || !q || !copies || !abc || !srs) return fail(PBF_EINVAL, "null argument");
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  DevBuf &dq = ctx->buf("pv.q"), &dc = ctx->buf("pv.copies"), &dabc = ctx->buf("pv.abc"), &dsrs = ctx->buf("pv.srs");
  int rc;
  if ((rc = dq.ensure(5 * n * 32)) || (rc = dc.ensure(3 * n * 16)) || (rc = dabc.ensure(3 * n * 32)) ||
      (rc = dsrs.ensure(srs_m * 64)))
    return rc;
  PBF_HIP(hipMemcpyAsync(dq.p, q, 5 * n * 32, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(dc.p, copies, 3 * n * 16, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(dabc.p, abc, 3 * n * 32, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(dsrs.p, srs, srs_m * 64, hipMemcpyHostToDevice, s));
  rc = pbf_plonk_prove_bn254_dev(ctx, n, (const uint64_t*)dq.p, (const uint64_t*)dc.p, (const uint64_t*)dabc.p, chal,
                                 rnd, k1k2, (const uint64_t*)dsrs.p, srs_m, mode, out_pts, out_f, s);
  if (rc) return rc;
  PBF_HIP(hipStreamSynchronize(s));
  return 0;
}

// The host forms with pub (_pi with npub > 0, _fs with any npub): every argument error, the uploads,
// then the _dev form that chal (_pi) or digest (_fs) selects
static int prove_host_pub(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies, const uint64_t* abc,
                          const uint64_t* pub, size_t npub, const uint64_t* chal, const uint8_t* digest,
                          const uint64_t* rnd, const uint64_t* k1k2, const uint64_t* srs, size_t srs_m, int mode,
                          uint64_t* out_pts, uint64_t* out_f, uint64_t* out_chal) {
  if (!ctx || !q || !copies || !abc || !srs) return fail(PBF_EINVAL, "null argument");
  if (npub && !pub) return fail(PBF_EINVAL, "null pub with npub > 0");
  if (npub > n) return fail(PBF_EINVAL, "more public inputs than gates");
  if (npub && !fr_canonical(pub, npub)) return fail(PBF_EINVAL, "public input not canonical");
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  DevBuf &dq = ctx->buf("pv.q"), &dc = ctx->buf("pv.copies"), &dabc = ctx->buf("pv.abc"), &dsrs = ctx->buf("pv.srs"),
         &dpub = ctx->buf("pv.pub");
  int rc;
  if ((rc = dq.ensure(5 * n * 32)) || (rc = dc.ensure(3 * n * 16)) || (rc = dabc.ensure(3 * n * 32)) ||
      (rc = dsrs.ensure(srs_m * 64)) || (rc = dpub.ensure(npub * 32)))
    return rc;
  PBF_HIP(hipMemcpyAsync(dq.p, q, 5 * n * 32, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(dc.p, copies, 3 * n * 16, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(dabc.p, abc, 3 * n * 32, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(dsrs.p, srs, srs_m * 64, hipMemcpyHostToDevice, s));
  if (npub) PBF_HIP(hipMemcpyAsync(dpub.p, pub, npub * 32, hipMemcpyHostToDevice, s));
  const uint64_t* d_pub = npub ? (const uint64_t*)dpub.p : nullptr;
  if (digest)
    rc = pbf_plonk_prove_bn254_fs_dev(ctx, n, (const uint64_t*)dq.p, (const uint64_t*)dc.p, (const uint64_t*)dabc.p,
                                      d_pub, npub, digest, rnd, k1k2, (const uint64_t*)dsrs.p, srs_m, mode, out_pts,
                                      out_f, out_chal, s);
  else
    rc = pbf_plonk_prove_bn254_pi_dev(ctx, n, (const uint64_t*)dq.p, (const uint64_t*)dc.p, (const uint64_t*)dabc.p,
                                      d_pub, npub, chal, rnd, k1k2, (const uint64_t*)dsrs.p, srs_m, mode, out_pts, out_f,
                                      s);
  if (rc) return rc;
  PBF_HIP(hipStreamSynchronize(s));
  return 0;
}

// Public inputs: pub_i on gate row i < npub (pbf.h). One GPU; npub = 0 is the plain entry.
extern "C" int pbf_plonk_prove_bn254_pi_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                            const uint64_t* d_abc, const uint64_t* d_pub, size_t npub,
                                            const uint64_t* chal, const uint64_t* rnd, const uint64_t* k1k2,
                                            const uint64_t* d_srs, size_t srs_m, int mode, uint64_t* out_pts,
                                            uint64_t* out_f, void* stream) {
  return prove_impl(ctx, nullptr, n, d_q, d_copies, d_abc, chal, rnd, k1k2, d_srs, srs_m, mode, out_pts, out_f, stream,
                    d_pub, npub);
}

extern "C" int pbf_plonk_prove_bn254_pi(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                        const uint64_t* abc, const uint64_t* pub, size_t npub, const uint64_t* chal,
                                        const uint64_t* rnd, const uint64_t* k1k2, const uint64_t* srs, size_t srs_m,
                                        int mode, uint64_t* out_pts, uint64_t* out_f) {
  if (!npub) return pbf_plonk_prove_bn254(ctx, n, q, copies, abc, chal, rnd, k1k2, srs, srs_m, mode, out_pts, out_f);
  return prove_host_pub(ctx, n, q, copies, abc, pub, npub, chal, nullptr, rnd, k1k2, srs, srs_m, mode, out_pts, out_f,
                        nullptr);
}

// Fiat-Shamir (pbf.h): the circuit digest in place of chal; out_chal null, or 6 x 4
extern "C" int pbf_plonk_prove_bn254_fs_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                            const uint64_t* d_abc, const uint64_t* d_pub, size_t npub,
                                            const uint8_t* digest, const uint64_t* rnd, const uint64_t* k1k2,
                                            const uint64_t* d_srs, size_t srs_m, int mode, uint64_t* out_pts,
                                            uint64_t* out_f, uint64_t* out_chal, void* stream) {
  if (!digest) return fail(PBF_EINVAL, "null argument");
  return prove_impl(ctx, nullptr, n, d_q, d_copies, d_abc, nullptr, rnd, k1k2, d_srs, srs_m, mode, out_pts, out_f, stream,
                    d_pub, npub, digest, out_chal);
}

extern "C" int pbf_plonk_prove_bn254_fs(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                        const uint64_t* abc, const uint64_t* pub, size_t npub, const uint8_t* digest,
                                        const uint64_t* rnd, const uint64_t* k1k2, const uint64_t* srs, size_t srs_m,
                                        int mode, uint64_t* out_pts, uint64_t* out_f, uint64_t* out_chal) {
  if (!digest) return fail(PBF_EINVAL, "null argument");
  return prove_host_pub(ctx, n, q, copies, abc, pub, npub, nullptr, digest, rnd, k1k2, srs, srs_m, mode, out_pts, out_f,
                        out_chal);
}

// ---------------------------------------------------------------- synthetic config-5 inputs
namespace pbf {
__device__ __forceinline__ uint64_t sm64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// uniform canonical Fr from (seed, stream index): 4 splitmix64 words, top limb masked to
// 254 bits, re-mixed until < r
__device__ U256 rand_fr(uint64_t seed, uint64_t i) {
  const uint64_t G = 0x9E3779B97F4A7C15ull;
  uint64_t ctr = seed + (i + 1) * G * 4;
  for (;;) {
    uint64_t l[4];
    for (int k = 0; k < 4; ++k) l[k] = sm64(ctr += G);
    l[3] &= (1ull << 62) - 1;
    const U256 v = u256_from_u64(l);
    if (!Fr::geq_p(v)) return v;
  }
}
// BASELINE config 5 circuit: every gate a*b = c (q_m = 1, q_o = -1, q_l = q_r = q_c = 0),
// a, b uniform; every 4th gate's c feeds the next gate's a (a real copy constraint)
__global__ void k_synth_circuit(uint64_t n, uint64_t seed, uint64_t* q, uint64_t* copies, uint64_t* abc) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  U256 mone;
  for (int k = 0; k < 8; ++k) mone.w[k] = Bn254FrParams::P[k];
  mone.w[0] -= 1;  // r - 1
  const U256 z = u256_zero();
  U256 one = z;
  one.w[0] = 1;
  u256_to_u64(z, q + 4 * i);
  u256_to_u64(z, q + 4 * (n + i));
  u256_to_u64(mone, q + 4 * (2 * n + i));
  u256_to_u64(one, q + 4 * (3 * n + i));
  u256_to_u64(z, q + 4 * (4 * n + i));
  U256 b = rand_fr(seed ^ 0xB0B0ull, i);
  U256 a;
  if (i % 4 == 1) {  // a_i = c_{i-1} = a_{i-1} b_{i-1}
    a = Fr::from_mont(Fr::mul(Fr::to_mont(rand_fr(seed, i - 1)), Fr::to_mont(rand_fr(seed ^ 0xB0B0ull, i - 1))));
  } else {
    a = rand_fr(seed, i);
  }
  const U256 c = Fr::from_mont(Fr::mul(Fr::to_mont(a), Fr::to_mont(b)));
  u256_to_u64(a, abc + 4 * i);
  u256_to_u64(b, abc + 4 * (n + i));
  u256_to_u64(c, abc + 4 * (2 * n + i));
  // copies (kind, 1-based index): identity, with a_{i} <-> c_{i-1} swapped for i % 4 == 1
  uint64_t* ca = copies + 2 * i;
  uint64_t* cb = copies + 2 * (n + i);
  uint64_t* cc = copies + 2 * (2 * n + i);
  ca[0] = 0; ca[1] = i + 1;
  cb[0] = 1; cb[1] = i + 1;
  cc[0] = 2; cc[1] = i + 1;
  if (i % 4 == 1) { ca[0] = 2; ca[1] = i; }            // a_i is a copy of c_{i-1}
  if (i % 4 == 0 && i + 1 < n) { cc[0] = 0; cc[1] = i + 2; }  // c_i is a copy of a_{i+1}
}
}  // namespace pbf

extern "C" int pbf_plonk_synth_circuit_bn254_dev(pbf_ctx* ctx, size_t n, uint64_t seed, uint64_t* d_q,
                                                 uint64_t* d_copies, uint64_t* d_abc, void* stream) {
  if (!ctx || !d_q || !d_copies || !d_abc) return fail(PBF_EINVAL, "null argument");
  hipLaunchKernelGGL(k_synth_circuit, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, (uint64_t)n, seed, d_q,
                     d_copies, d_abc);
  PBF_HIP(hipGetLastError());
  return 0;
}

// SRS::create on the device: d_out = [G, sG, ..., s^n G] (n+1 affine points)
extern "C" int pbf_srs_create_bn254_dev(pbf_ctx* ctx, const uint64_t* s, size_t n, uint64_t* d_out, void* stream) {
  if (!ctx || !s || !d_out) return fail(PBF_EINVAL, "null argument");
  if (Fr::geq_p(u256_from_u64(s))) return fail(PBF_EINVAL, "s not canonical");
  hipStream_t st = (hipStream_t)stream;
  DevBuf& pw = ctx->buf("srs.pows");
  int rc = pw.ensure((n + 1) * 32);
  if (rc) return rc;
  hipLaunchKernelGGL(k_powers29, dim3(blocks_for((n + 1 + PV_CHUNK - 1) / PV_CHUNK)), dim3(256), 0, st, (uint64_t*)pw.p,
                     (uint64_t)(n + 1), powers_tab29(hm(s), fr_one_m()));
  PBF_HIP(hipGetLastError());
  return pbf_g1_bn254_mul_base_dev(ctx, (const uint64_t*)pw.p, d_out, n + 1, stream);
}
