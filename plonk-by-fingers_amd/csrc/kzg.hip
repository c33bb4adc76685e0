// KZG10 polynomial commitments over BN254 on gfx950 (include/pbf.h "KZG commitments"): commit,
// batched opening at one point, batched verification, and Poly::eval over Fr.
//
//   commit   SRS::eval_at_s (plonk.rs:51-58): one fixed-base MSM per polynomial against the
//            context's window table of the SRS (msm.hpp)
//   open     y_b = p_b(z) and W = commit((sum_b w_b (p_b - y_b)) / (x - z)) (plonk.rs:429-446), on
//            the prover's own kernels (prover.hpp): the chunked Horner evaluation, a linear
//            combination, the blocked synthetic division k_hs1..3. The quotient does not depend
//            on the subtracted constants (they only move the remainder, which is dropped), so
//            the division runs on sum_b w_b p_b as it stands and has no failing case. A fused
//            single-sweep kernel was built and measured against this sequence and not kept
//            (profiles/kzg/open_ab.txt).
//   open from evaluations   the same (y, W) from the polynomials' values on H = <omega> against the
//            Lagrange-basis SRS (g1_ntt.hip): denominators omega^i - z, the prover's batch
//            inversion, a barycentric dot product per polynomial, the pointwise quotient, one
//            MSM; z = omega^k is handled on the device and is no failing case either
//   open all   every opening on H at once by FK20: one Fr NTT of size 2n, 2n pointwise products
//            against the setup xext, the inverse G1 NTT of size 2n and the forward one of size n,
//            the three G1 steps in Xyzz throughout (g1_mul.hip, g1_ntt.hip)
//   cells    one proof per coset of l points (the cells of data-availability sampling): FK20 over
//            cosets, l slabs of size 2k = 2n/l through the same products, a sum of the l products
//            of every frequency, transforms of sizes 2k and k; the batched cell verifier with its
//            interpolation sweep
//   verify   e(sum rho_i W_i, [s]G2) e(-sum rho_i (C_i - y_i G + z_i W_i), G2) == 1: one MSM over
//            count points, one over 2 count + 1, one pairing check
//
// Everything is conversion-free where it touches coefficients: canonical values times
// Montgomery-form multipliers (z, its powers, the weights) are canonical products.
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../include/pbf.h"
#include "g1_win.hpp"

using namespace pbf;

namespace {

// ---------------------------------------------------------------- the opening's sweeps
// y (device, batch x 4) and the quotient's len - 1 coefficients in q. Evaluations: 12 polynomials
// per launch; the weighted sum: 10 inputs per launch, later launches taking the sum so far as one
// of them; then one division.
int open_sweeps(pbf_ctx* ctx, const uint64_t* d_polys, uint64_t len, uint64_t pitch, uint64_t batch, const U256& z,
                const std::vector<U256>& w, uint64_t* q, uint64_t* d_y, hipStream_t s) {
  int rc;
  for (uint64_t b0 = 0; b0 < batch; b0 += 12) {
    const int g = (int)std::min<uint64_t>(12, batch - b0);
    const uint64_t* polys[12];
    uint64_t lens[12];
    U256 xs[12];
    for (int b = 0; b < g; ++b) {
      polys[b] = d_polys + 4 * (b0 + b) * pitch;
      lens[b] = len;
      xs[b] = z;
    }
    if ((rc = fr_eval_run(polys, lens, xs, g, 0, ctx->partial, d_y + 4 * b0, s))) return rc;
  }
  if (len < 2) return 0;
  DevBuf &bc = ctx->buf("kzg.comb"), &br = ctx->buf("kzg.rem");
  if ((rc = bc.ensure(len * 32)) || (rc = br.ensure(32))) return rc;
  uint64_t* comb = (uint64_t*)bc.p;
  for (uint64_t b0 = 0; b0 < batch;) {
    const uint64_t* in[10];
    const uint64_t lens[10] = {len, len, len, len, len, len, len, len, len, len};
    U256 c[10];
    int k = 0;
    if (b0) {  // the sum so far
      in[k] = comb;
      c[k++] = fr_one_m();
    }
    while (k < 10 && b0 < batch) {
      in[k] = d_polys + 4 * b0 * pitch;
      c[k++] = w[b0++];
    }
    if ((rc = fr_lincomb_run(k, in, lens, c, u256_zero(), comb, len, s))) return rc;
  }
  HsArgs ha;
  ha.p = comb;
  ha.L = len;
  ha.y = u256_zero();
  hs_set_point(ha, z);
  return hs_div_run(ctx, ha, q, (uint64_t*)br.p, s);
}

// ---------------------------------------------------------------- verify
// One lane per entry i: pts = [C_0.. | W_0.. | (G, by the host)], sc = [rho_i | rho_i z_i | .],
// part[block] = sum of the block's rho_i y_i; *flag set by a point that is not canonical or not on
// the curve.
__global__ void __launch_bounds__(256) k_kzg_vprep(const uint64_t* commits, const uint64_t* w, const uint64_t* z,
                                                   const uint64_t* y, const uint64_t* rho, uint32_t count,
                                                   uint64_t* pts, uint64_t* sc, uint64_t* part, int* flag) {
  __shared__ U256 sh[256];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  U256 ry = u256_zero();
  if (i < count) {
    const uint64_t *c = commits + 8 * (uint64_t)i, *wi = w + 8 * (uint64_t)i;
    if (g1_bad(c) || g1_bad(wi)) atomicOr(flag, 1);
    uint64_t *pc = pts + 8 * (uint64_t)i, *pw = pts + 8 * ((uint64_t)count + i);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      pc[k] = c[k];
      pw[k] = wi[k];
    }
    const U256 r = u256_from_u64(rho + 4 * (uint64_t)i), rm = Fr::to_mont(r);
    u256_to_u64(r, sc + 4 * (uint64_t)i);
    u256_to_u64(Fr::mul(rm, u256_from_u64(z + 4 * (uint64_t)i)), sc + 4 * ((uint64_t)count + i));
    ry = Fr::mul(rm, u256_from_u64(y + 4 * (uint64_t)i));
  }
  const uint32_t t = threadIdx.x;
  sh[t] = ry;
  __syncthreads();
  for (uint32_t s = 128; s; s >>= 1) {
    if (t < s) sh[t] = Fr::add(sh[t], sh[t + s]);
    __syncthreads();
  }
  if (t == 0) u256_to_u64(sh[0], part + 4 * (uint64_t)blockIdx.x);
}
// sc[2 count] = -(sum of the nparts partial sums): the scalar of G; one workgroup
__global__ void __launch_bounds__(256) k_kzg_vsum(const uint64_t* part, uint32_t nparts, uint64_t* out) {
  __shared__ U256 sh[256];
  const uint32_t t = threadIdx.x;
  U256 acc = u256_zero();
  for (uint32_t i = t; i < nparts; i += 256) acc = Fr::add(acc, u256_from_u64(part + 4 * (uint64_t)i));
  sh[t] = acc;
  __syncthreads();
  for (uint32_t s = 128; s; s >>= 1) {
    if (t < s) sh[t] = Fr::add(sh[t], sh[t + s]);
    __syncthreads();
  }
  if (t == 0) u256_to_u64(Fr::sub(u256_zero(), sh[0]), out);
}

// every argument error of commit / open, before anything is enqueued
int poly_args(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* polys, size_t len, size_t pitch,
              size_t batch, size_t need) {
  if (!ctx || !srs || !polys) return fail(PBF_EINVAL, "null argument");
  if (len == 0) return fail(PBF_EINVAL, "len must be at least 1");
  if (batch == 0 || batch > ((size_t)1 << 16)) return fail(PBF_EINVAL, "batch must be in 1 .. 2^16");
  if (pitch < len) return fail(PBF_EINVAL, "pitch shorter than len");
  if (srs_m < need) return fail(PBF_EINVAL, "SRS too short");
  return 0;
}
int open_args(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* polys, size_t len, size_t pitch,
              size_t batch, const uint64_t* z, const uint64_t* weights, const uint64_t* out_y, const uint64_t* out_w) {
  if (!z || !weights || !out_y || !out_w) return fail(PBF_EINVAL, "null argument");
  int rc = poly_args(ctx, srs, srs_m, polys, len, pitch, batch, len ? len - 1 : 0);
  if (rc) return rc;
  if (!fr_canonical(z)) return fail(PBF_EINVAL, "z must be canonical");
  if (!fr_canonical(weights, batch)) return fail(PBF_EINVAL, "weights must be canonical");
  return 0;
}

// the polynomials of a host-pointer call on the device, compact (pitch = len)
int upload_polys(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* polys, size_t len, size_t pitch,
                 size_t batch, hipStream_t s) {
  DevBuf &ds = ctx->buf("kzg.srs"), &dp = ctx->buf("kzg.polys");
  int rc;
  if ((rc = ds.ensure(std::max<size_t>(srs_m, 1) * 64)) || (rc = dp.ensure(batch * len * 32))) return rc;
  if (srs_m) PBF_HIP(hipMemcpyAsync(ds.p, srs, srs_m * 64, hipMemcpyHostToDevice, s));
  if (pitch == len) {
    PBF_HIP(hipMemcpyAsync(dp.p, polys, batch * len * 32, hipMemcpyHostToDevice, s));
  } else {
    PBF_HIP(hipMemcpy2DAsync(dp.p, len * 32, polys, pitch * 32, len * 32, batch, hipMemcpyHostToDevice, s));
  }
  return 0;
}

// ---------------------------------------------------------------- opening from evaluations
// The polynomials as their values on H = <omega> (tw: fr_domain_table). Denominators, one batch
// inversion, a barycentric dot product per polynomial, the pointwise quotient. All canonical
// values times Montgomery multipliers, as above.
constexpr int EVD_G = 8;  // polynomials per dot-product launch: omega^i u_i is formed once for them

// the block's sum of v over its 256 lanes, valid on lane 0 (sh: 256 values)
__device__ __forceinline__ U256 block_sum(U256* sh, const U256& v) {
  const uint32_t t = threadIdx.x;
  __syncthreads();  // the previous sum's readers are done with sh
  sh[t] = v;
  __syncthreads();
  for (uint32_t s = 128; s; s >>= 1) {
    if (t < s) sh[t] = Fr::add(sh[t], sh[t + s]);
    __syncthreads();
  }
  return sh[0];
}

// den[i] = omega^i - z (canonical); where that is zero (z = omega^i) den[i] = 1 and *kidx = i, so
// that the inversion never sees the zero
__global__ void __launch_bounds__(256) k_ev_den(const uint64_t* tw, uint64_t n, U256 z, uint64_t* den, uint64_t* kidx) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  U256 d = Fr::sub(fr_domain_at(tw, n, i), z);
  if (Fr::is_zero(d)) {
    d = Fr::one_plain();
    *kidx = i;
  }
  u256_to_u64(d, den + 4 * i);
}
// part[(b0 + b) nblk + block] = the block's sum of p_b[i] omega^i u_i for the g <= EVD_G
// polynomials from b0 on (u: Montgomery form, as fr_inv_batch_run leaves it)
__global__ void __launch_bounds__(256) k_ev_dot(const uint64_t* evals, uint64_t pitch, uint64_t b0, uint32_t g, uint64_t n,
                                                const uint64_t* tw, const uint64_t* u, uint64_t* part) {
  __shared__ U256 sh[256];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  U256 f = u256_zero();
  if (i < n) f = Fr::mul(Fr::to_mont(fr_domain_at(tw, n, i)), u256_from_u64(u + 4 * i));
  for (uint32_t b = 0; b < g; ++b) {
    U256 v = u256_zero();
    if (i < n) v = Fr::mul(f, u256_from_u64(evals + 4 * ((b0 + b) * pitch + i)));
    const U256 sum = block_sum(sh, v);
    if (threadIdx.x == 0) u256_to_u64(sum, part + 4 * ((b0 + b) * gridDim.x + blockIdx.x));
  }
}
// y[b] = factor * (the sum of polynomial b's nblk partial sums); one workgroup per polynomial
__global__ void __launch_bounds__(256) k_ev_ysum(const uint64_t* part, uint64_t nblk, U256 factor, uint64_t* y) {
  __shared__ U256 sh[256];
  const uint64_t b = blockIdx.x;
  U256 acc = u256_zero();
  for (uint64_t i = threadIdx.x; i < nblk; i += 256) acc = Fr::add(acc, u256_from_u64(part + 4 * (b * nblk + i)));
  const U256 sum = block_sum(sh, acc);
  if (threadIdx.x == 0) u256_to_u64(Fr::mul(factor, sum), y + 4 * b);
}
// z = omega^k: y[b] = p_b[k]
__global__ void __launch_bounds__(256) k_ev_ypick(const uint64_t* evals, uint64_t pitch, uint64_t batch,
                                                  const uint64_t* kidx, uint64_t* y) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  for (int q = 0; q < 4; ++q) y[4 * b + q] = evals[4 * (b * pitch + *kidx) + q];
}
// *yc = sum_b w_b y_b (w: Montgomery form); one workgroup
__global__ void __launch_bounds__(256) k_ev_yc(const uint64_t* y, const uint64_t* w, uint64_t batch, uint64_t* yc) {
  __shared__ U256 sh[256];
  U256 acc = u256_zero();
  for (uint64_t b = threadIdx.x; b < batch; b += 256)
    acc = Fr::add(acc, Fr::mul(u256_from_u64(w + 4 * b), u256_from_u64(y + 4 * b)));
  const U256 sum = block_sum(sh, acc);
  if (threadIdx.x == 0) u256_to_u64(sum, yc);
}
// q[i] = (c[i] - *yc) u[i]; with kidx (z = omega^k): q[k] = 0 for now and part[block] = the
// block's sum of omega^i q[i]
__global__ void __launch_bounds__(256) k_ev_quot(const uint64_t* c, const uint64_t* yc, const uint64_t* u,
                                                 const uint64_t* tw, uint64_t n, const uint64_t* kidx, uint64_t* q,
                                                 uint64_t* part) {
  __shared__ U256 sh[256];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  U256 v = u256_zero();
  if (i < n) {
    if (!kidx || i != *kidx)
      v = Fr::mul(u256_from_u64(u + 4 * i), Fr::sub(u256_from_u64(c + 4 * i), u256_from_u64(yc)));
    u256_to_u64(v, q + 4 * i);
    if (kidx) v = Fr::mul(Fr::to_mont(fr_domain_at(tw, n, i)), v);
  }
  if (!kidx) return;
  const U256 sum = block_sum(sh, v);
  if (threadIdx.x == 0) u256_to_u64(sum, part + 4 * (uint64_t)blockIdx.x);
}
// q[k] = -omega^-k (the sum of the nblk partial sums); one workgroup
__global__ void __launch_bounds__(256) k_ev_qk(const uint64_t* part, uint64_t nblk, const uint64_t* tw, uint64_t n,
                                               const uint64_t* kidx, uint64_t* q) {
  __shared__ U256 sh[256];
  U256 acc = u256_zero();
  for (uint64_t i = threadIdx.x; i < nblk; i += 256) acc = Fr::add(acc, u256_from_u64(part + 4 * i));
  const U256 sum = block_sum(sh, acc);
  if (threadIdx.x) return;
  const uint64_t k = *kidx;
  const U256 wk_inv = Fr::to_mont(fr_domain_at(tw, n, (n - k) & (n - 1)));
  u256_to_u64(Fr::sub(u256_zero(), Fr::mul(wk_inv, sum)), q + 4 * k);
}

// y (device, batch x 4) and the quotient's n evaluations in q, for n >= 2; w: the weights in
// Montgomery form
int open_evals_sweeps(pbf_ctx* ctx, const uint64_t* tw, uint64_t n, const uint64_t* d_evals,
                      uint64_t pitch, uint64_t batch, const U256& zm, const std::vector<U256>& w, uint64_t* q,
                      uint64_t* d_y, hipStream_t s) {
  const uint64_t nblk = (n + 255) / 256;
  const U256 zn = fr_pow(zm, n);
  const bool in_h = heq1(zn);
  DevBuf &bu = ctx->buf("kzg.ev.u"), &bc = ctx->buf("kzg.comb"), &bp = ctx->buf("kzg.ev.part"),
         &bw = ctx->buf("kzg.ev.w"), &bs = ctx->buf("kzg.ev.small");
  int rc;
  if ((rc = bu.ensure(n * 32)) || (rc = bc.ensure(n * 32)) || (rc = bp.ensure(std::max(batch, (uint64_t)1) * nblk * 32)) ||
      (rc = bw.ensure(batch * 32)) || (rc = bs.ensure(64)))
    return rc;
  uint64_t *u = (uint64_t*)bu.p, *comb = (uint64_t*)bc.p, *part = (uint64_t*)bp.p, *d_w = (uint64_t*)bw.p;
  uint64_t *yc = (uint64_t*)bs.p, *kidx = yc + 4;
  int* bad = (int*)(yc + 5);  // never set: no denominator is zero
  PBF_HIP(hipMemcpyAsync(d_w, w.data(), batch * 32, hipMemcpyHostToDevice, s));  // w: the caller's, kept past its sync
  PBF_HIP(hipMemsetAsync(yc, 0, 64, s));
  const dim3 grid((uint32_t)nblk), blk(256);
  hipLaunchKernelGGL(k_ev_den, grid, blk, 0, s, tw, n, Fr::from_mont(zm), u, kidx);
  if ((rc = fr_inv_batch_run(ctx, u, u, n, bad, s))) return rc;
  if (in_h) {
    hipLaunchKernelGGL(k_ev_ypick, dim3((uint32_t)((batch + 255) / 256)), blk, 0, s, d_evals, pitch, batch,
                       (const uint64_t*)kidx, d_y);
  } else {
    for (uint64_t b0 = 0; b0 < batch; b0 += EVD_G)
      hipLaunchKernelGGL(k_ev_dot, grid, blk, 0, s, d_evals, pitch, b0, (uint32_t)std::min<uint64_t>(EVD_G, batch - b0),
                         n, tw, (const uint64_t*)u, part);
    // y = -(z^n - 1) n^-1 sum
    const U256 factor = Fr::mul(Fr::sub(fr_one_m(), zn), fr_inv(hm64(n)));
    hipLaunchKernelGGL(k_ev_ysum, dim3((uint32_t)batch), blk, 0, s, (const uint64_t*)part, nblk, factor, d_y);
  }
  hipLaunchKernelGGL(k_ev_yc, dim3(1), blk, 0, s, (const uint64_t*)d_y, (const uint64_t*)d_w, batch, yc);
  PBF_HIP(hipGetLastError());
  for (uint64_t b0 = 0; b0 < batch;) {  // c = sum_b w_b p_b, as open_sweeps
    const uint64_t* in[10];
    const uint64_t lens[10] = {n, n, n, n, n, n, n, n, n, n};
    U256 c[10];
    int k = 0;
    if (b0) {
      in[k] = comb;
      c[k++] = fr_one_m();
    }
    while (k < 10 && b0 < batch) {
      in[k] = d_evals + 4 * b0 * pitch;
      c[k++] = w[b0++];
    }
    if ((rc = fr_lincomb_run(k, in, lens, c, u256_zero(), comb, n, s))) return rc;
  }
  hipLaunchKernelGGL(k_ev_quot, grid, blk, 0, s, (const uint64_t*)comb, (const uint64_t*)yc, (const uint64_t*)u, tw, n,
                     in_h ? (const uint64_t*)kidx : nullptr, q, part);
  if (in_h)
    hipLaunchKernelGGL(k_ev_qk, dim3(1), blk, 0, s, (const uint64_t*)part, nblk, tw, n, (const uint64_t*)kidx, q);
  PBF_HIP(hipGetLastError());
  return 0;
}

int open_evals_args(pbf_ctx* ctx, const uint64_t* lsrs, size_t n, const uint64_t* omega, const uint64_t* evals,
                    size_t pitch, size_t batch, const uint64_t* z, const uint64_t* weights, const uint64_t* out_y,
                    const uint64_t* out_w, U256* wm) {
  if (!omega) return fail(PBF_EINVAL, "null argument");
  int rc = open_args(ctx, lsrs, n, evals, n, pitch, batch, z, weights, out_y, out_w);
  if (rc) return rc;
  return fr_domain_check(omega, n, wm);
}

// ---------------------------------------------------------------- every opening at once (FK20)
// W_(omega^i) = sum_m omega^(im) h_m with h_m = sum_k p_(m+1+k) srs[k]: h is the upper half of
// the convolution of a_t = srs[n - 2 - t] with p, taken in a cyclic convolution of size 2n that
// does not wrap. xext, the size-2n G1 NTT of a, is the setup; a call is one
// size-2n Fr NTT, 2n pointwise products, the size-2n inverse G1 NTT and the size-n forward one,
// the last three without leaving Xyzz (g1_mul.hip, g1_ntt.hip).
constexpr size_t FK20_MAX_N = (size_t)1 << 27;  // 2n stays within the 2-adicity of Fr

// a_t = srs[n - 2 - t] for t <= n - 2 and the identity (0, 0) for n - 1 <= t < 2n
__global__ void __launch_bounds__(256) k_fk20_a(const uint64_t* srs, uint64_t n, uint64_t* a) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * n) return;
#pragma unroll
  for (int k = 0; k < 8; ++k) a[8 * t + k] = t + 2 <= n ? srs[8 * (n - 2 - t) + k] : 0;
}

// n a power of two in 1 .. 2^27 and omega2 canonical of order exactly 2n; *w2m = omega2 (Montgomery)
int fk20_domain(size_t n, const uint64_t* omega2, U256* w2m) {
  if (n == 0 || (n & (n - 1)) || n > FK20_MAX_N) return fail(PBF_EINVAL, "n must be a power of two in 1 .. 2^27");
  return fr_domain_check(omega2, 2 * n, w2m);
}
int fk20_setup_args(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* omega2, size_t n,
                    const uint64_t* xext, U256* w2m) {
  if (!ctx || !srs || !omega2 || !xext) return fail(PBF_EINVAL, "null argument");
  int rc = fk20_domain(n, omega2, w2m);
  if (rc) return rc;
  if (srs_m + 1 < n) return fail(PBF_EINVAL, "SRS too short");
  return 0;
}
int fk20_open_args(pbf_ctx* ctx, const uint64_t* xext, size_t n, const uint64_t* omega2, const uint64_t* polys,
                   size_t len, size_t pitch, size_t batch, const uint64_t* weights, const uint64_t* out_w, U256* w2m) {
  if (!omega2 || !weights || !out_w) return fail(PBF_EINVAL, "null argument");
  int rc = poly_args(ctx, xext, 0, polys, len, pitch, batch, 0);
  if (rc) return rc;
  if ((rc = fk20_domain(n, omega2, w2m))) return rc;
  if (len > n) return fail(PBF_EINVAL, "len exceeds n");
  if (!fr_canonical(weights, batch)) return fail(PBF_EINVAL, "weights must be canonical");
  return 0;
}

// comb = scale sum_b weights_b p_b on len coefficients (weights: the caller's, canonical; scale:
// Montgomery form): 10 inputs per launch, later launches taking the sum so far as one of them
int fk20_comb(const uint64_t* d_polys, uint64_t len, uint64_t pitch, uint64_t batch, const uint64_t* weights,
              const U256& scale, uint64_t* comb, hipStream_t s) {
  int rc;
  for (uint64_t b0 = 0; b0 < batch;) {
    const uint64_t* in[10];
    const uint64_t lens[10] = {len, len, len, len, len, len, len, len, len, len};
    U256 c[10];
    int k = 0;
    if (b0) {  // the sum so far
      in[k] = comb;
      c[k++] = fr_one_m();
    }
    while (k < 10 && b0 < batch) {
      in[k] = d_polys + 4 * b0 * pitch;
      c[k++] = Fr::mul(hm(weights + 4 * b0++), scale);
    }
    if ((rc = fr_lincomb_run(k, in, lens, c, u256_zero(), comb, len, s))) return rc;
  }
  return 0;
}

// ---------------------------------------------------------------- cell proofs (FK20 over cosets)
// Cell i < k = n / l is the coset {omega^(i + k t) : t < l}, on which x^l = c_i = omega^(i l);
// W_i = [q_i(s)]G for p = q_i (x^l - c_i) + I_i. W = sum_m c_i^m h_m is the forward G1 NTT of size
// k, root omega^l, of h_m = sum_{r<l} (a_r * b_r)_(k-1+m): l convolutions of the shape above at
// size 2k, a_r[t] = srs[r + l (k-2-t)], b_r[u] = p_(r + l u). xext holds the l
// transforms of the a_r slab after slab; a call multiplies all 2n points as one vector, sums the
// l products of every frequency and runs the two transforms at sizes 2k and k.
constexpr size_t CELLS_MAX_COUNT = (size_t)1 << 20, CELLS_MAX_VALUES = (size_t)1 << 22;
constexpr int CV_CH = 32;  // entries per lane of the verifier's sweep

// a[r 2k + t] = srs[r + l (k-2-t)] for t <= k-2 and the identity (0, 0) for k-1 <= t < 2k, r < l
__global__ void __launch_bounds__(256) k_cells_a(const uint64_t* srs, uint64_t k, uint32_t log_l, uint64_t* a) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= (2 * k) << log_l) return;
  const uint64_t r = j / (2 * k), t = j % (2 * k);
#pragma unroll
  for (int q = 0; q < 8; ++q) a[8 * j + q] = t + 2 <= k ? srs[8 * (r + ((k - 2 - t) << log_l)) + q] : 0;
}

// b[r k + u] = c_(r + l u), zero from len on: the l inputs of the batched Fr NTT of size 2k
__global__ void __launch_bounds__(256) k_cells_gather(const uint64_t* c, uint64_t len, uint64_t k, uint32_t log_l,
                                                      uint64_t* b) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= k << log_l) return;
  const uint64_t src = j / k + ((j % k) << log_l);
#pragma unroll
  for (int q = 0; q < 4; ++q) b[4 * j + q] = src < len ? c[4 * src + q] : 0;
}

// out[(b k + i) l + t] = y[b n + i + k t]: the values of a transform of size n = k l, cell-major
__global__ void __launch_bounds__(256) k_cells_ystore(const uint64_t* y, uint64_t total, uint64_t k, uint32_t log_l,
                                                      uint64_t* out) {
  const uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  const uint64_t n = k << log_l, rem = o & (n - 1);
  const uint64_t src = (o - rem) + (rem >> log_l) + k * (rem & (((uint64_t)1 << log_l) - 1));
#pragma unroll
  for (int q = 0; q < 4; ++q) out[4 * o + q] = y[4 * src + q];
}

// chat_i = sum_{r<l} prod_(r 2k + i) for i < 2k, one lane per frequency. k_g1_mul_x left product
// j of the 2n at x[bitrev_2n((2n - j) mod 2n)]; the sum goes to out[bitrev_2k((2k - i) mod 2k)],
// where the stages of size 2k read the input of an inverse transform. add2 is the complete
// addition: equal, opposite and identity operands are ordinary inputs.
__global__ void __launch_bounds__(GN_T) __attribute__((amdgpu_waves_per_eu(2))) k_cells_sum(const Xyzz* x, Xyzz* out, uint32_t log_k2,
                                                   uint32_t log_l) {
  const uint64_t i = (uint64_t)blockIdx.x * GN_T + threadIdx.x;
  const uint64_t k2 = (uint64_t)1 << log_k2, n2 = k2 << log_l;
  if (i >= k2) return;
  const uint32_t log_n2 = log_k2 + log_l;
  Xyzz acc = ld_pt(x + (__brevll((n2 - i) & (n2 - 1)) >> (64 - log_n2)));
#pragma unroll 1
  for (uint64_t r = 1; r < ((uint64_t)1 << log_l); ++r) {
    const uint64_t j = (r << log_k2) + i;
    acc = G1::add2(acc, ld_pt(x + (__brevll(n2 - j) >> (64 - log_n2))));
  }
  st_pt(out + (__brevll((k2 - i) & (k2 - 1)) >> (64 - log_k2)), acc);
}

// omega^e for e < n from the domain table of (omega, n), Montgomery form; n = 1 has no table
__device__ __forceinline__ U256 cells_pow(const uint64_t* tw, uint64_t n, uint64_t e) {
  return n > 1 ? Fr::to_mont(fr_domain_at(tw, n, e)) : Fr::to_mont(Fr::one_plain());
}

// The verifier's per-entry pass, after k_kzg_vprep: pts = [C_0.. | W_0.. | srs[0 .. l), by the
// host], sc = [rho_j | rho_j c_(idx_j) | .]; *flag set by a point (an SRS point included) that is
// not canonical or not on the curve.
__global__ void __launch_bounds__(256) k_cells_vprep(const uint64_t* commits, const uint64_t* w, const uint64_t* rho,
                                                     const uint64_t* idx, uint32_t count, const uint64_t* tw, uint64_t n,
                                                     uint32_t log_l, uint64_t* pts, uint64_t* sc, int* flag) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < (1u << log_l) && g1_bad(pts + 8 * (2 * (uint64_t)count + i))) atomicOr(flag, 1);
  if (i >= count) return;
  const uint64_t *c = commits + 8 * (uint64_t)i, *wi = w + 8 * (uint64_t)i;
  if (g1_bad(c) || g1_bad(wi)) atomicOr(flag, 1);
  uint64_t *pc = pts + 8 * (uint64_t)i, *pw = pts + 8 * ((uint64_t)count + i);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    pc[q] = c[q];
    pw[q] = wi[q];
  }
  const U256 r = u256_from_u64(rho + 4 * (uint64_t)i);
  u256_to_u64(r, sc + 4 * (uint64_t)i);
  u256_to_u64(Fr::mul(cells_pow(tw, n, idx[i] << log_l), r), sc + 4 * ((uint64_t)count + i));
}
// The interpolation sweep: v[j l + t] = INTT_l(y_j)[t], so I_(j,t) = omega^(-idx_j t) v[j l + t].
// Lane (chunk, t): part[chunk l + t] = the sum over the chunk's CV_CH entries j of
// rho_j omega^(-idx_j t) v[j l + t].
__global__ void __launch_bounds__(256) k_cells_vsweep(const uint64_t* v, const uint64_t* rho, const uint64_t* idx,
                                                      uint32_t count, const uint64_t* tw, uint64_t n, uint32_t log_l,
                                                      uint32_t nchunks, uint64_t* part) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (uint64_t)nchunks << log_l) return;
  const uint64_t t = g & (((uint64_t)1 << log_l) - 1), j0 = (g >> log_l) * CV_CH;
  U256 acc = u256_zero();
  for (uint64_t j = j0; j < j0 + CV_CH && j < count; ++j) {
    const uint64_t e = (idx[j] * t) & (n - 1);
    const U256 f = Fr::mul(Fr::to_mont(u256_from_u64(rho + 4 * j)), cells_pow(tw, n, (n - e) & (n - 1)));
    acc = Fr::add(acc, Fr::mul(f, u256_from_u64(v + 4 * ((j << log_l) + t))));
  }
  u256_to_u64(acc, part + 4 * g);
}
// sc_srs[t] = -(the sum over the chunks of part[chunk l + t]): the scalar of srs[t]; one
// workgroup per t
__global__ void __launch_bounds__(256) k_cells_vsum(const uint64_t* part, uint32_t nchunks, uint32_t log_l, uint64_t* sc_srs) {
  __shared__ U256 sh[256];
  const uint64_t t = blockIdx.x;
  U256 acc = u256_zero();
  for (uint64_t c = threadIdx.x; c < nchunks; c += 256) acc = Fr::add(acc, u256_from_u64(part + 4 * ((c << log_l) + t)));
  const U256 sum = block_sum(sh, acc);
  if (threadIdx.x == 0) u256_to_u64(Fr::sub(u256_zero(), sum), sc_srs + 4 * t);
}

// l a power of two in 1 .. n; *log_l
int cells_l(size_t n, size_t l, uint32_t* log_l) {
  if (l == 0 || (l & (l - 1)) || l > n) return fail(PBF_EINVAL, "l must be a power of two in 1 .. n");
  *log_l = 0;
  while (((size_t)1 << *log_l) < l) ++*log_l;
  return 0;
}
int cells_setup_args(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* omega2, size_t n, size_t l,
                     const uint64_t* xext, U256* w2m, uint32_t* log_l) {
  if (!ctx || !srs || !omega2 || !xext) return fail(PBF_EINVAL, "null argument");
  int rc = fk20_domain(n, omega2, w2m);
  if (rc || (rc = cells_l(n, l, log_l))) return rc;
  if (srs_m < n - l) return fail(PBF_EINVAL, "SRS too short");
  return 0;
}
int cells_open_args(pbf_ctx* ctx, const uint64_t* xext, size_t n, size_t l, const uint64_t* omega2,
                    const uint64_t* polys, size_t len, size_t pitch, size_t batch, const uint64_t* weights,
                    const uint64_t* out_w, U256* w2m, uint32_t* log_l) {
  int rc = fk20_open_args(ctx, xext, n, omega2, polys, len, pitch, batch, weights, out_w, w2m);
  if (rc) return rc;
  return cells_l(n, l, log_l);
}

}  // namespace

int pbf::cells_ystore_run(const uint64_t* y, uint64_t batch, uint64_t k, uint32_t log_l, uint64_t* out, hipStream_t s) {
  const uint64_t total = (batch * k) << log_l;
  hipLaunchKernelGGL(k_cells_ystore, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, y, total, k, log_l, out);
  PBF_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- Poly::eval over Fr
extern "C" int pbf_poly_eval_fr256(pbf_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t* xs, size_t nx,
                                   uint64_t* ys) {
  if (!ctx || !coeffs || !xs || !ys) return fail(PBF_EINVAL, "null argument");
  if (n == 0 || nx == 0) return fail(PBF_EINVAL, "n and nx must be at least 1");
  if (!fr_canonical(xs, nx)) return fail(PBF_EINVAL, "evaluation point not canonical");
  if (!fr_canonical(coeffs, n)) return fail(PBF_EINVAL, "coefficient not canonical");
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  int rc;
  if ((rc = ctx->io0.ensure(n * 32)) || (rc = ctx->io1.ensure(nx * 32))) return rc;
  PBF_HIP(hipMemcpyAsync(ctx->io0.p, coeffs, n * 32, hipMemcpyHostToDevice, s));
  // the evaluation kernel keeps power tables of two points per launch
  for (size_t i = 0; i < nx; i += 2) {
    const int g = (int)std::min<size_t>(2, nx - i);
    const uint64_t* polys[2] = {(const uint64_t*)ctx->io0.p, (const uint64_t*)ctx->io0.p};
    const uint64_t lens[2] = {n, n};
    const U256 pt[2] = {Fr::to_mont(u256_from_u64(xs + 4 * i)), Fr::to_mont(u256_from_u64(xs + 4 * (i + g - 1)))};
    if ((rc = fr_eval_run(polys, lens, pt, g, 0, ctx->partial, (uint64_t*)ctx->io1.p + 4 * i, s))) return rc;
  }
  PBF_HIP(hipMemcpyAsync(ys, ctx->io1.p, nx * 32, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  return PBF_OK;
}

// ---------------------------------------------------------------- commit
extern "C" int pbf_kzg_commit_bn254_dev(pbf_ctx* ctx, const uint64_t* d_srs, size_t srs_m, const uint64_t* d_polys,
                                        size_t len, size_t pitch, size_t batch, uint64_t* out_pts, void* stream) {
  if (!out_pts) return fail(PBF_EINVAL, "null argument");
  int rc = poly_args(ctx, d_srs, srs_m, d_polys, len, pitch, batch, len);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  DevBuf& res = ctx->buf("kzg.commits");
  if ((rc = res.ensure(batch * sizeof(Xyzz)))) return rc;
  const Affine* tbl = nullptr;
  if ((rc = msm_fixed_table(ctx, d_srs, srs_m, s, &tbl))) return rc;
  for (size_t b = 0; b < batch; ++b)
    if ((rc = msm_fixed_device(ctx, tbl, srs_m, 0, d_polys + 4 * b * pitch, len, s, (Xyzz*)res.p + b))) return rc;
  if ((rc = msm_fixed_wait(ctx, s))) return rc;
  std::vector<Xyzz> h(batch);
  PBF_HIP(hipMemcpyAsync(h.data(), res.p, batch * sizeof(Xyzz), hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  for (size_t b = 0; b < batch; ++b) xyzz_to_affine_u64(h[b], out_pts + 8 * b);
  return PBF_OK;
}

extern "C" int pbf_kzg_commit_bn254(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* polys, size_t len,
                                    size_t pitch, size_t batch, uint64_t* out_pts) {
  if (!out_pts) return fail(PBF_EINVAL, "null argument");
  int rc = poly_args(ctx, srs, srs_m, polys, len, pitch, batch, len);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  if ((rc = upload_polys(ctx, srs, srs_m, polys, len, pitch, batch, s))) return rc;
  return pbf_kzg_commit_bn254_dev(ctx, (const uint64_t*)ctx->buf("kzg.srs").p, srs_m,
                                  (const uint64_t*)ctx->buf("kzg.polys").p, len, len, batch, out_pts, s);
}

// ---------------------------------------------------------------- open
extern "C" int pbf_kzg_open_bn254_dev(pbf_ctx* ctx, const uint64_t* d_srs, size_t srs_m, const uint64_t* d_polys,
                                      size_t len, size_t pitch, size_t batch, const uint64_t* z,
                                      const uint64_t* weights, uint64_t* out_y, uint64_t* out_w, void* stream) {
  int rc = open_args(ctx, d_srs, srs_m, d_polys, len, pitch, batch, z, weights, out_y, out_w);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  DevBuf &bq = ctx->buf("kzg.q"), &by = ctx->buf("kzg.y"), &res = ctx->buf("kzg.w");
  if ((rc = bq.ensure(std::max<size_t>(len - 1, 1) * 32)) || (rc = by.ensure(batch * 32)) ||
      (rc = res.ensure(sizeof(Xyzz))))
    return rc;
  const bool with_msm = len > 1;  // a constant polynomial's quotient is empty: W = the identity
  const Affine* tbl = nullptr;  // validated (one stream sync) before the sweep is enqueued
  if (with_msm && (rc = msm_fixed_table(ctx, d_srs, srs_m, s, &tbl))) return rc;
  const U256 zm = Fr::to_mont(u256_from_u64(z));
  std::vector<U256> w(batch);
  for (size_t b = 0; b < batch; ++b) w[b] = Fr::to_mont(u256_from_u64(weights + 4 * b));
  uint64_t *q = (uint64_t*)bq.p, *d_y = (uint64_t*)by.p;
  rc = open_sweeps(ctx, d_polys, len, pitch, batch, zm, w, q, d_y, s);
  if (rc) return rc;
  Xyzz hw;
  if (with_msm) {
    if ((rc = msm_fixed_device(ctx, tbl, srs_m, 0, q, len - 1, s, (Xyzz*)res.p))) return rc;
    if ((rc = msm_fixed_wait(ctx, s))) return rc;
    PBF_HIP(hipMemcpyAsync(&hw, res.p, sizeof(Xyzz), hipMemcpyDeviceToHost, s));
  }
  PBF_HIP(hipMemcpyAsync(out_y, d_y, batch * 32, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  if (with_msm) xyzz_to_affine_u64(hw, out_w);
  else for (int i = 0; i < 8; ++i) out_w[i] = 0;  // the empty quotient: the identity
  return PBF_OK;
}

extern "C" int pbf_kzg_open_bn254(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* polys, size_t len,
                                  size_t pitch, size_t batch, const uint64_t* z, const uint64_t* weights,
                                  uint64_t* out_y, uint64_t* out_w) {
  int rc = open_args(ctx, srs, srs_m, polys, len, pitch, batch, z, weights, out_y, out_w);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  if ((rc = upload_polys(ctx, srs, srs_m, polys, len, pitch, batch, s))) return rc;
  return pbf_kzg_open_bn254_dev(ctx, (const uint64_t*)ctx->buf("kzg.srs").p, srs_m,
                                (const uint64_t*)ctx->buf("kzg.polys").p, len, len, batch, z, weights, out_y, out_w, s);
}

// ---------------------------------------------------------------- verify
extern "C" int pbf_kzg_verify_bn254(pbf_ctx* ctx, const uint64_t* g2, size_t count, const uint64_t* commits,
                                    const uint64_t* z, const uint64_t* y, const uint64_t* w, const uint64_t* rho,
                                    int* ok) {
  if (!ctx || !g2 || !commits || !z || !y || !w || !rho || !ok) return fail(PBF_EINVAL, "null argument");
  *ok = 0;
  if (count == 0 || count > ((size_t)1 << 20)) return fail(PBF_EINVAL, "count must be in 1 .. 2^20");
  if (!fr_canonical(z, count) || !fr_canonical(y, count)) return fail(PBF_EINVAL, "z and y must be canonical");
  for (size_t i = 0; i < count; ++i) {
    const uint64_t* r = rho + 4 * i;
    if (!fr_canonical(r) || !(r[0] | r[1] | r[2] | r[3])) return fail(PBF_EINVAL, "rho must be canonical and nonzero");
  }
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  const size_t c = count;
  const uint32_t nparts = (uint32_t)((c + 255) / 256);
  DevBuf &bi = ctx->buf("kzg.v.in"), &bp = ctx->buf("kzg.v.pts"), &bs = ctx->buf("kzg.v.sc"),
         &bpart = ctx->buf("kzg.v.part"), &bfl = ctx->buf("kzg.v.flag");
  int rc;
  // inputs: commits, w (8 words each), z, y, rho (4 each) per entry
  if ((rc = bi.ensure(c * 28 * 8)) || (rc = bp.ensure((2 * c + 1) * 64)) || (rc = bs.ensure((2 * c + 1) * 32)) ||
      (rc = bpart.ensure((size_t)nparts * 32)) || (rc = bfl.ensure(sizeof(int))))
    return rc;
  uint64_t *in = (uint64_t*)bi.p, *pts = (uint64_t*)bp.p, *sc = (uint64_t*)bs.p;
  uint64_t *d_c = in, *d_w = in + 8 * c, *d_z = in + 16 * c, *d_y = in + 20 * c, *d_rho = in + 24 * c;
  PBF_HIP(hipMemcpyAsync(d_c, commits, c * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(d_w, w, c * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(d_z, z, c * 32, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(d_y, y, c * 32, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(d_rho, rho, c * 32, hipMemcpyHostToDevice, s));
  static const uint64_t G1_GEN[8] = {1, 0, 0, 0, 2, 0, 0, 0};
  PBF_HIP(hipMemcpyAsync(pts + 16 * c, G1_GEN, 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemsetAsync(bfl.p, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_kzg_vprep, dim3(nparts), dim3(256), 0, s, (const uint64_t*)d_c, (const uint64_t*)d_w,
                     (const uint64_t*)d_z, (const uint64_t*)d_y, (const uint64_t*)d_rho, (uint32_t)c, pts, sc,
                     (uint64_t*)bpart.p, (int*)bfl.p);
  hipLaunchKernelGGL(k_kzg_vsum, dim3(1), dim3(256), 0, s, (const uint64_t*)bpart.p, nparts, sc + 8 * c);
  PBF_HIP(hipGetLastError());
  int bad = 0;
  PBF_HIP(hipMemcpyAsync(&bad, bfl.p, sizeof(int), hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  if (bad) return PBF_OK;  // a point not canonical or not on the curve: *ok = 0
  uint64_t e1[8], e2[8];
  if ((rc = pbf_msm_g1_bn254_dev(ctx, pts + 8 * c, sc, c, e1, s))) return rc;  // sum rho_i W_i
  if ((rc = pbf_msm_g1_bn254_dev(ctx, pts, sc, 2 * c + 1, e2, s))) return rc;
  // e(sum rho W, [s]G2) e(-sum rho (C - y G + z W), G2) == 1
  uint64_t g1s[16], g2s[32];
  memcpy(g1s, e1, 64);
  neg_g1(e2, g1s + 8);
  memcpy(g2s, g2 + 16, 128);  // [s]G2
  memcpy(g2s + 16, g2, 128);  // G2
  return pairing_check_on_stream(ctx, g1s, g2s, 2, ok, s);
}

// ---------------------------------------------------------------- open from evaluations
extern "C" int pbf_kzg_open_evals_bn254_dev(pbf_ctx* ctx, const uint64_t* d_lsrs, size_t n, const uint64_t* omega,
                                            const uint64_t* d_evals, size_t pitch, size_t batch, const uint64_t* z,
                                            const uint64_t* weights, uint64_t* out_y, uint64_t* out_w, void* stream) {
  U256 wm;
  int rc = open_evals_args(ctx, d_lsrs, n, omega, d_evals, pitch, batch, z, weights, out_y, out_w, &wm);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  if (n == 1) {  // a constant: y_b = p_b[0], the quotient is zero and the SRS is not read
    PBF_HIP(hipMemcpy2DAsync(out_y, 32, d_evals, pitch * 32, 32, batch, hipMemcpyDeviceToHost, s));
    PBF_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < 8; ++i) out_w[i] = 0;
    return PBF_OK;
  }
  DevBuf &bq = ctx->buf("kzg.q"), &by = ctx->buf("kzg.y"), &res = ctx->buf("kzg.w");
  if ((rc = bq.ensure(n * 32)) || (rc = by.ensure(batch * 32)) || (rc = res.ensure(sizeof(Xyzz)))) return rc;
  const Affine* tbl = nullptr;  // validated (one stream sync) before the sweeps are enqueued
  if ((rc = msm_fixed_table(ctx, d_lsrs, n, s, &tbl))) return rc;
  const uint64_t* tw = nullptr;
  if ((rc = fr_domain_table(ctx, wm, n, s, &tw))) return rc;
  std::vector<U256> w(batch);
  for (size_t b = 0; b < batch; ++b) w[b] = hm(weights + 4 * b);
  uint64_t *q = (uint64_t*)bq.p, *d_y = (uint64_t*)by.p;
  if ((rc = open_evals_sweeps(ctx, tw, n, d_evals, pitch, batch, hm(z), w, q, d_y, s))) return rc;
  if ((rc = msm_fixed_device(ctx, tbl, n, 0, q, n, s, (Xyzz*)res.p))) return rc;
  if ((rc = msm_fixed_wait(ctx, s))) return rc;
  Xyzz hw;
  PBF_HIP(hipMemcpyAsync(&hw, res.p, sizeof(Xyzz), hipMemcpyDeviceToHost, s));
  PBF_HIP(hipMemcpyAsync(out_y, d_y, batch * 32, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  xyzz_to_affine_u64(hw, out_w);
  return PBF_OK;
}

extern "C" int pbf_kzg_open_evals_bn254(pbf_ctx* ctx, const uint64_t* lsrs, size_t n, const uint64_t* omega,
                                        const uint64_t* evals, size_t pitch, size_t batch, const uint64_t* z,
                                        const uint64_t* weights, uint64_t* out_y, uint64_t* out_w) {
  U256 wm;
  int rc = open_evals_args(ctx, lsrs, n, omega, evals, pitch, batch, z, weights, out_y, out_w, &wm);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  if ((rc = upload_polys(ctx, lsrs, n, evals, n, pitch, batch, s))) return rc;
  return pbf_kzg_open_evals_bn254_dev(ctx, (const uint64_t*)ctx->buf("kzg.srs").p, n, omega,
                                      (const uint64_t*)ctx->buf("kzg.polys").p, n, batch, z, weights, out_y, out_w, s);
}

// ---------------------------------------------------------------- every opening at once (FK20)
extern "C" int pbf_kzg_fk20_setup_bn254_dev(pbf_ctx* ctx, const uint64_t* d_srs, size_t srs_m, const uint64_t* omega2,
                                            size_t n, uint64_t* d_xext, void* stream) {
  U256 w2m;
  int rc = fk20_setup_args(ctx, d_srs, srs_m, omega2, n, d_xext, &w2m);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  if (n == 1) {  // a is two identities, and so is its transform
    PBF_HIP(hipMemsetAsync(d_xext, 0, 128, s));
    return PBF_OK;
  }
  hipLaunchKernelGGL(k_fk20_a, dim3((uint32_t)((2 * n + 255) / 256)), dim3(256), 0, s, d_srs, (uint64_t)n, d_xext);
  PBF_HIP(hipGetLastError());
  return g1_ntt_run(ctx, w2m, d_xext, d_xext, 2 * n, 0, s);
}

extern "C" int pbf_kzg_fk20_setup_bn254(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* omega2,
                                        size_t n, uint64_t* xext) {
  U256 w2m;
  int rc = fk20_setup_args(ctx, srs, srs_m, omega2, n, xext, &w2m);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  const size_t used = n - 1;  // the points the setup reads
  DevBuf &ds = ctx->buf("kzg.srs"), &dx = ctx->buf("kzg.fk20.xext");
  if ((rc = ds.ensure(std::max<size_t>(used, 1) * 64)) || (rc = dx.ensure(2 * n * 64))) return rc;
  if (used) {
    PBF_HIP(hipMemcpyAsync(ds.p, srs, used * 64, hipMemcpyHostToDevice, s));
    int bad = 0;
    if ((rc = g1_check_run(ctx, (const uint64_t*)ds.p, used, s, &bad))) return rc;
    if (bad) return fail(PBF_EINVAL, "a point is not canonical or not on the curve");
  }
  if ((rc = pbf_kzg_fk20_setup_bn254_dev(ctx, (const uint64_t*)ds.p, used, omega2, n, (uint64_t*)dx.p, s))) return rc;
  PBF_HIP(hipMemcpyAsync(xext, dx.p, 2 * n * 64, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  return PBF_OK;
}

extern "C" int pbf_kzg_open_all_bn254_dev(pbf_ctx* ctx, const uint64_t* d_xext, size_t n, const uint64_t* omega2,
                                          const uint64_t* d_polys, size_t len, size_t pitch, size_t batch,
                                          const uint64_t* weights, uint64_t* d_out_y, uint64_t* d_out_w, void* stream) {
  U256 w2m;
  int rc = fk20_open_args(ctx, d_xext, n, omega2, d_polys, len, pitch, batch, weights, d_out_w, &w2m);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const uint64_t one[4] = {1, 0, 0, 0};
  const U256 wm = Fr::mul(w2m, w2m);  // omega = omega2^2, of order n
  uint64_t om[4];
  hout(om, wm);
  // y_b = the size-n Fr NTT of p_b, zero-padded from len
  if (d_out_y && n == 1) {
    PBF_HIP(hipMemcpy2DAsync(d_out_y, 32, d_polys, pitch * 32, 32, batch, hipMemcpyDeviceToDevice, s));
  } else if (d_out_y && pitch == len) {
    if ((rc = pbf_ntt_fr256_coset_batch_dev(ctx, om, one, d_polys, len, d_out_y, n, batch, 0, s))) return rc;
  } else if (d_out_y) {
    for (size_t b = 0; b < batch; ++b)
      if ((rc = pbf_ntt_fr256_coset_batch_dev(ctx, om, one, d_polys + 4 * b * pitch, len, d_out_y + 4 * b * n, n, 1, 0, s)))
        return rc;
  }
  if (len == 1) {  // constants: every quotient is empty, every W the identity
    PBF_HIP(hipMemsetAsync(d_out_w, 0, n * 64, s));
    return PBF_OK;
  }
  const uint64_t n2 = 2 * (uint64_t)n;
  DevBuf &bc = ctx->buf("kzg.comb"), &bb = ctx->buf("kzg.fk20.bhat");
  G1Work w;
  if ((rc = bc.ensure(len * 32)) || (rc = bb.ensure(n2 * 32)) || (rc = g1_work(ctx, n2, n2, &w))) return rc;
  uint64_t *comb = (uint64_t*)bc.p, *bhat = (uint64_t*)bb.p;
  // c = (2n)^-1 sum_b w_b p_b: the inverse transform's factor rides on the weights
  const U256 inv2n = fr_inv(hm64(n2));
  if ((rc = fk20_comb(d_polys, len, pitch, batch, weights, inv2n, comb, s))) return rc;
  if ((rc = pbf_ntt_fr256_coset_batch_dev(ctx, omega2, one, comb, len, bhat, n2, 1, 0, s))) return rc;
  // chat_i = [bhat_i] xext_i where the inverse transform reads it; c = a * b; h = c[n-1 .. 2n-1); W = NTT_n(h)
  if ((rc = g1_mul_xyzz_run(w, d_xext, bhat, n2, s)) || (rc = g1_ntt_stages(ctx, w2m, n2, w, s)) ||
      (rc = g1_ntt_slice(w, n, s)) || (rc = g1_ntt_stages(ctx, wm, n, w, s)))
    return rc;
  return g1_ntt_store(w, d_out_w, n, s);
}

extern "C" int pbf_kzg_open_all_bn254(pbf_ctx* ctx, const uint64_t* xext, size_t n, const uint64_t* omega2,
                                      const uint64_t* polys, size_t len, size_t pitch, size_t batch,
                                      const uint64_t* weights, uint64_t* out_y, uint64_t* out_w) {
  U256 w2m;
  int rc = fk20_open_args(ctx, xext, n, omega2, polys, len, pitch, batch, weights, out_w, &w2m);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  if ((rc = upload_polys(ctx, xext, 2 * n, polys, len, pitch, batch, s))) return rc;
  DevBuf &by = ctx->buf("kzg.fk20.y"), &bw = ctx->buf("kzg.fk20.w");
  if ((out_y && (rc = by.ensure(batch * n * 32))) || (rc = bw.ensure(n * 64))) return rc;
  if ((rc = pbf_kzg_open_all_bn254_dev(ctx, (const uint64_t*)ctx->buf("kzg.srs").p, n, omega2,
                                       (const uint64_t*)ctx->buf("kzg.polys").p, len, len, batch, weights,
                                       out_y ? (uint64_t*)by.p : nullptr, (uint64_t*)bw.p, s)))
    return rc;
  if (out_y) PBF_HIP(hipMemcpyAsync(out_y, by.p, batch * n * 32, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipMemcpyAsync(out_w, bw.p, n * 64, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  return PBF_OK;
}

// ---------------------------------------------------------------- cell proofs (FK20 over cosets)
extern "C" int pbf_kzg_cells_setup_bn254_dev(pbf_ctx* ctx, const uint64_t* d_srs, size_t srs_m, const uint64_t* omega2,
                                             size_t n, size_t l, uint64_t* d_xext, void* stream) {
  U256 w2m;
  uint32_t log_l;
  int rc = cells_setup_args(ctx, d_srs, srs_m, omega2, n, l, d_xext, &w2m, &log_l);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const uint64_t k = n / l, k2 = 2 * k;
  if (k == 1) {  // every a_r is two identities, and so is its transform
    PBF_HIP(hipMemsetAsync(d_xext, 0, 2 * n * 64, s));
    return PBF_OK;
  }
  hipLaunchKernelGGL(k_cells_a, dim3((uint32_t)((2 * n + 255) / 256)), dim3(256), 0, s, d_srs, k, log_l, d_xext);
  PBF_HIP(hipGetLastError());
  const U256 wlm = fr_pow(w2m, l);  // omega2^l, of order 2k
  for (uint64_t r = 0; r < l; ++r)
    if ((rc = g1_ntt_run(ctx, wlm, d_xext + 8 * r * k2, d_xext + 8 * r * k2, k2, 0, s))) return rc;
  return PBF_OK;
}

extern "C" int pbf_kzg_cells_setup_bn254(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* omega2,
                                         size_t n, size_t l, uint64_t* xext) {
  U256 w2m;
  uint32_t log_l;
  int rc = cells_setup_args(ctx, srs, srs_m, omega2, n, l, xext, &w2m, &log_l);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  const size_t used = n - l;  // the points the setup reads
  DevBuf &ds = ctx->buf("kzg.srs"), &dx = ctx->buf("kzg.fk20.xext");
  if ((rc = ds.ensure(std::max<size_t>(used, 1) * 64)) || (rc = dx.ensure(2 * n * 64))) return rc;
  if (used) {
    PBF_HIP(hipMemcpyAsync(ds.p, srs, used * 64, hipMemcpyHostToDevice, s));
    int bad = 0;
    if ((rc = g1_check_run(ctx, (const uint64_t*)ds.p, used, s, &bad))) return rc;
    if (bad) return fail(PBF_EINVAL, "a point is not canonical or not on the curve");
  }
  if ((rc = pbf_kzg_cells_setup_bn254_dev(ctx, (const uint64_t*)ds.p, used, omega2, n, l, (uint64_t*)dx.p, s))) return rc;
  PBF_HIP(hipMemcpyAsync(xext, dx.p, 2 * n * 64, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  return PBF_OK;
}

extern "C" int pbf_kzg_open_cells_bn254_dev(pbf_ctx* ctx, const uint64_t* d_xext, size_t n, size_t l,
                                            const uint64_t* omega2, const uint64_t* d_polys, size_t len, size_t pitch,
                                            size_t batch, const uint64_t* weights, uint64_t* d_out_y, uint64_t* d_out_w,
                                            void* stream) {
  U256 w2m;
  uint32_t log_l;
  int rc = cells_open_args(ctx, d_xext, n, l, omega2, d_polys, len, pitch, batch, weights, d_out_w, &w2m, &log_l);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const uint64_t one[4] = {1, 0, 0, 0};
  const uint64_t k = n / l, k2 = 2 * k, n2 = 2 * (uint64_t)n;
  const U256 wm = Fr::mul(w2m, w2m);  // omega = omega2^2, of order n
  uint64_t om[4];
  hout(om, wm);
  // y_b = the size-n Fr NTT of p_b, zero-padded from len, stored cell-major (l = 1 and l = n: as it stands)
  if (d_out_y && n == 1) {
    PBF_HIP(hipMemcpy2DAsync(d_out_y, 32, d_polys, pitch * 32, 32, batch, hipMemcpyDeviceToDevice, s));
  } else if (d_out_y) {
    const bool direct = l == 1 || k == 1;
    DevBuf& by = ctx->buf("kzg.cells.y");
    if (!direct && (rc = by.ensure(batch * n * 32))) return rc;
    uint64_t* y = direct ? d_out_y : (uint64_t*)by.p;
    if (pitch == len) {
      if ((rc = pbf_ntt_fr256_coset_batch_dev(ctx, om, one, d_polys, len, y, n, batch, 0, s))) return rc;
    } else {
      for (size_t b = 0; b < batch; ++b)
        if ((rc = pbf_ntt_fr256_coset_batch_dev(ctx, om, one, d_polys + 4 * b * pitch, len, y + 4 * b * n, n, 1, 0, s)))
          return rc;
    }
    if (!direct && (rc = cells_ystore_run(y, batch, k, log_l, d_out_y, s))) return rc;
  }
  if (len <= l) {  // degree below l: every quotient is zero, every W the identity (k = 1 included)
    PBF_HIP(hipMemsetAsync(d_out_w, 0, k * 64, s));
    return PBF_OK;
  }
  DevBuf &bc = ctx->buf("kzg.comb"), &bg = ctx->buf("kzg.cells.b"), &bb = ctx->buf("kzg.fk20.bhat");
  G1Work w;
  if ((rc = bc.ensure(len * 32)) || (rc = bg.ensure(n * 32)) || (rc = bb.ensure(n2 * 32)) ||
      (rc = g1_work(ctx, l == 1 ? n2 : n2 + k2, n2, &w)))
    return rc;
  uint64_t *comb = (uint64_t*)bc.p, *b = (uint64_t*)bg.p, *bhat = (uint64_t*)bb.p;
  // c = (2k)^-1 sum_b w_b p_b: the inverse transform's factor rides on the weights
  if ((rc = fk20_comb(d_polys, len, pitch, batch, weights, fr_inv(hm64(k2)), comb, s))) return rc;
  hipLaunchKernelGGL(k_cells_gather, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, (const uint64_t*)comb,
                     (uint64_t)len, k, log_l, b);
  PBF_HIP(hipGetLastError());
  const U256 wlm = fr_pow(w2m, l);  // omega2^l, of order 2k; its square omega^l, of order k
  uint64_t wl[4];
  hout(wl, wlm);
  if ((rc = pbf_ntt_fr256_coset_batch_dev(ctx, wl, one, b, k, bhat, k2, l, 0, s))) return rc;
  // the 2n products as one vector; with l = 1 they lie where the inverse transform reads them,
  // else their sums per frequency are put there, behind the products
  if ((rc = g1_mul_xyzz_run(w, d_xext, bhat, n2, s))) return rc;
  if (l > 1) {
    uint32_t log_k2 = 0;
    while (((uint64_t)1 << log_k2) < k2) ++log_k2;
    hipLaunchKernelGGL(k_cells_sum, dim3((uint32_t)((k2 + GN_T - 1) / GN_T)), dim3(GN_T), 0, s, (const Xyzz*)w.x,
                       w.x + n2, log_k2, log_l);
    PBF_HIP(hipGetLastError());
    w.x += n2;
  }
  // c = a * b summed over the slabs; h = c[k-1 .. 2k-1); W = NTT_k(h)
  if ((rc = g1_ntt_stages(ctx, wlm, k2, w, s)) || (rc = g1_ntt_slice(w, k, s)) ||
      (rc = g1_ntt_stages(ctx, Fr::mul(wlm, wlm), k, w, s)))
    return rc;
  return g1_ntt_store(w, d_out_w, k, s);
}

extern "C" int pbf_kzg_open_cells_bn254(pbf_ctx* ctx, const uint64_t* xext, size_t n, size_t l, const uint64_t* omega2,
                                        const uint64_t* polys, size_t len, size_t pitch, size_t batch,
                                        const uint64_t* weights, uint64_t* out_y, uint64_t* out_w) {
  U256 w2m;
  uint32_t log_l;
  int rc = cells_open_args(ctx, xext, n, l, omega2, polys, len, pitch, batch, weights, out_w, &w2m, &log_l);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  const size_t k = n / l;
  if ((rc = upload_polys(ctx, xext, 2 * n, polys, len, pitch, batch, s))) return rc;
  DevBuf &by = ctx->buf("kzg.fk20.y"), &bw = ctx->buf("kzg.fk20.w");
  if ((out_y && (rc = by.ensure(batch * n * 32))) || (rc = bw.ensure(k * 64))) return rc;
  if ((rc = pbf_kzg_open_cells_bn254_dev(ctx, (const uint64_t*)ctx->buf("kzg.srs").p, n, l, omega2,
                                         (const uint64_t*)ctx->buf("kzg.polys").p, len, len, batch, weights,
                                         out_y ? (uint64_t*)by.p : nullptr, (uint64_t*)bw.p, s)))
    return rc;
  if (out_y) PBF_HIP(hipMemcpyAsync(out_y, by.p, batch * n * 32, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipMemcpyAsync(out_w, bw.p, k * 64, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  return PBF_OK;
}

extern "C" int pbf_kzg_verify_cells_bn254(pbf_ctx* ctx, const uint64_t* g2, const uint64_t* srs, size_t srs_m,
                                          const uint64_t* omega, size_t n, size_t l, size_t count,
                                          const uint64_t* commits, const uint64_t* cell_idx, const uint64_t* ys,
                                          const uint64_t* w, const uint64_t* rho, int* ok) {
  if (!ctx || !g2 || !srs || !omega || !commits || !cell_idx || !ys || !w || !rho || !ok)
    return fail(PBF_EINVAL, "null argument");
  *ok = 0;
  if (n == 0 || (n & (n - 1)) || n > FK20_MAX_N) return fail(PBF_EINVAL, "n must be a power of two in 1 .. 2^27");
  U256 wm;
  uint32_t log_l;
  int rc = fr_domain_check(omega, n, &wm);
  if (rc || (rc = cells_l(n, l, &log_l))) return rc;
  if (srs_m < l) return fail(PBF_EINVAL, "SRS too short");
  if (count == 0 || count > CELLS_MAX_COUNT) return fail(PBF_EINVAL, "count must be in 1 .. 2^20");
  if (count * l > CELLS_MAX_VALUES) return fail(PBF_EINVAL, "count * l must be at most 2^22");
  const size_t k = n / l, c = count, vals = count * l;
  for (size_t i = 0; i < c; ++i)
    if (cell_idx[i] >= k) return fail(PBF_EINVAL, "cell_idx must be below n / l");
  if (!fr_canonical(ys, vals)) return fail(PBF_EINVAL, "ys must be canonical");
  for (size_t i = 0; i < c; ++i) {
    const uint64_t* r = rho + 4 * i;
    if (!fr_canonical(r) || !(r[0] | r[1] | r[2] | r[3])) return fail(PBF_EINVAL, "rho must be canonical and nonzero");
  }
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  const uint32_t nchunks = (uint32_t)((c + CV_CH - 1) / CV_CH);
  DevBuf &bi = ctx->buf("kzg.v.in"), &bp = ctx->buf("kzg.v.pts"), &bs = ctx->buf("kzg.v.sc"),
         &bpart = ctx->buf("kzg.v.part"), &bfl = ctx->buf("kzg.v.flag");
  // inputs: commits, w (8 words each), rho (4), cell_idx (1) per entry; the values and their inverse transforms
  if ((rc = bi.ensure((c * 21 + vals * 8) * 8)) || (rc = bp.ensure((2 * c + l) * 64)) ||
      (rc = bs.ensure((2 * c + l) * 32)) || (rc = bpart.ensure(((size_t)nchunks << log_l) * 32)) ||
      (rc = bfl.ensure(sizeof(int))))
    return rc;
  const uint64_t* tw = nullptr;
  if (n > 1 && (rc = fr_domain_table(ctx, wm, n, s, &tw))) return rc;
  uint64_t *in = (uint64_t*)bi.p, *pts = (uint64_t*)bp.p, *sc = (uint64_t*)bs.p;
  uint64_t *d_c = in, *d_w = in + 8 * c, *d_rho = in + 16 * c, *d_idx = in + 20 * c, *d_y = in + 21 * c;
  uint64_t* d_v = l > 1 ? d_y + 4 * vals : d_y;  // the inverse transform of size 1 is the value itself
  PBF_HIP(hipMemcpyAsync(d_c, commits, c * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(d_w, w, c * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(d_rho, rho, c * 32, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(d_idx, cell_idx, c * 8, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(d_y, ys, vals * 32, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(pts + 16 * c, srs, l * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemsetAsync(bfl.p, 0, sizeof(int), s));
  if (l > 1) {  // v_j = INTT_l(y_j), root omega^k, all cells in one batch
    uint64_t wk[4];
    hout(wk, fr_pow(wm, k));
    if ((rc = pbf_ntt_fr256_batch_dev(ctx, wk, d_y, d_v, l, c, 1, s))) return rc;
  }
  hipLaunchKernelGGL(k_cells_vprep, dim3((uint32_t)((std::max(c, l) + 255) / 256)), dim3(256), 0, s,
                     (const uint64_t*)d_c, (const uint64_t*)d_w, (const uint64_t*)d_rho, (const uint64_t*)d_idx,
                     (uint32_t)c, tw, (uint64_t)n, log_l, pts, sc, (int*)bfl.p);
  hipLaunchKernelGGL(k_cells_vsweep, dim3((uint32_t)((((uint64_t)nchunks << log_l) + 255) / 256)), dim3(256), 0, s,
                     (const uint64_t*)d_v, (const uint64_t*)d_rho, (const uint64_t*)d_idx, (uint32_t)c, tw, (uint64_t)n,
                     log_l, nchunks, (uint64_t*)bpart.p);
  hipLaunchKernelGGL(k_cells_vsum, dim3((uint32_t)l), dim3(256), 0, s, (const uint64_t*)bpart.p, nchunks, log_l,
                     sc + 8 * c);
  PBF_HIP(hipGetLastError());
  int bad = 0;
  PBF_HIP(hipMemcpyAsync(&bad, bfl.p, sizeof(int), hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  if (bad) return PBF_OK;  // a point not canonical or not on the curve: *ok = 0
  uint64_t e1[8], e2[8];
  if ((rc = pbf_msm_g1_bn254_dev(ctx, pts + 8 * c, sc, c, e1, s))) return rc;  // sum rho_j W_j
  if ((rc = pbf_msm_g1_bn254_dev(ctx, pts, sc, 2 * c + l, e2, s))) return rc;
  // e(sum rho W, [s^l]G2) e(-(sum rho C - [sum rho I](s) G + sum rho c W), G2) == 1
  uint64_t g1s[16], g2s[32];
  memcpy(g1s, e1, 64);
  neg_g1(e2, g1s + 8);
  memcpy(g2s, g2 + 16, 128);  // [s^l]G2
  memcpy(g2s + 16, g2, 128);  // G2
  return pairing_check_on_stream(ctx, g1s, g2s, 2, ok, s);
}
