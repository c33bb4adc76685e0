// Batched Plonk::verify over BN254 on gfx950: `count` proofs of one circuit, one 2-pair
// pairing check (include/pbf.h pbf_plonk_verify_bn254_batch*).
//
// The single verifier (verify.hip) checks, per proof i,
//     e(E1_i, [s]G2) == e(E2_i, G2),   E1_i = W_z,i + u_i W_zw,i,   E2_i = sum_j scal_ij base_ij
// with 18 bases: the proof's 9 points, the circuit's 8 preprocessed commitments and G. The
// pairing is bilinear, so for caller-chosen weights rho_i
//     e(sum_i rho_i E1_i, [s]G2) == e(sum_i rho_i E2_i, G2)
// holds when every proof's equation does, and fails with overwhelming probability over
// unpredictable rho when one does not. The 9 shared bases collect sum_i rho_i scal_ij, so the
// batch is one MSM over 9 count + 9 points, one over 2 count points and one pairing check.
//
// Work split:
//   k_vb_curve    one lane per proof POINT: canonical coordinates, y^2 = x^3 + 3 in Fq; ORs
//                 into the proof's flag; gathers W_z, W_zw into the compact E1 point array
//   k_vb_scalars  one lane per PROOF (blocks of one wave): fields canonical, then steps 4-10 as
//                 plonk_terms.hpp states them for this kernel and the single verifier
//                 (plonk_verifier_scalars: Z_H(z) != 0, the Fr formulas scaled by rho_i); a flagged
//                 proof's scalars are written as zero, so its points ride through the MSM inert
//   k_vb_pi_*     public inputs (the _pi entries): sum_j pub_ij w^j / (z_i - w^j) of every proof as
//                 one fraction (N_i, D_i): a wave per (chunk of 256 inputs, proof), then a wave per
//                 proof over its chunks; plonk_verifier_scalars folds D_i into its one inversion
//   k_vb_colsum*  the 9 shared-base scalars of an index range [lo, hi): LDS tree per block,
//                 second step across blocks (field addition is exact: any order, same limbs)
// chal, u and rho reach the device by upload, or (the _fs entries) are written there by the
// transcript's kernels (transcript.hip fs_batch_run) from the proofs and pub this unit uploads.
// Every scalar is the canonical value the single verifier's run of the same formulas gives.
// Localisation (ok_each) halves the index range, recomputing only the column sums, the two MSMs and
// the pairing per range.
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../include/pbf.h"
#include "plonk_terms.hpp"
#include "prover.hpp"
#include "transcript.hpp"

using namespace pbf;

namespace {

constexpr uint32_t VB_PART = 64;  // column-sum partial blocks per column (one wave in step 2)
// The E1 MSM runs over W_z, W_zw gathered compactly: E1_N points and scalars (rho, rho u) per proof.
constexpr uint32_t E1_N = 2;

struct VbParams {
  U256 k1, k2;  // Montgomery
  PlonkDomain dom;
  uint32_t count;
  int mode;
};

__device__ __forceinline__ U256 ldm(const uint64_t* p) { return Fr::to_mont(u256_from_u64(p)); }
__device__ __forceinline__ void st_zero(uint64_t* p) { p[0] = p[1] = p[2] = p[3] = 0; }

// flag bits: 1 a point not canonical / off the curve, 2 a field >= r, 4 Z_H(z) = 0
__global__ void __launch_bounds__(256) k_vb_curve(const uint64_t* pts, uint32_t npts, int* flag, uint64_t* e1pts) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npts) return;
  const uint32_t i = t / 9, j = t % 9;
  const uint64_t* p = pts + 8 * (uint64_t)t;
  uint64_t l[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) l[k] = p[k];
  if (j >= 7) {
    uint64_t* o = e1pts + 8 * ((uint64_t)2 * i + (j - 7));
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = l[k];
  }
  uint64_t any = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) any |= l[k];
  if (any == 0) return;  // the identity (0, 0) is accepted (G1P::in_curve)
  const U256 x = u256_from_u64(l), y = u256_from_u64(l + 4);
  bool bad = Fq::geq_p(x) || Fq::geq_p(y);
  if (!bad) {
    const U256 xm = Fq::to_mont(x), ym = Fq::to_mont(y);
    U256 three = u256_zero();
    three.w[0] = 3;
    const U256 rhs = Fq::add(Fq::mul(Fq::mul(xm, xm), xm), Fq::to_mont(three));
    bad = !Fq::eq(Fq::mul(ym, ym), rhs);
  }
  if (bad) atomicOr(flag + i, 1);
}

// Steps 4-10 (plonk_terms.hpp plonk_verifier_scalars) for proof i = one lane, every output times rho_i:
//   sc[9 i + j]      j < 9: a b c z t_lo t_mid t_hi w_z w_zw
//   e1s[E1_N i + 0, 1]  rho, rho u
//   contrib[j][i]    j < 9: q_m q_l q_r q_o q_c s1 s2 (-d3 on s3) (-E on G)
// What is about storage stays here: the fields canonical, and zeros for a flagged proof (Z_H(z) is
// looked at only for a proof not yet flagged). PI: step 7 takes r_z + PI(z) from the fraction
// (N_i, D_i) of pi_nd (k_vb_pi_*); PI = false is the kernel of the plain entries.
template <bool PI>
__global__ void __launch_bounds__(64) k_vb_scalars(const uint64_t* __restrict__ pf, const uint64_t* __restrict__ chal,
                                                   const uint64_t* __restrict__ u_in, const uint64_t* __restrict__ rho_in,
                                                   const uint64_t* __restrict__ pi_nd, VbParams P, int* flag,
                                                   uint64_t* sc, uint64_t* e1s, uint64_t* contrib) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.count) return;
  const uint64_t* f = pf + 28 * (uint64_t)i;
  const uint64_t* ch = chal + 20 * (uint64_t)i;
  int bad = flag[i];
  for (int k = 0; k < 7; ++k)
    if (Fr::geq_p(u256_from_u64(f + 4 * k))) bad |= 2;
  if (!bad) {
    const PlonkChallenges c{ldm(ch), ldm(ch + 4), ldm(ch + 8), ldm(ch + 12), ldm(ch + 16), P.k1, P.k2};
    PlonkEvals e;  // Proof order: a b c s1 s2 r zw
    e.a_z = ldm(f), e.b_z = ldm(f + 4), e.c_z = ldm(f + 8), e.s1_z = ldm(f + 12), e.s2_z = ldm(f + 16);
    e.r_z = ldm(f + 20), e.zw_z = ldm(f + 24);
    const PlonkVerifierArgs g{ldm(u_in + 4 * (uint64_t)i), ldm(rho_in + 4 * (uint64_t)i), P.dom, P.mode};
    const uint32_t count = P.count;
    const auto store = [=](int j, const U256& m) {  // canonical, where the MSMs and the column sums read
      hout(j < 9 ? sc + 4 * ((uint64_t)9 * i + j)
                 : j < 11 ? e1s + 4 * ((uint64_t)E1_N * i + (j - 9)) : contrib + 4 * ((uint64_t)(j - 11) * count + i),
           m);
    };
    // D_i = prod_j (z w^-j - 1) is zero only for z in H, which is Z_H(z) = 0: never read then
    if (!plonk_verifier_scalars(c, e, g, PI ? pi_nd + 8 * (uint64_t)i : nullptr, store)) bad = 4;
  }
  if (bad) {
    flag[i] = bad;
    for (int j = 0; j < 9; ++j) st_zero(sc + 4 * ((uint64_t)9 * i + j));
    for (uint32_t j = 0; j < E1_N; ++j) st_zero(e1s + 4 * ((uint64_t)E1_N * i + j));
    for (int j = 0; j < 9; ++j) st_zero(contrib + 4 * ((uint64_t)j * P.count + i));
  }
}

// ---- public inputs: PI(z) = -(z^n - 1)/n * S, S = sum_{j<npub} pub_j w^j / (z - w^j) = sum_j pub_j / (z w^-j - 1)
// S is kept as a fraction (N, D): adding the term p / d is (N, D) <- (N d + p D, D d), two
// fractions add as (N1 D2 + N2 D1, D1 D2); no inversion until k_vb_scalars' one. Field sums and
// products are exact, so every order of combination gives the same value N / D. z in H makes a d
// zero and with it D (and N / D meaningless): the kernels run through, and k_vb_scalars never
// reads the fraction of such a proof (flag bit 4).
constexpr uint32_t PI_PER = 4, PI_BLK = 64 * PI_PER;  // one wave per chunk: lane l takes j = chunk PI_BLK + l + 64 k
constexpr int PI_VBITS = 20;                          // chunks < 2^20 (npub <= n <= 2^26)
struct PiPow {
  U256 step;          // w^-64
  U256 tl[64];        // w^-l
  U256 tv[PI_VBITS];  // w^-(PI_BLK 2^k)
};
static_assert(sizeof(PiPow) + 64 <= 4096, "kernel argument limit");

// the wave's fractions added up through LDS (shN, shD: 64 values each); the sum on every lane
__device__ __forceinline__ void pi_wave_sum(U256* shN, U256* shD, U256& N, U256& D) {
  const uint32_t t = threadIdx.x;
  shN[t] = N;
  shD[t] = D;
  __syncthreads();
  for (uint32_t s = 32; s; s >>= 1) {
    if (t < s) {
      const U256 n1 = shN[t], d1 = shD[t], n2 = shN[t + s], d2 = shD[t + s];
      shN[t] = Fr::add(fmul(n1, d2), fmul(n2, d1));
      shD[t] = fmul(d1, d2);
    }
    __syncthreads();
  }
  N = shN[0];
  D = shD[0];
}

// part[proof chunks + chunk] = (N, D) of the chunk's terms, Montgomery form; grid chunks x count
// (flat, chunk fastest), one wave. R-degrees: x = z w^-j and d at 1, N at 1, pub as stored (0), so
// D is carried at degree 2 (pub D lands at 1 with no conversion of pub) and lowered once at the end.
__global__ void __launch_bounds__(64) k_vb_pi_partial(const uint64_t* __restrict__ pub, const uint64_t* __restrict__ chal,
                                                      uint32_t npub, uint32_t chunks, PiPow pw, uint64_t* part) {
  __shared__ U256 shN[64], shD[64];
  const uint32_t l = threadIdx.x, v = blockIdx.x % chunks;
  const uint64_t proof = blockIdx.x / chunks;
  const U256 one = Fr::to_mont(Fr::one_plain());
  U256 N = u256_zero(), D = one;
  uint64_t j = (uint64_t)v * PI_BLK + l;
  if (j < npub) {
    U256 x = fmul(ldm(chal + 20 * proof + 12), pw.tl[l]);
    for (uint32_t k = 0, vv = v; vv; vv >>= 1, ++k)
      if (vv & 1) x = fmul(x, pw.tv[k]);
    U256 D2 = Fr::to_mont(one);
    const uint64_t* p = pub + 4 * (proof * npub + j);
    for (uint32_t k = 0; k < PI_PER && j < npub; ++k, j += 64, p += 4 * 64) {
      const U256 d = Fr::sub(x, one);
      N = Fr::add(fmul(N, d), fmul(u256_from_u64(p), D2));
      D2 = fmul(D2, d);
      x = fmul(x, pw.step);
    }
    D = Fr::from_mont(D2);
  }
  pi_wave_sum(shN, shD, N, D);
  if (l == 0) {
    uint64_t* o = part + 8 * (uint64_t)blockIdx.x;
    u256_to_u64(N, o);
    u256_to_u64(D, o + 4);
  }
}

// nd[proof] = the sum of the proof's `chunks` partial fractions; grid count, one wave
__global__ void __launch_bounds__(64) k_vb_pi_combine(const uint64_t* __restrict__ part, uint32_t chunks, uint64_t* nd) {
  __shared__ U256 shN[64], shD[64];
  const uint64_t proof = blockIdx.x;
  U256 N = u256_zero(), D = Fr::to_mont(Fr::one_plain());
  for (uint32_t c = threadIdx.x; c < chunks; c += 64) {
    const uint64_t* p = part + 8 * (proof * chunks + c);
    const U256 n2 = u256_from_u64(p), d2 = u256_from_u64(p + 4);
    N = Fr::add(fmul(N, d2), fmul(n2, D));
    D = fmul(D, d2);
  }
  pi_wave_sum(shN, shD, N, D);
  if (threadIdx.x == 0) {
    u256_to_u64(N, nd + 8 * proof);
    u256_to_u64(D, nd + 8 * proof + 4);
  }
}

// canonical residues add like any others: no Montgomery conversion in the sums (fr_block_sum)
// part[j][b] = sum of contrib[j][i] over this block's share of [lo, hi); grid (nb <= VB_PART, 9)
__global__ void __launch_bounds__(256) k_vb_colsum(const uint64_t* contrib, uint32_t count, uint32_t lo, uint32_t hi,
                                                   uint64_t* part) {
  __shared__ U256 sh[256];
  const uint32_t j = blockIdx.y;
  U256 acc = u256_zero();
  for (uint64_t i = (uint64_t)lo + blockIdx.x * 256u + threadIdx.x; i < hi; i += (uint64_t)gridDim.x * 256u)
    acc = Fr::add(acc, u256_from_u64(contrib + 4 * ((uint64_t)j * count + i)));
  acc = fr_block_sum(sh, acc);
  if (threadIdx.x == 0) u256_to_u64(acc, part + 4 * ((uint64_t)j * VB_PART + blockIdx.x));
}

// out[j] = sum_b part[j][b]; grid 9, one wave
__global__ void __launch_bounds__(64) k_vb_colsum2(const uint64_t* part, uint32_t nb, uint64_t* out) {
  __shared__ U256 sh[VB_PART];
  const uint32_t j = blockIdx.x;
  U256 acc = u256_zero();
  if (threadIdx.x < nb) acc = u256_from_u64(part + 4 * ((uint64_t)j * VB_PART + threadIdx.x));
  acc = fr_block_sum(sh, acc);
  if (threadIdx.x == 0) u256_to_u64(acc, out + 4 * j);
}

struct Batch {
  pbf_ctx* ctx;
  hipStream_t s;
  const uint64_t* g2;
  size_t count;
  uint64_t *pts, *sc, *e1p, *e1s, *contrib, *part;
  const int* hflag;  // host copy of the per-proof flags (valid after the first MSM's sync)
  int* each;

  // the combined equation over proofs [lo, hi): column sums, two MSMs, one pairing check
  int check(size_t lo, size_t hi, int* ok) {
    const size_t len = hi - lo;
    int rc;
    uint64_t *P = pts, *S = sc;
    if (len != count) {  // a sub-range: its points and scalars, then the shared bases, contiguous
      DevBuf &wp = ctx->buf("vb.wpts"), &ws = ctx->buf("vb.wsc");
      if ((rc = wp.ensure((9 * len + 9) * 64)) || (rc = ws.ensure((9 * len + 9) * 32))) return rc;
      P = (uint64_t*)wp.p;
      S = (uint64_t*)ws.p;
      PBF_HIP(hipMemcpyAsync(P, pts + 72 * lo, 9 * len * 64, hipMemcpyDeviceToDevice, s));
      PBF_HIP(hipMemcpyAsync(P + 72 * len, pts + 72 * count, 9 * 64, hipMemcpyDeviceToDevice, s));
      PBF_HIP(hipMemcpyAsync(S, sc + 36 * lo, 9 * len * 32, hipMemcpyDeviceToDevice, s));
    }
    const uint32_t nb = (uint32_t)std::min<size_t>((len + 255) / 256, VB_PART);
    hipLaunchKernelGGL(k_vb_colsum, dim3(nb, 9), dim3(256), 0, s, (const uint64_t*)contrib, (uint32_t)count,
                       (uint32_t)lo, (uint32_t)hi, part);
    hipLaunchKernelGGL(k_vb_colsum2, dim3(9), dim3(64), 0, s, (const uint64_t*)part, nb, S + 36 * len);
    PBF_HIP(hipGetLastError());
    uint64_t e1[8], e2[8];
    if ((rc = pbf_msm_g1_bn254_dev(ctx, P, S, 9 * len + 9, e2, s))) return rc;
    if ((rc = pbf_msm_g1_bn254_dev(ctx, e1p + 16 * lo, e1s + 4 * E1_N * lo, E1_N * len, e1, s))) return rc;
    return pairing_tail(ctx, e1, e2, g2, ok, s);  // e(sum rho E1, [s]G2) e(-sum rho E2, G2) == 1
  }

  // ok_each over [lo, hi) by halving. failed: the range's equation is already known to fail
  // (its parent failed and its sibling passed: the sums are linear), so it is not run again.
  int localise(size_t lo, size_t hi, bool failed, bool* passed) {
    size_t live = 0;
    for (size_t i = lo; i < hi; ++i) live += hflag[i] == 0;
    *passed = true;
    if (!live) return 0;  // only rejected proofs: every scalar is zero
    int rc, ok = 0;
    if (!failed && (rc = check(lo, hi, &ok))) return rc;
    if (ok) {
      for (size_t i = lo; i < hi; ++i) each[i] = hflag[i] == 0;
      return 0;
    }
    *passed = false;
    if (hi - lo == 1) return 0;  // each[lo] stays 0
    const size_t mid = lo + (hi - lo) / 2;
    bool left = false, right = false;
    if ((rc = localise(lo, mid, false, &left))) return rc;
    return localise(mid, hi, left, &right);
  }
};

// every argument error, before anything is enqueued. chal and u are taken as the single
// verifier takes them (fr_host.hpp hm()): any 256-bit value, reduced mod r. fs: the _fs entries,
// whose chal, u and rho are null (the transcript's kernels write them on the device).
int vb_validate(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies, const uint64_t* srs, size_t srs_m,
                const uint64_t* g2, size_t count, const uint64_t* proof_pts, const uint64_t* proof_f,
                const uint64_t* chal, const uint64_t* u, const uint64_t* rho, const uint64_t* k1k2, int* ok, bool fs) {
  int rc = verifier_shape({ctx, q, copies, srs, g2, proof_pts, proof_f, k1k2}, n, srs_m, ok);
  if (rc) return rc;
  if (!fs && (!chal || !u || !rho)) return fail(PBF_EINVAL, "null argument");
  if (count == 0 || count > ((size_t)1 << 20)) return fail(PBF_EINVAL, "count must be in 1 .. 2^20");
  for (size_t i = 0; !fs && i < count; ++i) {
    const uint64_t* r = rho + 4 * i;
    if (!fr_canonical(r) || !(r[0] | r[1] | r[2] | r[3])) return fail(PBF_EINVAL, "rho must be canonical and nonzero");
  }
  return 0;
}

}  // namespace

// prover.hpp: the public-input fractions of `count` proofs, for both verifiers
int pbf::plonk_pi_fraction_run(pbf_ctx* ctx, const U256& omega, const uint64_t* d_pub, uint64_t npub,
                               const uint64_t* d_chal, uint64_t count, uint64_t* d_nd, hipStream_t s) {
  const uint64_t chunks = (npub + PI_BLK - 1) / PI_BLK;
  if (!chunks || !count) return fail(PBF_EINVAL, "no public input");
  if (chunks >> PI_VBITS || count * chunks > 0x7fffffffull)
    return fail(PBF_EINVAL, "count x npub exceeds one launch of the public-input kernels");
  uint64_t* part = d_nd;  // one chunk: its fraction is the proof's
  if (chunks > 1) {
    DevBuf& pb = ctx->buf("vb.pipart");
    int rc = pb.ensure(count * chunks * 64);
    if (rc) return rc;
    part = (uint64_t*)pb.p;
  }
  PiPow pw;
  const U256 wi = fr_inv(omega);
  pw.step = fr_pow(wi, 64);
  pw.tl[0] = fr_one_m();
  for (int l = 1; l < 64; ++l) pw.tl[l] = Fr::mul(pw.tl[l - 1], wi);
  pw.tv[0] = fr_pow(wi, PI_BLK);
  for (int k = 1; k < PI_VBITS; ++k) pw.tv[k] = Fr::mul(pw.tv[k - 1], pw.tv[k - 1]);
  hipLaunchKernelGGL(k_vb_pi_partial, dim3((uint32_t)(count * chunks)), dim3(64), 0, s, d_pub, d_chal, (uint32_t)npub,
                     (uint32_t)chunks, pw, part);
  if (chunks > 1)
    hipLaunchKernelGGL(k_vb_pi_combine, dim3((uint32_t)count), dim3(64), 0, s, (const uint64_t*)part, (uint32_t)chunks,
                       d_nd);
  PBF_HIP(hipGetLastError());
  return 0;
}

// pub of the _pi verifiers: host values, checked before anything is enqueued
int pbf::plonk_pub_validate(size_t n, const uint64_t* pub, size_t npub, size_t count) {
  if (npub > n) return fail(PBF_EINVAL, "more public inputs than gates");
  if (npub && !pub) return fail(PBF_EINVAL, "null pub with npub > 0");
  if (npub && !fr_canonical(pub, count * npub)) return fail(PBF_EINVAL, "public input not canonical");
  return 0;
}

static int vb_run(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies, const uint64_t* d_srs,
                  size_t srs_m, const uint64_t* g2, size_t count, const uint64_t* proof_pts, const uint64_t* proof_f,
                  const uint64_t* pub, size_t npub, const uint64_t* chal, const uint64_t* u, const uint64_t* rho,
                  const uint64_t* k1k2, int mode, int* ok, int* ok_each, void* stream, bool fs = false) {
  int rc;
  if ((rc = vb_validate(ctx, n, d_q, d_copies, d_srs, srs_m, g2, count, proof_pts, proof_f, chal, u, rho, k1k2, ok, fs)) ||
      (rc = plonk_pub_validate(n, pub, npub, count)) || (fs && (rc = fs_batch_validate(count, npub))))
    return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const PlonkDomain dom = plonk_domain(n);
  uint64_t pre[8][8];
  if ((rc = verifier_vk(ctx, n, dom.omega, d_q, d_copies, d_srs, srs_m, k1k2, s, pre))) return rc;

  const size_t c = count;
  DevBuf &bp = ctx->buf("vb.pts"), &bs = ctx->buf("vb.sc"), &bf = ctx->buf("vb.f"), &bc = ctx->buf("vb.chal"),
         &bu = ctx->buf("vb.u"), &br = ctx->buf("vb.rho"), &bfl = ctx->buf("vb.flag"), &bq = ctx->buf("vb.e1p"),
         &bt = ctx->buf("vb.e1s"), &bk = ctx->buf("vb.contrib"), &bpart = ctx->buf("vb.part");
  if ((rc = bp.ensure((9 * c + 9) * 64)) || (rc = bs.ensure((9 * c + 9) * 32)) || (rc = bf.ensure(7 * c * 32)) ||
      (rc = bc.ensure(5 * c * 32)) || (rc = bu.ensure(c * 32)) || (rc = br.ensure(c * 32)) ||
      (rc = bfl.ensure(c * sizeof(int))) || (rc = bq.ensure(2 * c * 64)) || (rc = bt.ensure(E1_N * c * 32)) ||
      (rc = bk.ensure(9 * c * 32)) || (rc = bpart.ensure(9 * VB_PART * 32)))
    return rc;
  uint64_t* pts = (uint64_t*)bp.p;
  // bases: the proofs' points in place, then q_m q_l q_r q_o q_c s1 s2 s3 and G
  PBF_HIP(hipMemcpyAsync(pts, proof_pts, 9 * c * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(pts + 72 * c, &pre[0][0], 8 * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(pts + 72 * c + 64, d_srs, 64, hipMemcpyDeviceToDevice, s));
  PBF_HIP(hipMemcpyAsync(bf.p, proof_f, 7 * c * 32, hipMemcpyHostToDevice, s));
  DevBuf& bpub = ctx->buf("vb.pub");  // read by the transcript (fs) and by the public-input sums below
  if ((rc = bpub.ensure(c * npub * 32))) return rc;
  if (npub) PBF_HIP(hipMemcpyAsync(bpub.p, pub, c * npub * 32, hipMemcpyHostToDevice, s));
  if (fs) {  // chal, u, rho from the transcript of the proofs and pub just uploaded, never through the host
    uint64_t h0[4];
    fs_circuit_digest(mode, n, npub, k1k2, pre, g2, h0);
    if ((rc = fs_batch_run(ctx, h0, c, (const uint64_t*)pts, (const uint64_t*)bf.p,
                           npub ? (const uint64_t*)bpub.p : nullptr, npub, (uint64_t*)bc.p, (uint64_t*)bu.p,
                           (uint64_t*)br.p, s)))
      return rc;
  } else {
    PBF_HIP(hipMemcpyAsync(bc.p, chal, 5 * c * 32, hipMemcpyHostToDevice, s));
    PBF_HIP(hipMemcpyAsync(bu.p, u, c * 32, hipMemcpyHostToDevice, s));
    PBF_HIP(hipMemcpyAsync(br.p, rho, c * 32, hipMemcpyHostToDevice, s));
  }
  PBF_HIP(hipMemsetAsync(bfl.p, 0, c * sizeof(int), s));
  const VbParams P{hm(k1k2), hm(k1k2 + 4), dom, (uint32_t)c, mode};
  const uint32_t npts = (uint32_t)(9 * c);
  hipLaunchKernelGGL(k_vb_curve, dim3((npts + 255) / 256), dim3(256), 0, s, (const uint64_t*)pts, npts, (int*)bfl.p,
                     (uint64_t*)bq.p);
  if (npub) {  // once per call: localisation reuses the per-proof scalars
    DevBuf& bnd = ctx->buf("vb.pind");
    if ((rc = bnd.ensure(c * 64))) return rc;
    if ((rc = plonk_pi_fraction_run(ctx, dom.omega, (const uint64_t*)bpub.p, npub, (const uint64_t*)bc.p, c,
                                    (uint64_t*)bnd.p, s)))
      return rc;
    hipLaunchKernelGGL(k_vb_scalars<true>, dim3((uint32_t)((c + 63) / 64)), dim3(64), 0, s, (const uint64_t*)bf.p,
                       (const uint64_t*)bc.p, (const uint64_t*)bu.p, (const uint64_t*)br.p, (const uint64_t*)bnd.p, P,
                       (int*)bfl.p, (uint64_t*)bs.p, (uint64_t*)bt.p, (uint64_t*)bk.p);
  } else {
    hipLaunchKernelGGL(k_vb_scalars<false>, dim3((uint32_t)((c + 63) / 64)), dim3(64), 0, s, (const uint64_t*)bf.p,
                       (const uint64_t*)bc.p, (const uint64_t*)bu.p, (const uint64_t*)br.p, (const uint64_t*)nullptr, P,
                       (int*)bfl.p, (uint64_t*)bs.p, (uint64_t*)bt.p, (uint64_t*)bk.p);
  }
  PBF_HIP(hipGetLastError());
  std::vector<int> hflag(c);
  PBF_HIP(hipMemcpyAsync(hflag.data(), bfl.p, c * sizeof(int), hipMemcpyDeviceToHost, s));

  Batch B{ctx, s, g2, c, pts, (uint64_t*)bs.p, (uint64_t*)bq.p, (uint64_t*)bt.p, (uint64_t*)bk.p, (uint64_t*)bpart.p,
          hflag.data(), ok_each};
  int all = 0;
  if ((rc = B.check(0, c, &all))) return rc;  // synchronises s: hflag is complete
  bool rejected = false;
  for (size_t i = 0; i < c; ++i) rejected = rejected || hflag[i] != 0;
  *ok = all && !rejected;
  if (!ok_each) return 0;
  for (size_t i = 0; i < c; ++i) ok_each[i] = all && hflag[i] == 0;
  if (all || c == 1) return 0;
  const size_t mid = c / 2;
  bool left = false, right = false;
  if ((rc = B.localise(0, mid, false, &left))) return rc;
  return B.localise(mid, c, left, &right);
}

// the host forms: every argument error before the uploads
static int vb_host(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies, const uint64_t* srs, size_t srs_m,
                   const uint64_t* g2, size_t count, const uint64_t* proof_pts, const uint64_t* proof_f,
                   const uint64_t* pub, size_t npub, const uint64_t* chal, const uint64_t* u, const uint64_t* rho,
                   const uint64_t* k1k2, int mode, int* ok, int* ok_each, bool fs) {
  int rc;
  if ((rc = vb_validate(ctx, n, q, copies, srs, srs_m, g2, count, proof_pts, proof_f, chal, u, rho, k1k2, ok, fs)) ||
      (rc = plonk_pub_validate(n, pub, npub, count)))
    return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  const uint64_t *d_q, *d_copies, *d_srs;
  if ((rc = verifier_upload(ctx, n, q, copies, srs, srs_m, s, &d_q, &d_copies, &d_srs))) return rc;
  return vb_run(ctx, n, d_q, d_copies, d_srs, srs_m, g2, count, proof_pts, proof_f, pub, npub, chal, u, rho, k1k2, mode, ok,
                ok_each, s, fs);
}

extern "C" int pbf_plonk_verify_bn254_batch_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                                const uint64_t* d_srs, size_t srs_m, const uint64_t* g2, size_t count,
                                                const uint64_t* proof_pts, const uint64_t* proof_f,
                                                const uint64_t* chal, const uint64_t* u, const uint64_t* rho,
                                                const uint64_t* k1k2, int mode, int* ok, int* ok_each, void* stream) {
  return vb_run(ctx, n, d_q, d_copies, d_srs, srs_m, g2, count, proof_pts, proof_f, nullptr, 0, chal, u, rho, k1k2, mode,
                ok, ok_each, stream);
}

extern "C" int pbf_plonk_verify_bn254_batch_pi_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                                   const uint64_t* d_srs, size_t srs_m, const uint64_t* g2, size_t count,
                                                   const uint64_t* proof_pts, const uint64_t* proof_f,
                                                   const uint64_t* pub, size_t npub, const uint64_t* chal,
                                                   const uint64_t* u, const uint64_t* rho, const uint64_t* k1k2, int mode,
                                                   int* ok, int* ok_each, void* stream) {
  return vb_run(ctx, n, d_q, d_copies, d_srs, srs_m, g2, count, proof_pts, proof_f, pub, npub, chal, u, rho, k1k2, mode,
                ok, ok_each, stream);
}

extern "C" int pbf_plonk_verify_bn254_batch(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                            const uint64_t* srs, size_t srs_m, const uint64_t* g2, size_t count,
                                            const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* chal,
                                            const uint64_t* u, const uint64_t* rho, const uint64_t* k1k2, int mode,
                                            int* ok, int* ok_each) {
  return pbf_plonk_verify_bn254_batch_pi(ctx, n, q, copies, srs, srs_m, g2, count, proof_pts, proof_f, nullptr, 0, chal,
                                         u, rho, k1k2, mode, ok, ok_each);
}

extern "C" int pbf_plonk_verify_bn254_batch_pi(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                               const uint64_t* srs, size_t srs_m, const uint64_t* g2, size_t count,
                                               const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* pub,
                                               size_t npub, const uint64_t* chal, const uint64_t* u, const uint64_t* rho,
                                               const uint64_t* k1k2, int mode, int* ok, int* ok_each) {
  return vb_host(ctx, n, q, copies, srs, srs_m, g2, count, proof_pts, proof_f, pub, npub, chal, u, rho, k1k2, mode, ok,
                 ok_each, false);
}

// Fiat-Shamir (pbf.h): no chal, no u, no rho
extern "C" int pbf_plonk_verify_bn254_batch_fs(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                               const uint64_t* srs, size_t srs_m, const uint64_t* g2, size_t count,
                                               const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* pub,
                                               size_t npub, const uint64_t* k1k2, int mode, int* ok, int* ok_each) {
  return vb_host(ctx, n, q, copies, srs, srs_m, g2, count, proof_pts, proof_f, pub, npub, nullptr, nullptr, nullptr, k1k2,
                 mode, ok, ok_each, true);
}

extern "C" int pbf_plonk_verify_bn254_batch_fs_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                                   const uint64_t* d_srs, size_t srs_m, const uint64_t* g2, size_t count,
                                                   const uint64_t* proof_pts, const uint64_t* proof_f,
                                                   const uint64_t* pub, size_t npub, const uint64_t* k1k2, int mode,
                                                   int* ok, int* ok_each, void* stream) {
  return vb_run(ctx, n, d_q, d_copies, d_srs, srs_m, g2, count, proof_pts, proof_f, pub, npub, nullptr, nullptr, nullptr,
                k1k2, mode, ok, ok_each, stream, true);
}
