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
//   verify   e(sum rho_i W_i, [s]G2) e(-sum rho_i (C_i - y_i G + z_i W_i), G2) == 1: one MSM over
//            count points, one over 2 count + 1, one pairing check
// The opening from evaluations (kzg_evals.hip), FK20 and the cell proofs (kzg_cells.hip) and the
// recovery from cells (kzg_recover.hip) are units of their own; kzg.hpp holds what they share.
//
// Everything is conversion-free where it touches coefficients: canonical values times
// Montgomery-form multipliers (z, its powers, the weights) are canonical products.
#include "kzg.hpp"

using namespace pbf;

namespace {

// ---------------------------------------------------------------- the opening's sweeps
// y (device, batch x 4) and the quotient's len - 1 coefficients in q. Evaluations: 12 polynomials
// per launch; the weighted sum (kzg_comb; w: Montgomery form); then one division.
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
  if ((rc = kzg_comb(d_polys, len, pitch, batch, w.data(), comb, s))) return rc;
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
    kzg_vpoints(commits, w, count, i, pts, flag);
    const U256 r = u256_from_u64(rho + 4 * (uint64_t)i), rm = Fr::to_mont(r);
    u256_to_u64(r, sc + 4 * (uint64_t)i);
    u256_to_u64(Fr::mul(rm, u256_from_u64(z + 4 * (uint64_t)i)), sc + 4 * ((uint64_t)count + i));
    ry = Fr::mul(rm, u256_from_u64(y + 4 * (uint64_t)i));
  }
  const U256 sum = fr_block_sum(sh, ry);
  if (threadIdx.x == 0) u256_to_u64(sum, part + 4 * (uint64_t)blockIdx.x);
}
// sc[2 count] = -(sum of the nparts partial sums): the scalar of G; one workgroup
__global__ void __launch_bounds__(256) k_kzg_vsum(const uint64_t* part, uint32_t nparts, uint64_t* out) {
  __shared__ U256 sh[256];
  U256 acc = u256_zero();
  for (uint32_t i = threadIdx.x; i < nparts; i += 256) acc = Fr::add(acc, u256_from_u64(part + 4 * (uint64_t)i));
  const U256 sum = fr_block_sum(sh, acc);
  if (threadIdx.x == 0) u256_to_u64(Fr::sub(u256_zero(), sum), out);
}

}  // namespace

int pbf::kzg_vsum_run(const uint64_t* part, uint32_t nparts, uint64_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_kzg_vsum, dim3(1), dim3(256), 0, s, part, nparts, out);
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
  if ((rc = open_sweeps(ctx, d_polys, len, pitch, batch, zm, w, q, d_y, s))) return rc;
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
  int rc = kzg_rho_check(rho, count);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  const size_t c = count;
  const uint32_t nparts = (uint32_t)((c + 255) / 256);
  // inputs: commits, w (8 words each), z, y, rho (4 each) per entry
  KzgVerify v;
  if ((rc = kzg_verify_bufs(ctx, c, 1, c * 28, nparts, &v))) return rc;
  uint64_t *d_z = v.in + 16 * c, *d_y = v.in + 20 * c, *d_rho = v.in + 24 * c;
  if ((rc = kzg_verify_upload(v, c, commits, w, rho, d_rho, s))) return rc;
  PBF_HIP(hipMemcpyAsync(d_z, z, c * 32, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(d_y, y, c * 32, hipMemcpyHostToDevice, s));
  static const uint64_t G1_GEN[8] = {1, 0, 0, 0, 2, 0, 0, 0};
  PBF_HIP(hipMemcpyAsync(v.pts + 16 * c, G1_GEN, 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemsetAsync(v.flag, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_kzg_vprep, dim3(nparts), dim3(256), 0, s, (const uint64_t*)v.in, (const uint64_t*)(v.in + 8 * c),
                     (const uint64_t*)d_z, (const uint64_t*)d_y, (const uint64_t*)d_rho, (uint32_t)c, v.pts, v.sc, v.part,
                     v.flag);
  if ((rc = kzg_vsum_run(v.part, nparts, v.sc + 8 * c, s))) return rc;
  // e(sum rho W, [s]G2) e(-sum rho (C - y G + z W), G2) == 1
  return kzg_verify_tail(ctx, v, c, 1, g2, ok, s);
}
