// KZG openings from evaluations over BN254 on gfx950 (include/pbf.h "KZG in evaluation form";
// DESIGN.md 3.10): the (y, W) of kzg.hip's opening from the polynomials' values on H = <omega>
// against the Lagrange-basis SRS (g1_ntt.hip). Denominators omega^i - z, the prover's batch
// inversion, a barycentric dot product per polynomial, the pointwise quotient, one MSM; z = omega^k
// is handled on the device and is no failing case either. All canonical values times Montgomery
// multipliers, as in kzg.hip.
#include "kzg.hpp"

using namespace pbf;

namespace {

constexpr int EVD_G = 8;  // polynomials per dot-product launch: omega^i u_i is formed once for them

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
    const U256 sum = fr_block_sum(sh, v);
    if (threadIdx.x == 0) u256_to_u64(sum, part + 4 * ((b0 + b) * gridDim.x + blockIdx.x));
  }
}
// y[b] = factor * (the sum of polynomial b's nblk partial sums); one workgroup per polynomial
__global__ void __launch_bounds__(256) k_ev_ysum(const uint64_t* part, uint64_t nblk, U256 factor, uint64_t* y) {
  __shared__ U256 sh[256];
  const uint64_t b = blockIdx.x;
  U256 acc = u256_zero();
  for (uint64_t i = threadIdx.x; i < nblk; i += 256) acc = Fr::add(acc, u256_from_u64(part + 4 * (b * nblk + i)));
  const U256 sum = fr_block_sum(sh, acc);
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
  const U256 sum = fr_block_sum(sh, acc);
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
  const U256 sum = fr_block_sum(sh, v);
  if (threadIdx.x == 0) u256_to_u64(sum, part + 4 * (uint64_t)blockIdx.x);
}
// q[k] = -omega^-k (the sum of the nblk partial sums); one workgroup
__global__ void __launch_bounds__(256) k_ev_qk(const uint64_t* part, uint64_t nblk, const uint64_t* tw, uint64_t n,
                                               const uint64_t* kidx, uint64_t* q) {
  __shared__ U256 sh[256];
  U256 acc = u256_zero();
  for (uint64_t i = threadIdx.x; i < nblk; i += 256) acc = Fr::add(acc, u256_from_u64(part + 4 * i));
  const U256 sum = fr_block_sum(sh, acc);
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
  if ((rc = kzg_comb(d_evals, n, pitch, batch, w.data(), comb, s))) return rc;  // c = sum_b w_b p_b
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

}  // namespace

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
