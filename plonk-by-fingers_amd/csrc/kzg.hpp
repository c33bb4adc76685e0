// What the KZG units share (kzg.hip, kzg_multi.hip, kzg_evals.hip, kzg_cells.hip, kzg_recover.hip):
// one statement of every step that more than one scheme takes, inline; only cells_ystore_run and
// kzg_vsum_run cross units.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../include/pbf.h"
#include "g1_win.hpp"

namespace pbf {

// ---------------------------------------------------------------- argument checks and upload
// every argument error of commit / open, before anything is enqueued
inline int poly_args(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* polys, size_t len, size_t pitch,
                     size_t batch, size_t need) {
  if (!ctx || !srs || !polys) return fail(PBF_EINVAL, "null argument");
  if (len == 0) return fail(PBF_EINVAL, "len must be at least 1");
  if (batch == 0 || batch > ((size_t)1 << 16)) return fail(PBF_EINVAL, "batch must be in 1 .. 2^16");
  if (pitch < len) return fail(PBF_EINVAL, "pitch shorter than len");
  if (srs_m < need) return fail(PBF_EINVAL, "SRS too short");
  return 0;
}
inline int open_args(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* polys, size_t len, size_t pitch,
                     size_t batch, const uint64_t* z, const uint64_t* weights, const uint64_t* out_y,
                     const uint64_t* out_w) {
  if (!z || !weights || !out_y || !out_w) return fail(PBF_EINVAL, "null argument");
  int rc = poly_args(ctx, srs, srs_m, polys, len, pitch, batch, len ? len - 1 : 0);
  if (rc) return rc;
  if (!fr_canonical(z)) return fail(PBF_EINVAL, "z must be canonical");
  if (!fr_canonical(weights, batch)) return fail(PBF_EINVAL, "weights must be canonical");
  return 0;
}

// the polynomials of a host-pointer call on the device, compact (pitch = len)
inline int upload_polys(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* polys, size_t len,
                        size_t pitch, size_t batch, hipStream_t s) {
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

// ---------------------------------------------------------------- the weighted sum of a batch
// comb = sum_b c_b p_b on len coefficients over the `batch` polynomials p_b = poly(b) (c: Montgomery
// form): 10 inputs per launch, later launches taking the sum so far as one of them
template <class PolyAt>
inline int kzg_comb_of(PolyAt poly, uint64_t len, uint64_t batch, const U256* c, uint64_t* comb, hipStream_t s) {
  int rc;
  for (uint64_t b0 = 0; b0 < batch;) {
    const uint64_t* in[10];
    const uint64_t lens[10] = {len, len, len, len, len, len, len, len, len, len};
    U256 ck[10];
    int k = 0;
    if (b0) {  // the sum so far
      in[k] = comb;
      ck[k++] = fr_one_m();
    }
    while (k < 10 && b0 < batch) {
      in[k] = poly(b0);
      ck[k++] = c[b0++];
    }
    if ((rc = fr_lincomb_run(k, in, lens, ck, u256_zero(), comb, len, s))) return rc;
  }
  return 0;
}
// the same over a whole batch, p_b at d_polys + 4 b pitch
inline int kzg_comb(const uint64_t* d_polys, uint64_t len, uint64_t pitch, uint64_t batch, const U256* c,
                    uint64_t* comb, hipStream_t s) {
  return kzg_comb_of([=](uint64_t b) { return d_polys + 4 * b * pitch; }, len, batch, c, comb, s);
}

// ---------------------------------------------------------------- geometry of the cells
constexpr size_t KZG_MAX_N = (size_t)1 << 27;  // 2n stays within the 2-adicity of Fr

inline int kzg_n_check(size_t n) {
  if (n == 0 || (n & (n - 1)) || n > KZG_MAX_N) return fail(PBF_EINVAL, "n must be a power of two in 1 .. 2^27");
  return 0;
}
// l a power of two in 1 .. n; *log_l
inline int kzg_l_check(size_t n, size_t l, uint32_t* log_l) {
  if (l == 0 || (l & (l - 1)) || l > n) return fail(PBF_EINVAL, "l must be a power of two in 1 .. n");
  *log_l = 0;
  while (((size_t)1 << *log_l) < l) ++*log_l;
  return 0;
}
inline int kzg_idx_check(const uint64_t* cell_idx, size_t count, size_t k) {
  for (size_t i = 0; i < count; ++i)
    if (cell_idx[i] >= k) return fail(PBF_EINVAL, "cell_idx must be below n / l");
  return 0;
}

// omega^e canonical, e < n, from the domain table of (omega, n); n = 1 has no table
__device__ __forceinline__ U256 fr_domain_pow(const uint64_t* tw, uint64_t n, uint64_t e) {
  return n > 1 ? fr_domain_at(tw, n, e) : Fr::one_plain();
}

// kzg_cells.hip: the cell-major store of the cell proofs, shared with the recovery:
// out[(b k + i) l + t] = y[b n + i + k t] for `batch` transforms of size n = k l (k_cells_ystore)
int cells_ystore_run(const uint64_t* y, uint64_t batch, uint64_t k, uint32_t log_l, uint64_t* out, hipStream_t s);

// kzg.hip: *out = -(sum of the nparts partial sums at part), the scalar of G of the verifiers of
// kzg.hip and kzg_multi.hip (k_kzg_vsum)
int kzg_vsum_run(const uint64_t* part, uint32_t nparts, uint64_t* out, hipStream_t s);

// ---------------------------------------------------------------- the batched verifiers
// All check e(sum rho_i W_i, g2[1]) e(-(sum of sc pts), g2[0]) == 1 on the context's kzg.v.*
// buffers. The single-point ones keep pts = [C_0.. | W_0.. | `extra` shared bases] and differ in
// the scalars sc only; the multi-point one has more points per opening and says where its W are.
struct KzgVerify {
  uint64_t *in, *pts, *sc, *part;
  int* flag;
};
// in_words u64 of inputs (C, then W, first), 2 c + extra points and scalars, `parts` partial sums
inline int kzg_verify_bufs(pbf_ctx* ctx, size_t c, size_t extra, size_t in_words, size_t parts, KzgVerify* v) {
  DevBuf &bi = ctx->buf("kzg.v.in"), &bp = ctx->buf("kzg.v.pts"), &bs = ctx->buf("kzg.v.sc"),
         &bpart = ctx->buf("kzg.v.part"), &bfl = ctx->buf("kzg.v.flag");
  int rc;
  if ((rc = bi.ensure(in_words * 8)) || (rc = bp.ensure((2 * c + extra) * 64)) ||
      (rc = bs.ensure((2 * c + extra) * 32)) || (rc = bpart.ensure(parts * 32)) || (rc = bfl.ensure(sizeof(int))))
    return rc;
  *v = {(uint64_t*)bi.p, (uint64_t*)bp.p, (uint64_t*)bs.p, (uint64_t*)bpart.p, (int*)bfl.p};
  return 0;
}
inline int kzg_rho_check(const uint64_t* rho, size_t count) {
  for (size_t i = 0; i < count; ++i) {
    const uint64_t* r = rho + 4 * i;
    if (!fr_canonical(r) || !(r[0] | r[1] | r[2] | r[3])) return fail(PBF_EINVAL, "rho must be canonical and nonzero");
  }
  return 0;
}
// C and W to the head of v.in, rho to d_rho (within v.in, where the scheme keeps it)
inline int kzg_verify_upload(const KzgVerify& v, size_t c, const uint64_t* commits, const uint64_t* w,
                             const uint64_t* rho, uint64_t* d_rho, hipStream_t s) {
  PBF_HIP(hipMemcpyAsync(v.in, commits, c * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(v.in + 8 * c, w, c * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(d_rho, rho, c * 32, hipMemcpyHostToDevice, s));
  return 0;
}
// entry i < count of the per-entry kernels: C_i and W_i into pts, *flag set by either being not
// canonical or not on the curve
__device__ __forceinline__ void kzg_vpoints(const uint64_t* commits, const uint64_t* w, uint32_t count, uint32_t i,
                                            uint64_t* pts, int* flag) {
  const uint64_t *c = commits + 8 * (uint64_t)i, *wi = w + 8 * (uint64_t)i;
  if (g1_bad(c) || g1_bad(wi)) atomicOr(flag, 1);
  uint64_t *pc = pts + 8 * (uint64_t)i, *pw = pts + 8 * ((uint64_t)count + i);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    pc[k] = c[k];
    pw[k] = wi[k];
  }
}
// After the scheme's kernels: a flagged point gives *ok = 0 (set by the caller) and PBF_OK; else
// the MSM over the c points w_pts with the scalars w_sc (sum rho_i W_i), the MSM over all `total`
// points of v.pts with v.sc, one pairing check.
inline int kzg_verify_tail_at(pbf_ctx* ctx, const KzgVerify& v, const uint64_t* w_pts, const uint64_t* w_sc, size_t c,
                              size_t total, const uint64_t* g2, int* ok, hipStream_t s) {
  PBF_HIP(hipGetLastError());
  int bad = 0, rc;
  PBF_HIP(hipMemcpyAsync(&bad, v.flag, sizeof(int), hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  if (bad) return PBF_OK;
  uint64_t e1[8], e2[8];
  if ((rc = pbf_msm_g1_bn254_dev(ctx, w_pts, w_sc, c, e1, s))) return rc;  // sum rho_i W_i
  if ((rc = pbf_msm_g1_bn254_dev(ctx, v.pts, v.sc, total, e2, s))) return rc;
  return pairing_tail(ctx, e1, e2, g2, ok, s);  // g2[1]: [s]G2, or [s^l]G2 for cells
}
// the layout [C | W | extra]: the W half carries rho at the head of sc
inline int kzg_verify_tail(pbf_ctx* ctx, const KzgVerify& v, size_t c, size_t extra, const uint64_t* g2, int* ok,
                           hipStream_t s) {
  return kzg_verify_tail_at(ctx, v, v.pts + 8 * c, v.sc, c, 2 * c + extra, g2, ok, s);
}

}  // namespace pbf
