// Recovery of polynomials from any sufficient set of their KZG cells over BN254 on gfx950
// (include/pbf.h "Recovery from cells"): the erasure decoding of data-availability
// sampling, for a batch of polynomials that share one pattern of missing cells.
//
// Cell i < k = n / l is the l values on {omega^(i + k t) : t < l}, where x^l = c_i = omega^(i l).
// With M the missing cells, Z(x) = prod_{i in M} (x^l - c_i) vanishes on exactly the missing
// points, and R_b, the interpolant of degree < count l of the known values, satisfies
// (E_b Z)(x) = (R_b Z)(x) on all of H = <omega> for E_b = the known values with zero on the missing
// cells; deg R_b Z < n, so the inverse transform of size n of E_b Z is R_b Z exactly. Both R_b Z and
// Z are then taken on the coset g H, divided pointwise and transformed back:
//   k_rec_zvals     Z depends on x only through y = x^l: k values on H (Z(omega^j) is that of
//                   j mod k) and k on g H (y = g^l c_m), formed directly as the product over M,
//                   once per call for the whole batch; the k coset values through the prover's
//                   batch inversion
//   k_rec_scatter   the known cells, cell-major, to E_b Z in natural order, zeros on the missing cells
//   three batched Fr transforms of size n (pbf_ntt_fr256_batch_dev): inverse, forward, inverse
//   k_rec_shift     before the second, the factors g^j that put it on the coset: one launch for the
//                   batch against the context's table of g's powers. The public coset transforms
//                   launch their scaling once per polynomial, which at batch 64 cost nine times the
//                   transform itself (profiles/recover/bench_coset_route.txt), so they are not used
//   k_rec_div       between the last two, the product with 1 / Z at j mod k
//   k_rec_flag      the factors g^-j, the first len coefficients to the caller, and consistent_b =
//                   no coefficient from len on is non-zero
//   out_y           one more forward transform, of what k_rec_flag left in the working array, and
//                   the cell-major store of the cell proofs (kzg_cells.hip cells_ystore_run)
// g = 5: 5^(2^28) != 1 in Fr (tests/test_recover_expect.py), so g^n != 1 for every n <= 2^27, hence
// g^l c_m is no k-th root of unity and Z has no zero on g H whatever is missing.
//
// Conversion-free like the rest of the KZG code: canonical values times Montgomery-form multipliers
// are canonical products. A chain of m products of canonical factors loses R^m, which the chain's
// first operand carries in advance.
#include <cstdio>
#include <ctime>
#include <string>
#include "kzg.hpp"

using namespace pbf;

namespace {

constexpr size_t REC_MAX_K = (size_t)1 << 16, REC_MAX_BATCH = (size_t)1 << 16;
constexpr uint32_t REC_NONE = 0xffffffffu;  // the slot of a missing cell
constexpr uint64_t REC_SHIFT = 5;           // g
constexpr uint32_t REC_LANES = 1u << 16;    // k_rec_zvals splits M until 2k values fill this many lanes

// z[m] = Z at y = c_m in Montgomery form for m < k, z[k + m] = Z at y = g^l c_m canonical: the
// product over the nmiss missing cells of (y - c_i). A workgroup takes 256 >> log_p values of y,
// 2^log_p lanes each; the roots c_i are staged through LDS 256 at a time, a lane multiplies every
// 2^log_p-th of them into its part and the parts are multiplied up through LDS. Each product of
// canonical factors loses one R: start_h = R^(nmiss+1) and start_c = R^nmiss, the first operand of
// part 0, and R in the other parts (one per product that joins them) make up for it.
__global__ void __launch_bounds__(256) k_rec_zvals(const uint64_t* tw, uint64_t n, uint32_t log_l, uint32_t k,
                                                   const uint32_t* miss, uint32_t nmiss, U256 gl, U256 start_h,
                                                   U256 start_c, uint32_t log_p, uint64_t* z) {
  __shared__ U256 sh[256];
  const uint32_t t = threadIdx.x, ys = 256u >> log_p;
  const uint32_t p = t >> (8 - log_p), yi = t & (ys - 1);
  const uint64_t m = (uint64_t)blockIdx.x * ys + yi;
  const bool live = m < 2 * (uint64_t)k;
  U256 y = u256_zero();
  if (live) {
    y = fr_domain_pow(tw, n, (m & (k - 1)) << log_l);
    if (m >= k) y = Fr::mul(gl, y);
  }
  U256 acc = p ? fr_one_m() : (m < k ? start_h : start_c);
  for (uint32_t r0 = 0; r0 < nmiss; r0 += 256) {
    __syncthreads();  // the previous tile's readers are done with sh
    if (r0 + t < nmiss) sh[t] = fr_domain_pow(tw, n, (uint64_t)miss[r0 + t] << log_l);
    __syncthreads();
    const uint32_t cnt = min(256u, nmiss - r0);
    for (uint32_t r = p; r < cnt; r += 1u << log_p) acc = Fr::mul(acc, Fr::sub(y, sh[r]));
  }
  for (uint32_t s = (1u << log_p) >> 1; s; s >>= 1) {
    __syncthreads();
    sh[t] = acc;
    __syncthreads();
    if (p < s) acc = Fr::mul(acc, sh[t + s * ys]);
  }
  if (live && p == 0) u256_to_u64(acc, z + 4 * m);
}

// out[b n + i + k t] = z[i] cells[(b count + slot[i]) l + t], zero where cell i is missing
// (slot[i] = REC_NONE): the inverse of k_cells_ystore over the known cells, times Z on H
__global__ void __launch_bounds__(256) k_rec_scatter(const uint64_t* cells, const uint32_t* slot, const uint64_t* z,
                                                     uint64_t total, uint32_t log_n, uint32_t log_l, uint64_t count,
                                                     uint64_t* out) {
  const uint32_t log_k = log_n - log_l;
  const uint64_t n = (uint64_t)1 << log_n, k = (uint64_t)1 << log_k;
  for (uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (uint64_t)gridDim.x * 256) {
    const uint64_t j = o & (n - 1), b = o >> log_n, i = j & (k - 1), t = j >> log_k;
    const uint32_t s = slot[i];
    U256 v = u256_zero();
    if (s != REC_NONE) v = Fr::mul(u256_from_u64(z + 4 * i), u256_from_u64(cells + 4 * (((b * count + s) << log_l) + t)));
    u256_to_u64(v, out + 4 * o);
  }
}

// a[b n + j] *= zinv[j mod k] (zinv: Montgomery form, as fr_inv_batch_run leaves it)
__global__ void __launch_bounds__(256) k_rec_div(uint64_t* a, const uint64_t* zinv, uint64_t total, uint64_t k) {
  for (uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (uint64_t)gridDim.x * 256)
    u256_to_u64(Fr::mul(u256_from_u64(zinv + 4 * (o & (k - 1))), u256_from_u64(a + 4 * o)), a + 4 * o);
}

// a[b n + j] *= g^j: onto the coset (gtab[i] = g^i in Montgomery form, i <= n)
__global__ void __launch_bounds__(256) k_rec_shift(uint64_t* a, const uint64_t* gtab, uint64_t total, uint64_t n) {
  for (uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (uint64_t)gridDim.x * 256)
    u256_to_u64(Fr::mul(u256_from_u64(gtab + 4 * (o & (n - 1))), u256_from_u64(a + 4 * o)), a + 4 * o);
}

// Back from the coset and out: polys[b pitch + j] = g^(n-j) a[b n + j] for j < len (the missing
// g^-n went into 1 / Z), and consistent[b] (1 before the launch) cleared by a non-zero a[b n + j]
// with j >= len, which needs no factor. From n = 256 on a workgroup lies within one polynomial
// and clears the flag once for its 256 lanes. With keep, a is left holding the polynomials just
// written, zero from len on: the input of the forward transform for out_y.
__global__ void __launch_bounds__(256) k_rec_flag(uint64_t* a, const uint64_t* gtab, uint64_t total, uint32_t log_n,
                                                  uint64_t len, uint64_t pitch, uint64_t* polys, int* consistent,
                                                  int keep) {
  const uint64_t n = (uint64_t)1 << log_n, nblk = (total + 255) / 256;
  for (uint64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const uint64_t o = blk * 256 + threadIdx.x, j = o & (n - 1), b = o >> log_n;
    int nz = 0;
    if (o < total) {
      uint64_t v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = a[4 * o + q];
      if (j < len) {
        const U256 c = Fr::mul(u256_from_u64(gtab + 4 * (n - j)), u256_from_u64(v));
        u256_to_u64(c, polys + 4 * (b * pitch + j));
        if (keep) u256_to_u64(c, a + 4 * o);
      } else {
        nz = (v[0] | v[1] | v[2] | v[3]) != 0;
        if (keep && nz) u256_to_u64(u256_zero(), a + 4 * o);
      }
    }
    if (log_n >= 8) {
      if (__syncthreads_or(nz) && threadIdx.x == 0) atomicAnd(consistent + b, 0);
    } else if (nz) {
      atomicAnd(consistent + b, 0);
    }
  }
}

// option recover.timing = 1: per-stage wall times on stderr (stream synchronised at each mark)
struct RecMarks {
  hipStream_t s;
  bool on;
  double t_last = 0;
  void mark(const char* what) {
    if (!on) return;
    (void)hipStreamSynchronize(s);
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    const double t = ts.tv_sec * 1e3 + ts.tv_nsec / 1e6;
    if (t_last > 0) fprintf(stderr, "[pbf recover] %-28s %9.3f ms\n", what, t - t_last);
    t_last = t;
  }
};

uint32_t rec_grid(uint64_t total) { return (uint32_t)std::min<uint64_t>((total + 255) / 256, (uint64_t)1 << 22); }

struct RecGeom {
  U256 wm;  // omega, Montgomery form
  uint32_t log_n = 0, log_l = 0;
  std::vector<uint32_t> tab;  // slot[i], i < k, then the missing cells
};

// every argument error of the two forms, before anything is enqueued; g.tab from cell_idx
int rec_args(pbf_ctx* ctx, const uint64_t* omega, size_t n, size_t l, size_t len, size_t count,
             const uint64_t* cell_idx, const uint64_t* cells, size_t batch, const uint64_t* out_polys, size_t pitch,
             const int* consistent, RecGeom* g) {
  if (!ctx || !omega || !cell_idx || !cells || !out_polys || !consistent) return fail(PBF_EINVAL, "null argument");
  int rc = kzg_n_check(n);
  if (rc || (rc = kzg_l_check(n, l, &g->log_l))) return rc;
  const size_t k = n / l;
  if (k > REC_MAX_K) return fail(PBF_EINVAL, "n / l must be at most 2^16");
  if ((rc = fr_domain_check(omega, n, &g->wm))) return rc;
  if (len == 0 || len > n) return fail(PBF_EINVAL, "len must be in 1 .. n");
  if (count == 0 || count > k) return fail(PBF_EINVAL, "count must be in 1 .. n / l");
  if (count * l < len) return fail(PBF_EINVAL, "count * l must be at least len");
  if (batch == 0 || batch > REC_MAX_BATCH) return fail(PBF_EINVAL, "batch must be in 1 .. 2^16");
  if (pitch < len) return fail(PBF_EINVAL, "pitch shorter than len");
  if ((rc = kzg_idx_check(cell_idx, count, k))) return rc;
  g->tab.assign(k, REC_NONE);
  for (size_t j = 0; j < count; ++j) {
    const uint64_t i = cell_idx[j];
    if (g->tab[i] != REC_NONE) return fail(PBF_EINVAL, "cell_idx must be distinct");
    g->tab[i] = (uint32_t)j;
  }
  for (size_t i = 0; i < k; ++i)
    if (g->tab[i] == REC_NONE) g->tab.push_back((uint32_t)i);
  while (((size_t)1 << g->log_n) < n) ++g->log_n;
  return 0;
}

// gtab[i] = g^i in Montgomery form, i <= n: the context's table of the coset shift for this n,
// built once on s by fr_powers_run (one stream sync, as fr_domain_table) and kept with the context.
// One launch scales a whole batch by it, where the public coset transforms launch their scaling
// once per polynomial.
int rec_shift_table(pbf_ctx* ctx, uint32_t log_n, hipStream_t s, const uint64_t** gtab) {
  DevBuf& b = ctx->buf("kzg.rec.g" + std::to_string(log_n));
  if (!b.p) {
    const uint64_t entries = ((uint64_t)1 << log_n) + 1;
    int rc = b.ensure(entries * 32);
    // start = R as a field element: the canonical R g^i is the Montgomery form of g^i
    if (!rc) rc = fr_powers_run((uint64_t*)b.p, entries, hm64(REC_SHIFT), Fr::to_mont(fr_one_m()), s);
    if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = fail(3 /*PBF_EDEVICE*/, "hipStreamSynchronize");
    if (rc) {
      b.release();
      return rc;
    }
  }
  *gtab = (const uint64_t*)b.p;
  return 0;
}

// the call past its argument checks, everything on s
int rec_run(pbf_ctx* ctx, const RecGeom& g, size_t n, size_t l, size_t len, size_t count, const uint64_t* d_cells,
            size_t batch, uint64_t* d_polys, size_t pitch, uint64_t* d_out_y, int* d_consistent, hipStream_t s) {
  const uint64_t k = n / l, total = (uint64_t)batch * n;
  const uint32_t nmiss = (uint32_t)(k - count);
  DevBuf &ba = ctx->buf("kzg.rec.a"), &bz = ctx->buf("kzg.rec.z"), &bt = ctx->buf("kzg.rec.tab");
  int rc;
  if ((rc = ba.ensure(total * 32)) || (rc = bz.ensure(2 * k * 32 + sizeof(int))) || (rc = bt.ensure(2 * k * 4))) return rc;
  const uint64_t* tw = nullptr;
  if (n > 1 && (rc = fr_domain_table(ctx, g.wm, n, s, &tw))) return rc;
  const uint64_t* gtab = nullptr;
  if ((rc = rec_shift_table(ctx, g.log_n, s, &gtab))) return rc;
  uint64_t *a = (uint64_t*)ba.p, *z = (uint64_t*)bz.p, *zc = z + 4 * k;
  // never set: g^n != 1, so Z has no zero on the coset and the inversion meets none
  int* bad = (int*)(z + 8 * k);
  uint32_t *slot = (uint32_t*)bt.p, *miss = slot + k;
  RecMarks tm{s, ctx->options.num("recover.timing", 0) != 0};
  tm.mark("start");
  // pageable memory: the copy has read g.tab when the call returns
  PBF_HIP(hipMemcpyAsync(slot, g.tab.data(), g.tab.size() * 4, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemsetD32Async((hipDeviceptr_t)d_consistent, 1, batch, s));
  // Z on H and on g H, once for the batch; 1 / Z on the coset
  uint32_t log_p = 0;
  while (log_p < 8 && ((2 * k) << log_p) < REC_LANES && (2u << log_p) <= nmiss) ++log_p;
  // the coset's values carry g^n, so that 1 / Z carries the g^-n that k_rec_flag's factors g^(n-j) lack
  const U256 gm = hm64(REC_SHIFT), start_h = fr_pow(Fr::to_mont(fr_one_m()), nmiss);
  const U256 start_c = Fr::mul(Fr::from_mont(start_h), fr_pow(gm, n));
  const uint32_t ys = 256u >> log_p;
  hipLaunchKernelGGL(k_rec_zvals, dim3((uint32_t)((2 * k + ys - 1) / ys)), dim3(256), 0, s, tw, (uint64_t)n, g.log_l,
                     (uint32_t)k, (const uint32_t*)miss, nmiss, fr_pow(gm, l), start_h, start_c, log_p, z);
  PBF_HIP(hipGetLastError());
  if ((rc = fr_inv_batch_run(ctx, zc, zc, k, bad, s))) return rc;
  tm.mark("Z values and inversion");
  hipLaunchKernelGGL(k_rec_scatter, dim3(rec_grid(total)), dim3(256), 0, s, d_cells, (const uint32_t*)slot,
                     (const uint64_t*)z, total, g.log_n, g.log_l, (uint64_t)count, a);
  PBF_HIP(hipGetLastError());
  tm.mark("scatter");
  uint64_t om[4];
  hout(om, g.wm);
  if ((rc = pbf_ntt_fr256_batch_dev(ctx, om, a, a, n, batch, 1, s))) return rc;
  tm.mark("inverse transform");
  hipLaunchKernelGGL(k_rec_shift, dim3(rec_grid(total)), dim3(256), 0, s, a, gtab, total, (uint64_t)n);
  PBF_HIP(hipGetLastError());
  if ((rc = pbf_ntt_fr256_batch_dev(ctx, om, a, a, n, batch, 0, s))) return rc;
  tm.mark("shift and coset transform");
  hipLaunchKernelGGL(k_rec_div, dim3(rec_grid(total)), dim3(256), 0, s, a, (const uint64_t*)zc, total, k);
  PBF_HIP(hipGetLastError());
  tm.mark("division");
  if ((rc = pbf_ntt_fr256_batch_dev(ctx, om, a, a, n, batch, 1, s))) return rc;
  tm.mark("inverse coset transform");
  hipLaunchKernelGGL(k_rec_flag, dim3(rec_grid(total)), dim3(256), 0, s, a, gtab, total, g.log_n, (uint64_t)len,
                     (uint64_t)pitch, d_polys, d_consistent, d_out_y ? 1 : 0);
  PBF_HIP(hipGetLastError());
  tm.mark("shift back, flag and copy-out");
  if (!d_out_y) return PBF_OK;
  // every cell of the polynomials just written, which k_rec_flag left in the working array, in the
  // order of pbf_kzg_open_cells_bn254_dev's out_y (l = 1 and l = n: the transform's own order)
  const bool direct = l == 1 || k == 1;
  uint64_t* y = direct ? d_out_y : a;
  if ((rc = pbf_ntt_fr256_batch_dev(ctx, om, a, y, n, batch, 0, s))) return rc;
  if (!direct && (rc = cells_ystore_run(y, batch, k, g.log_l, d_out_y, s))) return rc;
  tm.mark("out_y");
  return PBF_OK;
}

}  // namespace

extern "C" int pbf_kzg_recover_cells_bn254_dev(pbf_ctx* ctx, const uint64_t* omega, size_t n, size_t l, size_t len,
                                               size_t count, const uint64_t* cell_idx, const uint64_t* d_cells,
                                               size_t batch, uint64_t* d_out_polys, size_t pitch, uint64_t* d_out_y,
                                               int* d_consistent, void* stream) {
  RecGeom g;
  int rc = rec_args(ctx, omega, n, l, len, count, cell_idx, d_cells, batch, d_out_polys, pitch, d_consistent, &g);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  return rec_run(ctx, g, n, l, len, count, d_cells, batch, d_out_polys, pitch, d_out_y, d_consistent,
                 (hipStream_t)stream);
}

extern "C" int pbf_kzg_recover_cells_bn254(pbf_ctx* ctx, const uint64_t* omega, size_t n, size_t l, size_t len,
                                           size_t count, const uint64_t* cell_idx, const uint64_t* cells, size_t batch,
                                           uint64_t* out_polys, size_t pitch, uint64_t* out_y, int* consistent) {
  RecGeom g;
  int rc = rec_args(ctx, omega, n, l, len, count, cell_idx, cells, batch, out_polys, pitch, consistent, &g);
  if (rc) return rc;
  const size_t vals = batch * count * l;
  if (!fr_canonical(cells, vals)) return fail(PBF_EINVAL, "cells must be canonical");
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  DevBuf &bc = ctx->buf("kzg.rec.cells"), &bp = ctx->buf("kzg.rec.polys"), &by = ctx->buf("kzg.rec.y"),
         &bf = ctx->buf("kzg.rec.flag");
  if ((rc = bc.ensure(vals * 32)) || (rc = bp.ensure(batch * len * 32)) || (rc = bf.ensure(batch * sizeof(int))) ||
      (out_y && (rc = by.ensure(batch * n * 32))))
    return rc;
  PBF_HIP(hipMemcpyAsync(bc.p, cells, vals * 32, hipMemcpyHostToDevice, s));
  if ((rc = rec_run(ctx, g, n, l, len, count, (const uint64_t*)bc.p, batch, (uint64_t*)bp.p, len,
                    out_y ? (uint64_t*)by.p : nullptr, (int*)bf.p, s)))
    return rc;
  PBF_HIP(hipMemcpy2DAsync(out_polys, pitch * 32, bp.p, len * 32, len * 32, batch, hipMemcpyDeviceToHost, s));
  if (out_y) PBF_HIP(hipMemcpyAsync(out_y, by.p, batch * n * 32, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipMemcpyAsync(consistent, bf.p, batch * sizeof(int), hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  return PBF_OK;
}
