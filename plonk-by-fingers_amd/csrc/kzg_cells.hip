// Every KZG opening on a domain at once over BN254 on gfx950 (include/pbf.h "Every opening at
// once", "KZG cell proofs"): FK20 and, over cosets of l points, the cell proofs of
// data-availability sampling with their batched verifier. The sections below say
// how; the verifier's kernels run between the head and the tail that kzg.hpp gives both verifiers.
#include "kzg.hpp"

using namespace pbf;

namespace {

// ---------------------------------------------------------------- every opening at once (FK20)
// W_(omega^i) = sum_m omega^(im) h_m with h_m = sum_k p_(m+1+k) srs[k]: h is the upper half of
// the convolution of a_t = srs[n - 2 - t] with p, taken in a cyclic convolution of size 2n that
// does not wrap. xext, the size-2n G1 NTT of a, is the setup; a call is one
// size-2n Fr NTT, 2n pointwise products, the size-2n inverse G1 NTT and the size-n forward one,
// the last three without leaving Xyzz (g1_mul.hip, g1_ntt.hip).

// a_t = srs[n - 2 - t] for t <= n - 2 and the identity (0, 0) for n - 1 <= t < 2n
__global__ void __launch_bounds__(256) k_fk20_a(const uint64_t* srs, uint64_t n, uint64_t* a) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * n) return;
#pragma unroll
  for (int k = 0; k < 8; ++k) a[8 * t + k] = t + 2 <= n ? srs[8 * (n - 2 - t) + k] : 0;
}

// n a power of two in 1 .. 2^27 and omega2 canonical of order exactly 2n; *w2m = omega2 (Montgomery)
int fk20_domain(size_t n, const uint64_t* omega2, U256* w2m) {
  int rc = kzg_n_check(n);
  return rc ? rc : fr_domain_check(omega2, 2 * n, w2m);
}
int fk20_setup_args(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* omega2, size_t n,
                    const uint64_t* xext, U256* w2m) {
  if (!ctx || !srs || !omega2 || !xext) return fail(PBF_EINVAL, "null argument");
  int rc = fk20_domain(n, omega2, w2m);
  if (rc) return rc;
  if (srs_m + 1 < n) return fail(PBF_EINVAL, "SRS too short");
  return 0;
}
// what the multi-openings check of xext, the domain and the polynomials; the weighted ones add the weights
int fk20_polys_args(pbf_ctx* ctx, const uint64_t* xext, size_t n, const uint64_t* omega2, const uint64_t* polys,
                    size_t len, size_t pitch, size_t batch, const uint64_t* out_w, U256* w2m) {
  if (!omega2 || !out_w) return fail(PBF_EINVAL, "null argument");
  int rc = poly_args(ctx, xext, 0, polys, len, pitch, batch, 0);
  if (rc) return rc;
  if ((rc = fk20_domain(n, omega2, w2m))) return rc;
  if (len > n) return fail(PBF_EINVAL, "len exceeds n");
  return 0;
}
int fk20_open_args(pbf_ctx* ctx, const uint64_t* xext, size_t n, const uint64_t* omega2, const uint64_t* polys,
                   size_t len, size_t pitch, size_t batch, const uint64_t* weights, const uint64_t* out_w, U256* w2m) {
  if (!weights) return fail(PBF_EINVAL, "null argument");
  int rc = fk20_polys_args(ctx, xext, n, omega2, polys, len, pitch, batch, out_w, w2m);
  if (rc) return rc;
  if (!fr_canonical(weights, batch)) return fail(PBF_EINVAL, "weights must be canonical");
  return 0;
}

// kzg_comb's coefficients: the canonical weights times scale, the inverse transform's factor
std::vector<U256> scaled_weights(const uint64_t* weights, size_t batch, const U256& scale) {
  std::vector<U256> c(batch);
  for (size_t b = 0; b < batch; ++b) c[b] = Fr::mul(hm(weights + 4 * b), scale);
  return c;
}

// y[b n + i] = p_b(omega^i): the size-n Fr NTT of every polynomial, zero-padded from len (om:
// omega, canonical); out_y of open_all, and of open_cells before its cell-major store
int polys_ntt(pbf_ctx* ctx, const uint64_t* om, const uint64_t* d_polys, size_t len, size_t pitch, size_t batch,
              size_t n, uint64_t* y, hipStream_t s) {
  const uint64_t one[4] = {1, 0, 0, 0};
  int rc;
  if (n == 1) {
    PBF_HIP(hipMemcpy2DAsync(y, 32, d_polys, pitch * 32, 32, batch, hipMemcpyDeviceToDevice, s));
  } else if (pitch == len) {
    return pbf_ntt_fr256_coset_batch_dev(ctx, om, one, d_polys, len, y, n, batch, 0, s);
  } else {
    for (size_t b = 0; b < batch; ++b)
      if ((rc = pbf_ntt_fr256_coset_batch_dev(ctx, om, one, d_polys + 4 * b * pitch, len, y + 4 * b * n, n, 1, 0, s)))
        return rc;
  }
  return 0;
}

// The host-pointer form of a setup past its argument checks: the `used` points of the SRS that it
// reads uploaded and checked, dev(d_srs, d_xext, s) the _dev form, the 2n points of xext back.
template <class Dev>
int setup_host(pbf_ctx* ctx, const uint64_t* srs, size_t used, size_t n, uint64_t* xext, const Dev& dev) {
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  DevBuf &ds = ctx->buf("kzg.srs"), &dx = ctx->buf("kzg.fk20.xext");
  int rc;
  if ((rc = ds.ensure(std::max<size_t>(used, 1) * 64)) || (rc = dx.ensure(2 * n * 64))) return rc;
  if (used) {
    PBF_HIP(hipMemcpyAsync(ds.p, srs, used * 64, hipMemcpyHostToDevice, s));
    int bad = 0;
    if ((rc = g1_check_run(ctx, (const uint64_t*)ds.p, used, s, &bad))) return rc;
    if (bad) return fail(PBF_EINVAL, "a point is not canonical or not on the curve");
  }
  if ((rc = dev((const uint64_t*)ds.p, (uint64_t*)dx.p, s))) return rc;
  PBF_HIP(hipMemcpyAsync(xext, dx.p, 2 * n * 64, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  return PBF_OK;
}
// The same of a multi-opening: xext and the polynomials (compact) uploaded,
// dev(d_xext, d_polys, d_y or null, d_w, s) the _dev form, batch x n values and nw proofs back.
template <class Dev>
int open_host(pbf_ctx* ctx, const uint64_t* xext, size_t n, const uint64_t* polys, size_t len, size_t pitch,
              size_t batch, uint64_t* out_y, uint64_t* out_w, size_t nw, const Dev& dev) {
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  int rc;
  if ((rc = upload_polys(ctx, xext, 2 * n, polys, len, pitch, batch, s))) return rc;
  DevBuf &by = ctx->buf("kzg.fk20.y"), &bw = ctx->buf("kzg.fk20.w");
  if ((out_y && (rc = by.ensure(batch * n * 32))) || (rc = bw.ensure(nw * 64))) return rc;
  if ((rc = dev((const uint64_t*)ctx->buf("kzg.srs").p, (const uint64_t*)ctx->buf("kzg.polys").p,
                out_y ? (uint64_t*)by.p : nullptr, (uint64_t*)bw.p, s)))
    return rc;
  if (out_y) PBF_HIP(hipMemcpyAsync(out_y, by.p, batch * n * 32, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipMemcpyAsync(out_w, bw.p, nw * 64, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  return PBF_OK;
}

// ---------------------------------------------------------------- cell proofs (FK20 over cosets)
// Cell i < k = n / l is the coset {omega^(i + k t) : t < l}, on which x^l = c_i = omega^(i l);
// W_i = [q_i(s)]G for p = q_i (x^l - c_i) + I_i. W = sum_m c_i^m h_m is the forward G1 NTT of size
// k, root omega^l, of h_m = sum_{r<l} (a_r * b_r)_(k-1+m): l convolutions of the shape above at
// size 2k, a_r[t] = srs[r + l (k-2-t)], b_r[u] = p_(r + l u). xext holds the l
// transforms of the a_r slab after slab; a call multiplies all 2n points as one vector, sums the
// l products of every frequency and runs the two transforms at sizes 2k and k.
//
// The proofs of each of B polynomials (pbf_kzg_open_cells_each_bn254*) are the
// same steps with every vector B times as long, and the weighted call is B = 1 of them on the
// combination c (cells_proofs): the B x 2n products run as ONE vector over the same xext, so a
// launch is as wide as the tile whatever 2n is and takes polynomials' products together or splits
// one polynomial's between two launches; their sums, B x 2k, lie behind them; the transforms of
// sizes 2k and k are the batched G1 NTT (g1_ntt.hip) over B transforms, the size-k ones at the
// pitch 2k that k_g1_slice leaves them at. Scratch: B x (2n + 2k) points.
constexpr size_t CELLS_MAX_COUNT = (size_t)1 << 20, CELLS_MAX_VALUES = (size_t)1 << 22;
constexpr size_t CELLS_EACH_MAX = (size_t)1 << 24;  // batch * n of one call: 4 GiB of products
constexpr int CV_CH = 32;  // entries per lane of the verifier's sweep

// a[r 2k + t] = srs[r + l (k-2-t)] for t <= k-2 and the identity (0, 0) for k-1 <= t < 2k, r < l
__global__ void __launch_bounds__(256) k_cells_a(const uint64_t* srs, uint64_t k, uint32_t log_l, uint64_t* a) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= (2 * k) << log_l) return;
  const uint64_t r = j / (2 * k), t = j % (2 * k);
#pragma unroll
  for (int q = 0; q < 8; ++q) a[8 * j + q] = t + 2 <= k ? srs[8 * (r + ((k - 2 - t) << log_l)) + q] : 0;
}

// b[p n + r k + u] = scale c_(p, r + l u), zero from len on, polynomial p < total / n at c + 4 p pitch:
// the l inputs per polynomial of the batched Fr NTT of size 2k (scale: Montgomery form, the
// inverse transform's (2k)^-1; the product is canonical)
__global__ void __launch_bounds__(256) k_cells_gather(const uint64_t* c, uint64_t len, uint64_t pitch, uint64_t total,
                                                      uint64_t k, uint32_t log_l, U256 scale, uint64_t* b) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= total) return;
  const uint64_t n = k << log_l, m = j & (n - 1);
  const uint64_t src = m / k + ((m % k) << log_l);
  U256 v = u256_zero();
  if (src < len) v = Fr::mul(scale, u256_from_u64(c + 4 * ((j - m) / n * pitch + src)));
  u256_to_u64(v, b + 4 * j);
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
// addition: equal, opposite and identity operands are ordinary inputs. Lane t < total = batch x 2k
// is frequency i = t mod 2k of polynomial t / 2k, whose products lie at x + 2n (t / 2k) and whose
// sums go to out + 2k (t / 2k).
__global__ void __launch_bounds__(GN_T) __attribute__((amdgpu_waves_per_eu(2))) k_cells_sum(const Xyzz* x, Xyzz* out, uint64_t total, uint32_t log_k2,
                                                   uint32_t log_l) {
  const uint64_t t = (uint64_t)blockIdx.x * GN_T + threadIdx.x;
  const uint64_t k2 = (uint64_t)1 << log_k2, n2 = k2 << log_l;
  if (t >= total) return;
  const uint64_t i = t & (k2 - 1);
  x += (t - i) << log_l;
  out += t - i;
  const uint32_t log_n2 = log_k2 + log_l;
  Xyzz acc = ld_pt(x + (__brevll((n2 - i) & (n2 - 1)) >> (64 - log_n2)));
#pragma unroll 1
  for (uint64_t r = 1; r < ((uint64_t)1 << log_l); ++r) {
    const uint64_t j = (r << log_k2) + i;
    acc = G1::add2(acc, ld_pt(x + (__brevll(n2 - j) >> (64 - log_n2))));
  }
  st_pt(out + (__brevll((k2 - i) & (k2 - 1)) >> (64 - log_k2)), acc);
}

// The verifier's per-entry pass: pts = [C_0.. | W_0.. | srs[0 .. l), by the host],
// sc = [rho_j | rho_j c_(idx_j) | .]; *flag set by a point (an SRS point included) that is not
// canonical or not on the curve.
__global__ void __launch_bounds__(256) k_cells_vprep(const uint64_t* commits, const uint64_t* w, const uint64_t* rho,
                                                     const uint64_t* idx, uint32_t count, const uint64_t* tw, uint64_t n,
                                                     uint32_t log_l, uint64_t* pts, uint64_t* sc, int* flag) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < (1u << log_l) && g1_bad(pts + 8 * (2 * (uint64_t)count + i))) atomicOr(flag, 1);
  if (i >= count) return;
  kzg_vpoints(commits, w, count, i, pts, flag);
  const U256 r = u256_from_u64(rho + 4 * (uint64_t)i);
  u256_to_u64(r, sc + 4 * (uint64_t)i);
  u256_to_u64(Fr::mul(Fr::to_mont(fr_domain_pow(tw, n, idx[i] << log_l)), r), sc + 4 * ((uint64_t)count + i));
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
    const U256 f = Fr::mul(Fr::to_mont(u256_from_u64(rho + 4 * j)), Fr::to_mont(fr_domain_pow(tw, n, (n - e) & (n - 1))));
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
  const U256 sum = fr_block_sum(sh, acc);
  if (threadIdx.x == 0) u256_to_u64(Fr::sub(u256_zero(), sum), sc_srs + 4 * t);
}

int cells_setup_args(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* omega2, size_t n, size_t l,
                     const uint64_t* xext, U256* w2m, uint32_t* log_l) {
  if (!ctx || !srs || !omega2 || !xext) return fail(PBF_EINVAL, "null argument");
  int rc = fk20_domain(n, omega2, w2m);
  if (rc || (rc = kzg_l_check(n, l, log_l))) return rc;
  if (srs_m < n - l) return fail(PBF_EINVAL, "SRS too short");
  return 0;
}
int cells_open_args(pbf_ctx* ctx, const uint64_t* xext, size_t n, size_t l, const uint64_t* omega2,
                    const uint64_t* polys, size_t len, size_t pitch, size_t batch, const uint64_t* weights,
                    const uint64_t* out_w, U256* w2m, uint32_t* log_l) {
  int rc = fk20_open_args(ctx, xext, n, omega2, polys, len, pitch, batch, weights, out_w, w2m);
  if (rc) return rc;
  return kzg_l_check(n, l, log_l);
}
int cells_each_args(pbf_ctx* ctx, const uint64_t* xext, size_t n, size_t l, const uint64_t* omega2,
                    const uint64_t* polys, size_t len, size_t pitch, size_t batch, const uint64_t* out_w, U256* w2m,
                    uint32_t* log_l) {
  int rc = fk20_polys_args(ctx, xext, n, omega2, polys, len, pitch, batch, out_w, w2m);
  if (rc || (rc = kzg_l_check(n, l, log_l))) return rc;
  if (batch > CELLS_EACH_MAX / n) return fail(PBF_EINVAL, "this version supports batch * n <= 2^24");
  return 0;
}

// out_y of both cell openings: the values of every polynomial, stored cell-major (l = 1 and l = n:
// as the transform leaves them); wm = omega, of order n
int cells_values(pbf_ctx* ctx, const U256& wm, const uint64_t* d_polys, size_t len, size_t pitch, size_t batch,
                 size_t n, size_t l, uint32_t log_l, uint64_t* d_out_y, hipStream_t s) {
  uint64_t om[4];
  hout(om, wm);
  const bool direct = l == 1 || l == n;
  DevBuf& by = ctx->buf("kzg.cells.y");
  int rc;
  if (!direct && (rc = by.ensure(batch * n * 32))) return rc;
  uint64_t* y = direct ? d_out_y : (uint64_t*)by.p;
  if ((rc = polys_ntt(ctx, om, d_polys, len, pitch, batch, n, y, s))) return rc;
  return direct ? 0 : cells_ystore_run(y, batch, n / l, log_l, d_out_y, s);
}

// d_out_w[p k + i] = W_i of polynomial p < np (len > l coefficients at d_polys + 4 p pitch): the
// steps of the section's head, every vector np times as long. The weighted call is np = 1 on c.
int cells_proofs(pbf_ctx* ctx, const uint64_t* d_xext, size_t n, size_t l, uint32_t log_l, const U256& w2m,
                 const uint64_t* d_polys, size_t len, size_t pitch, size_t np, uint64_t* d_out_w, hipStream_t s) {
  const uint64_t one[4] = {1, 0, 0, 0};
  const uint64_t k = n / l, k2 = 2 * k, n2 = 2 * (uint64_t)n;
  DevBuf &bg = ctx->buf("kzg.cells.b"), &bb = ctx->buf("kzg.fk20.bhat");
  G1Work w;
  int rc;
  if ((rc = bg.ensure(np * n * 32)) || (rc = bb.ensure(np * n2 * 32)) ||
      (rc = g1_work(ctx, np * (l == 1 ? n2 : n2 + k2), np * n2, &w)))
    return rc;
  uint64_t *b = (uint64_t*)bg.p, *bhat = (uint64_t*)bb.p;
  // b_(p,r) = (2k)^-1 times every l-th coefficient of p: the inverse transform's factor rides on them
  hipLaunchKernelGGL(k_cells_gather, dim3((uint32_t)((np * n + 255) / 256)), dim3(256), 0, s, d_polys, (uint64_t)len,
                     (uint64_t)pitch, (uint64_t)(np * n), k, log_l, fr_inv(hm64(k2)), b);
  PBF_HIP(hipGetLastError());
  const U256 wlm = fr_pow(w2m, l);  // omega2^l, of order 2k; its square omega^l, of order k
  uint64_t wl[4];
  hout(wl, wlm);
  if ((rc = pbf_ntt_fr256_coset_batch_dev(ctx, wl, one, b, k, bhat, k2, np * l, 0, s))) return rc;
  // the np x 2n products as one vector; with l = 1 they lie where the inverse transforms read
  // them, else their sums per frequency are put there, behind the products
  if ((rc = g1_mul_xyzz_run(w, d_xext, bhat, n2, np, s))) return rc;
  if (l > 1) {
    uint32_t log_k2 = 0;
    while (((uint64_t)1 << log_k2) < k2) ++log_k2;
    hipLaunchKernelGGL(k_cells_sum, dim3((uint32_t)((np * k2 + GN_T - 1) / GN_T)), dim3(GN_T), 0, s, (const Xyzz*)w.x,
                       w.x + np * n2, (uint64_t)(np * k2), log_k2, log_l);
    PBF_HIP(hipGetLastError());
    w.x += np * n2;
  }
  // c = a * b summed over the slabs; h = c[k-1 .. 2k-1); W = NTT_k(h), at the pitch 2k throughout
  if ((rc = g1_ntt_stages(ctx, wlm, k2, np, k2, w, s)) || (rc = g1_ntt_slice(w, k, np, s)) ||
      (rc = g1_ntt_stages(ctx, Fr::mul(wlm, wlm), k, np, k2, w, s)))
    return rc;
  return g1_ntt_store(w, d_out_w, k, np, k2, s);
}

}  // namespace

int pbf::cells_ystore_run(const uint64_t* y, uint64_t batch, uint64_t k, uint32_t log_l, uint64_t* out, hipStream_t s) {
  const uint64_t total = (batch * k) << log_l;
  hipLaunchKernelGGL(k_cells_ystore, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, y, total, k, log_l, out);
  PBF_HIP(hipGetLastError());
  return 0;
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
  return g1_ntt_run(ctx, w2m, d_xext, d_xext, 2 * n, 1, 0, s);
}

extern "C" int pbf_kzg_fk20_setup_bn254(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* omega2,
                                        size_t n, uint64_t* xext) {
  U256 w2m;
  int rc = fk20_setup_args(ctx, srs, srs_m, omega2, n, xext, &w2m);
  if (rc) return rc;
  const size_t used = n - 1;  // the points the setup reads
  return setup_host(ctx, srs, used, n, xext, [&](const uint64_t* d_srs, uint64_t* d_xext, hipStream_t s) {
    return pbf_kzg_fk20_setup_bn254_dev(ctx, d_srs, used, omega2, n, d_xext, s);
  });
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
  if (d_out_y && (rc = polys_ntt(ctx, om, d_polys, len, pitch, batch, n, d_out_y, s))) return rc;
  if (len == 1) {  // constants: every quotient is empty, every W the identity
    PBF_HIP(hipMemsetAsync(d_out_w, 0, n * 64, s));
    return PBF_OK;
  }
  const uint64_t n2 = 2 * (uint64_t)n;
  DevBuf &bc = ctx->buf("kzg.comb"), &bb = ctx->buf("kzg.fk20.bhat");
  G1Work w;
  if ((rc = bc.ensure(len * 32)) || (rc = bb.ensure(n2 * 32)) || (rc = g1_work(ctx, n2, n2, &w))) return rc;
  uint64_t *comb = (uint64_t*)bc.p, *bhat = (uint64_t*)bb.p;
  // c = (2n)^-1 sum_b w_b p_b
  if ((rc = kzg_comb(d_polys, len, pitch, batch, scaled_weights(weights, batch, fr_inv(hm64(n2))).data(), comb, s)))
    return rc;
  if ((rc = pbf_ntt_fr256_coset_batch_dev(ctx, omega2, one, comb, len, bhat, n2, 1, 0, s))) return rc;
  // chat_i = [bhat_i] xext_i where the inverse transform reads it; c = a * b; h = c[n-1 .. 2n-1); W = NTT_n(h)
  if ((rc = g1_mul_xyzz_run(w, d_xext, bhat, n2, 1, s)) || (rc = g1_ntt_stages(ctx, w2m, n2, 1, n2, w, s)) ||
      (rc = g1_ntt_slice(w, n, 1, s)) || (rc = g1_ntt_stages(ctx, wm, n, 1, n2, w, s)))
    return rc;
  return g1_ntt_store(w, d_out_w, n, 1, n2, s);
}

extern "C" int pbf_kzg_open_all_bn254(pbf_ctx* ctx, const uint64_t* xext, size_t n, const uint64_t* omega2,
                                      const uint64_t* polys, size_t len, size_t pitch, size_t batch,
                                      const uint64_t* weights, uint64_t* out_y, uint64_t* out_w) {
  U256 w2m;
  int rc = fk20_open_args(ctx, xext, n, omega2, polys, len, pitch, batch, weights, out_w, &w2m);
  if (rc) return rc;
  return open_host(ctx, xext, n, polys, len, pitch, batch, out_y, out_w, n,
                   [&](const uint64_t* d_xext, const uint64_t* d_polys, uint64_t* d_y, uint64_t* d_w, hipStream_t s) {
                     return pbf_kzg_open_all_bn254_dev(ctx, d_xext, n, omega2, d_polys, len, len, batch, weights, d_y, d_w, s);
                   });
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
  const uint64_t k = n / l;
  if (k == 1) {  // every a_r is two identities, and so is its transform
    PBF_HIP(hipMemsetAsync(d_xext, 0, 2 * n * 64, s));
    return PBF_OK;
  }
  hipLaunchKernelGGL(k_cells_a, dim3((uint32_t)((2 * n + 255) / 256)), dim3(256), 0, s, d_srs, k, log_l, d_xext);
  PBF_HIP(hipGetLastError());
  // the l slabs are one batch of transforms of size 2k, root omega2^l, in place
  return g1_ntt_run(ctx, fr_pow(w2m, l), d_xext, d_xext, 2 * k, l, 0, s);
}

extern "C" int pbf_kzg_cells_setup_bn254(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* omega2,
                                         size_t n, size_t l, uint64_t* xext) {
  U256 w2m;
  uint32_t log_l;
  int rc = cells_setup_args(ctx, srs, srs_m, omega2, n, l, xext, &w2m, &log_l);
  if (rc) return rc;
  const size_t used = n - l;  // the points the setup reads
  return setup_host(ctx, srs, used, n, xext, [&](const uint64_t* d_srs, uint64_t* d_xext, hipStream_t s) {
    return pbf_kzg_cells_setup_bn254_dev(ctx, d_srs, used, omega2, n, l, d_xext, s);
  });
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
  const uint64_t k = n / l;
  if (d_out_y &&
      (rc = cells_values(ctx, Fr::mul(w2m, w2m), d_polys, len, pitch, batch, n, l, log_l, d_out_y, s)))  // omega = omega2^2
    return rc;
  if (len <= l) {  // degree below l: every quotient is zero, every W the identity (k = 1 included)
    PBF_HIP(hipMemsetAsync(d_out_w, 0, k * 64, s));
    return PBF_OK;
  }
  DevBuf& bc = ctx->buf("kzg.comb");
  if ((rc = bc.ensure(len * 32))) return rc;
  uint64_t* comb = (uint64_t*)bc.p;
  // c = sum_b w_b p_b, then its proofs
  if ((rc = kzg_comb(d_polys, len, pitch, batch, scaled_weights(weights, batch, fr_one_m()).data(), comb, s)))
    return rc;
  return cells_proofs(ctx, d_xext, n, l, log_l, w2m, comb, len, len, 1, d_out_w, s);
}

extern "C" int pbf_kzg_open_cells_each_bn254_dev(pbf_ctx* ctx, const uint64_t* d_xext, size_t n, size_t l,
                                                 const uint64_t* omega2, const uint64_t* d_polys, size_t len,
                                                 size_t pitch, size_t batch, uint64_t* d_out_y, uint64_t* d_out_w,
                                                 void* stream) {
  U256 w2m;
  uint32_t log_l;
  int rc = cells_each_args(ctx, d_xext, n, l, omega2, d_polys, len, pitch, batch, d_out_w, &w2m, &log_l);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  if (d_out_y &&
      (rc = cells_values(ctx, Fr::mul(w2m, w2m), d_polys, len, pitch, batch, n, l, log_l, d_out_y, s)))  // omega = omega2^2
    return rc;
  if (len <= l) {  // degree below l: every quotient is zero, every W the identity (k = 1 included)
    PBF_HIP(hipMemsetAsync(d_out_w, 0, batch * (n / l) * 64, s));
    return PBF_OK;
  }
  return cells_proofs(ctx, d_xext, n, l, log_l, w2m, d_polys, len, pitch, batch, d_out_w, s);
}

extern "C" int pbf_kzg_open_cells_each_bn254(pbf_ctx* ctx, const uint64_t* xext, size_t n, size_t l,
                                             const uint64_t* omega2, const uint64_t* polys, size_t len, size_t pitch,
                                             size_t batch, uint64_t* out_y, uint64_t* out_w) {
  U256 w2m;
  uint32_t log_l;
  int rc = cells_each_args(ctx, xext, n, l, omega2, polys, len, pitch, batch, out_w, &w2m, &log_l);
  if (rc) return rc;
  return open_host(ctx, xext, n, polys, len, pitch, batch, out_y, out_w, batch * (n / l),
                   [&](const uint64_t* d_xext, const uint64_t* d_polys, uint64_t* d_y, uint64_t* d_w, hipStream_t s) {
                     return pbf_kzg_open_cells_each_bn254_dev(ctx, d_xext, n, l, omega2, d_polys, len, len, batch, d_y, d_w,
                                                              s);
                   });
}

extern "C" int pbf_kzg_open_cells_bn254(pbf_ctx* ctx, const uint64_t* xext, size_t n, size_t l, const uint64_t* omega2,
                                        const uint64_t* polys, size_t len, size_t pitch, size_t batch,
                                        const uint64_t* weights, uint64_t* out_y, uint64_t* out_w) {
  U256 w2m;
  uint32_t log_l;
  int rc = cells_open_args(ctx, xext, n, l, omega2, polys, len, pitch, batch, weights, out_w, &w2m, &log_l);
  if (rc) return rc;
  return open_host(ctx, xext, n, polys, len, pitch, batch, out_y, out_w, n / l,
                   [&](const uint64_t* d_xext, const uint64_t* d_polys, uint64_t* d_y, uint64_t* d_w, hipStream_t s) {
                     return pbf_kzg_open_cells_bn254_dev(ctx, d_xext, n, l, omega2, d_polys, len, len, batch, weights, d_y,
                                                         d_w, s);
                   });
}

extern "C" int pbf_kzg_verify_cells_bn254(pbf_ctx* ctx, const uint64_t* g2, const uint64_t* srs, size_t srs_m,
                                          const uint64_t* omega, size_t n, size_t l, size_t count,
                                          const uint64_t* commits, const uint64_t* cell_idx, const uint64_t* ys,
                                          const uint64_t* w, const uint64_t* rho, int* ok) {
  if (!ctx || !g2 || !srs || !omega || !commits || !cell_idx || !ys || !w || !rho || !ok)
    return fail(PBF_EINVAL, "null argument");
  *ok = 0;
  U256 wm;
  uint32_t log_l;
  int rc = kzg_n_check(n);
  if (rc || (rc = fr_domain_check(omega, n, &wm)) || (rc = kzg_l_check(n, l, &log_l))) return rc;
  if (srs_m < l) return fail(PBF_EINVAL, "SRS too short");
  if (count == 0 || count > CELLS_MAX_COUNT) return fail(PBF_EINVAL, "count must be in 1 .. 2^20");
  if (count * l > CELLS_MAX_VALUES) return fail(PBF_EINVAL, "count * l must be at most 2^22");
  const size_t k = n / l, c = count, vals = count * l;
  if ((rc = kzg_idx_check(cell_idx, c, k))) return rc;
  if (!fr_canonical(ys, vals)) return fail(PBF_EINVAL, "ys must be canonical");
  if ((rc = kzg_rho_check(rho, c))) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  const uint32_t nchunks = (uint32_t)((c + CV_CH - 1) / CV_CH);
  // inputs: commits, w (8 words each), rho (4), cell_idx (1) per entry; the values and their inverse transforms
  KzgVerify v;
  if ((rc = kzg_verify_bufs(ctx, c, l, c * 21 + vals * 8, (size_t)nchunks << log_l, &v))) return rc;
  const uint64_t* tw = nullptr;
  if (n > 1 && (rc = fr_domain_table(ctx, wm, n, s, &tw))) return rc;
  uint64_t *d_rho = v.in + 16 * c, *d_idx = v.in + 20 * c, *d_y = v.in + 21 * c;
  uint64_t* d_v = l > 1 ? d_y + 4 * vals : d_y;  // the inverse transform of size 1 is the value itself
  if ((rc = kzg_verify_upload(v, c, commits, w, rho, d_rho, s))) return rc;
  PBF_HIP(hipMemcpyAsync(d_idx, cell_idx, c * 8, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(d_y, ys, vals * 32, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(v.pts + 16 * c, srs, l * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemsetAsync(v.flag, 0, sizeof(int), s));
  if (l > 1) {  // v_j = INTT_l(y_j), root omega^k, all cells in one batch
    uint64_t wk[4];
    hout(wk, fr_pow(wm, k));
    if ((rc = pbf_ntt_fr256_batch_dev(ctx, wk, d_y, d_v, l, c, 1, s))) return rc;
  }
  hipLaunchKernelGGL(k_cells_vprep, dim3((uint32_t)((std::max(c, l) + 255) / 256)), dim3(256), 0, s,
                     (const uint64_t*)v.in, (const uint64_t*)(v.in + 8 * c), (const uint64_t*)d_rho,
                     (const uint64_t*)d_idx, (uint32_t)c, tw, (uint64_t)n, log_l, v.pts, v.sc, v.flag);
  hipLaunchKernelGGL(k_cells_vsweep, dim3((uint32_t)((((uint64_t)nchunks << log_l) + 255) / 256)), dim3(256), 0, s,
                     (const uint64_t*)d_v, (const uint64_t*)d_rho, (const uint64_t*)d_idx, (uint32_t)c, tw, (uint64_t)n,
                     log_l, nchunks, v.part);
  hipLaunchKernelGGL(k_cells_vsum, dim3((uint32_t)l), dim3(256), 0, s, (const uint64_t*)v.part, nchunks, log_l,
                     v.sc + 8 * c);
  // e(sum rho W, [s^l]G2) e(-(sum rho C - [sum rho I](s) G + sum rho c W), G2) == 1
  return kzg_verify_tail(ctx, v, c, l, g2, ok, s);
}
