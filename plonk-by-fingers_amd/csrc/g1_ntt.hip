// NTT over BN254 G1 on gfx950 (include/pbf.h "KZG in evaluation form"): out[k] = sum_j
// [omega^(jk)] in[j] over points, and the evaluation domain H = <omega> it shares with the
// opening from evaluations (kzg.hip). Its main use is the Lagrange-basis SRS: the inverse
// transform of [s^j]G is [L_i(s)]G, with no trapdoor.
//
//   load      canonical affine in[i] -> Xyzz (Montgomery) at scratch[bitrev(i)]; the transform
//             runs in the scratch, so in and out may be one buffer
//   stages    log2 n radix-2 decimation-in-time launches, one lane per butterfly
//             (P, Q) -> (P + [w]Q, P - [w]Q), w = omega^(j n / 2h) for position j of a group of
//             half-width h. The first stage (h = 1) and position 0 of every group have w = 1 and
//             skip the product. With the table holding omega^i for i < n/2 only, no twiddle is
//             -1: the butterfly's own subtraction is the negation.
//   store     Xyzz -> canonical affine (to_affine_plain). The inverse is the forward transform
//             read back at index (n - i) mod n, times n^-1: one product per point in this pass,
//             none added to the butterflies.
//
// [w]Q is a fixed 4-bit unsigned window: the lane writes 1Q .. 15Q (one dbl2, thirteen add2) to
// its own 15 x 128 B of a context scratch table, then 64 windows of four doublings and one
// addition of the table entry its digit names (none for digit 0). The digits come from the
// scalar's words in memory by shifts, and the entry by address, so no register array is indexed
// at run time. A launch covers at most 2^g1ntt.tile_log products (2^14: a 30 MiB table); wider
// stages run as several launches over the same table. Stages with h < 64 map lanes position-
// major, so that a wave shares one twiddle (uniform digits, uniform skips) whenever the stage
// has 64 groups or more. Every group operation is add2 / dbl2, the complete forms: a butterfly's
// operands can be equal, opposite or the identity (tests/test_g1_ntt_gpu.py builds each case).
//
// The window product and the point loads and stores live in g1_win.hpp, shared with the pointwise
// product (g1_mul.hip). FK20 (kzg.hip) strings the pieces together through prover.hpp without
// leaving Xyzz: the stages alone are the unscaled transform, and k_g1_slice loads a transform of
// half the size from the scratch of the one before.
//
// A batch of B transforms of size n under one omega (pbf_ntt_g1_bn254_batch*, the cell proofs'
// setup and pbf_kzg_open_cells_each_bn254*) is the same kernels over B n/2 butterflies per stage:
// loaded bit-reversed per transform and laid one behind the other, the B transforms are the first
// log2 n stages of a transform of size B n with the twiddles of size n. A launch of a stage costs
// the latency of one window product whether it carries 64 lanes or 2^14, so the batch fills
// launches that a single small transform leaves almost empty. Every kernel takes
// the transform's own log_n (twiddles, bit reversal, the inverse's (n - i) mod n), the number of
// transforms where it splits a lane index, and the pitch between transforms in the scratch (n
// here; 2k for the size-k transforms that k_g1_slice leaves in the scratch of the size-2k ones).
// The single entry points are batch = 1 of the same code. With B groups-of-a-stage to spread over,
// lanes run position-major over all B x groups whenever that is 64 or more, not only below half-
// width 64: position j has one twiddle in every transform, so a wave still shares its scalar. At
// B = 1 this is the mapping above. Launch boundaries fall inside and between transforms.
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../include/pbf.h"
#include "g1_win.hpp"

using namespace pbf;

namespace {

constexpr int GN_JM_LOG = 6;      // stages with half-width below 2^6 map lanes position-major
constexpr int GN_TILE_LOG = 14;   // products per launch (option g1ntt.tile_log, 6 .. 20)
constexpr size_t G1_NTT_MAX = (size_t)1 << 28;  // points per call: the scratch of the largest single transform

__global__ void __launch_bounds__(256) k_g1_check(const uint64_t* in, uint64_t n, int* flag) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && g1_bad(in + 8 * i)) atomicOr(flag, 1);
}

// in: `total` points, transforms of 2^log_n one behind the other; each to its own bit-reversed order
__global__ void __launch_bounds__(256) k_g1_load(const uint64_t* in, Xyzz* x, uint64_t total, uint32_t log_n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  uint64_t l[8], any = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) any |= (l[k] = in[8 * i + k]);
  Xyzz p = G1::identity();
  if (any) {
    Affine a;
    a.x = Fq::to_mont(u256_from_u64(l));
    a.y = Fq::to_mont(u256_from_u64(l + 4));
    p = G1::from_affine(a);
  }
  const uint64_t m = i & (((uint64_t)1 << log_n) - 1);
  st_pt(x + (i - m) + (__brevll(m) >> (64 - log_n)), p);  // log_n >= 1
}

// One stage: butterflies [b0, b0 + count) of the batch x n/2, half-width 2^log_half, transform q at
// x + q pitch. all_groups = batch x groups of this stage; the stage-wide group gg = q groups + g.
__global__ void __launch_bounds__(GN_T) __attribute__((amdgpu_waves_per_eu(2))) k_g1_stage(Xyzz* x, const uint64_t* tw, Xyzz* tbl, uint64_t stride, uint64_t b0,
                                                   uint64_t count, uint32_t log_half, uint32_t log_n, uint64_t all_groups,
                                                   uint64_t pitch) {
  const uint64_t t = (uint64_t)blockIdx.x * GN_T + threadIdx.x;
  if (t >= count) return;
  const uint64_t b = b0 + t;
  const uint32_t log_groups = log_n - 1 - log_half;
  const uint64_t groups = (uint64_t)1 << log_groups;
  uint64_t j, gg;
  // position-major: neighbouring lanes share the twiddle. One transform: below half-width 64; a
  // batch: also wherever it has 64 groups or more between its transforms
  if (log_half < GN_JM_LOG || (all_groups > groups && all_groups >= 64)) {
    j = b / all_groups;  // the batch need not be a power of two: one division against ~334 group operations
    gg = b - j * all_groups;
  } else {
    j = b & (((uint64_t)1 << log_half) - 1);
    gg = b >> log_half;
  }
  const uint64_t q = gg >> log_groups, g = gg & (groups - 1);
  const uint64_t i0 = q * pitch + (g << (log_half + 1)) + j, i1 = i0 + ((uint64_t)1 << log_half);
  Xyzz Q = ld_pt(x + i1);
  if (j) Q = g1_mul_win(Q, (const uint32_t*)(tw + 4 * (j << log_groups)), tbl + t, stride);
  const Xyzz P = ld_pt(x + i0);  // after the product: not live across it
  st_pt(x + i0, G1::add2(P, Q));
  Q.Y = Fq::sub(u256_zero(), Q.Y);
  st_pt(x + i1, G1::add2(P, Q));
}

// out[i] for i in [i0, i0 + count) of the batch x n, i = q n + m: transform q's x[m], or for the
// inverse [n^-1] x[(n - m) mod n]; transform q at x + q pitch, out compact
__global__ void __launch_bounds__(GN_T) __attribute__((amdgpu_waves_per_eu(2))) k_g1_store(const Xyzz* x, uint64_t* out, const uint32_t* ninv, Xyzz* tbl,
                                                   uint64_t stride, uint64_t i0, uint64_t count, uint32_t log_n,
                                                   uint64_t pitch) {
  const uint64_t t = (uint64_t)blockIdx.x * GN_T + threadIdx.x;
  if (t >= count) return;
  const uint64_t i = i0 + t, n = (uint64_t)1 << log_n, m = i & (n - 1);
  Xyzz p = ld_pt(x + (i >> log_n) * pitch + (ninv ? (n - m) & (n - 1) : m));
  if (ninv) p = g1_mul_win(p, ninv, tbl + t, stride);
  U256 ax, ay;
  G1::to_affine_plain(p, &ax, &ay);
  u256_to_u64(ax, out + 8 * i);
  u256_to_u64(ay, out + 8 * i + 4);
}

// FK20 (kzg_cells.hip): the size-n transform's load, from the scratch itself. x holds the 2n points
// c of the convolution in natural order; h_m = c[n - 1 + m] goes to x[bitrev_n(m)] for m < n - 1,
// and h_(n-1) = c[2n - 2], always the identity, is written as such. Lane 0 alone reads and writes
// below n (x[n - 1] -> x[0], then the identity at x[n - 1] = x[bitrev_n(n - 1)]); every other lane
// reads x[n .. 2n - 2) and writes x[1 .. n - 1), so no lane reads what another writes. A batch:
// `total` = batch x n lanes, transform q in place at x + 2 q n, where its 2n points lie: the
// transforms of size n keep the pitch 2n, so none is written over another's source.
__global__ void __launch_bounds__(256) k_g1_slice(Xyzz* x, uint64_t total, uint32_t log_n) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const uint64_t n = (uint64_t)1 << log_n, m = t & (n - 1);
  if (m + 1 >= n) return;
  x += 2 * (t - m);
  const Xyzz p = ld_pt(x + n - 1 + m);
  st_pt(x + (__brevll(m) >> (64 - log_n)), p);
  if (m == 0) st_pt(x + n - 1, G1::identity());
}

uint32_t blocks_of(uint64_t threads, uint32_t per) { return (uint32_t)((threads + per - 1) / per); }

int ntt_args(pbf_ctx* ctx, const uint64_t* omega, const uint64_t* in, const uint64_t* out, size_t n, size_t batch,
             U256* wm) {
  if (!ctx || !omega || !in || !out) return fail(PBF_EINVAL, "null argument");
  int rc = fr_domain_check(omega, n, wm);
  if (rc) return rc;
  if (batch == 0) return fail(PBF_EINVAL, "batch must be at least 1");
  if (batch > G1_NTT_MAX / n) return fail(PBF_EINVAL, "n * batch must be at most 2^28");
  return 0;
}

uint32_t log2_of(uint64_t n) {
  uint32_t log_n = 0;
  while (((uint64_t)1 << log_n) < n) ++log_n;
  return log_n;
}

// pbf_ntt_g1_bn254[_batch] past its argument checks: upload, check of every point, transform, download
int ntt_host(pbf_ctx* ctx, const U256& wm, const uint64_t* in, uint64_t* out, size_t n, size_t batch, int inverse) {
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  DevBuf& bio = ctx->buf("g1ntt.io");
  const size_t total = n * batch;
  int rc;
  if ((rc = bio.ensure(total * 64))) return rc;
  uint64_t* io = (uint64_t*)bio.p;
  PBF_HIP(hipMemcpyAsync(io, in, total * 64, hipMemcpyHostToDevice, s));
  int bad = 0;
  if ((rc = g1_check_run(ctx, io, total, s, &bad))) return rc;
  if (bad) return fail(PBF_EINVAL, "a point is not canonical or not on the curve");
  if ((rc = g1_ntt_run(ctx, wm, io, io, n, batch, inverse, s))) return rc;
  PBF_HIP(hipMemcpyAsync(out, io, total * 64, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  return PBF_OK;
}

}  // namespace

namespace pbf {

int fr_domain_check(const uint64_t* omega, size_t n, U256* wm) {
  if (n == 0 || (n & (n - 1))) return fail(PBF_EINVAL, "n must be a power of two");
  if (n > ((size_t)1 << 28)) return fail(PBF_EINVAL, "n exceeds the 2-adicity of BN254 Fr (2^28)");
  if (!fr_canonical(omega)) return fail(PBF_EINVAL, "omega not canonical");
  *wm = hm(omega);
  if (n == 1 ? !heq1(*wm) : (!heq1(fr_pow(*wm, n)) || heq1(fr_pow(*wm, n / 2))))
    return fail(PBF_EINVAL, "omega does not have order n");
  return 0;
}

int fr_domain_table(pbf_ctx* ctx, const U256& wm, uint64_t n, hipStream_t s, const uint64_t** tw) {
  std::array<uint64_t, 5> key;
  hout(key.data(), wm);
  key[4] = n;
  auto& slot = ctx->domain_tw[key];
  if (!slot) {
    std::unique_ptr<DevBuf> b(new DevBuf());
    const uint64_t h = n / 2;
    int rc = b->ensure((h + 1) * 32);
    if (rc) {
      ctx->domain_tw.erase(key);
      return rc;
    }
    uint64_t ninv[4];
    hout(ninv, fr_inv(hm64(n)));
    hipError_t e = hipMemcpyAsync((uint64_t*)b->p + 4 * h, ninv, 32, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) rc = fr_powers_run((uint64_t*)b->p, h, wm, fr_one_m(), s);
    if (e == hipSuccess && !rc) e = hipStreamSynchronize(s);  // other streams may use it next
    if (e != hipSuccess || rc) {
      ctx->domain_tw.erase(key);
      return rc ? rc : fail(PBF_EDEVICE, std::string("domain table: ") + hipGetErrorString(e));
    }
    slot = std::move(b);
  }
  *tw = (const uint64_t*)slot->p;
  return 0;
}

int g1_work(pbf_ctx* ctx, uint64_t points, uint64_t products, G1Work* w) {
  const long long tl = std::min<long long>(20, std::max<long long>(6, ctx->options.num("g1ntt.tile_log", GN_TILE_LOG)));
  w->stride = std::min((uint64_t)1 << tl, products);  // the widest launch that multiplies
  DevBuf &bx = ctx->buf("g1ntt.x"), &bt = ctx->buf("g1ntt.tbl");
  int rc;
  if (points && (rc = bx.ensure(points * sizeof(Xyzz)))) return rc;
  if ((rc = bt.ensure(w->stride * GN_ENT * sizeof(Xyzz)))) return rc;
  w->x = (Xyzz*)bx.p;
  w->tbl = (Xyzz*)bt.p;
  return 0;
}

int g1_check_run(pbf_ctx* ctx, const uint64_t* d_pts, uint64_t n, hipStream_t s, int* bad) {
  DevBuf& bfl = ctx->buf("g1ntt.flag");
  int rc;
  if ((rc = bfl.ensure(sizeof(int)))) return rc;
  PBF_HIP(hipMemsetAsync(bfl.p, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_g1_check, dim3(blocks_of(n, 256)), dim3(256), 0, s, d_pts, n, (int*)bfl.p);
  PBF_HIP(hipGetLastError());
  PBF_HIP(hipMemcpyAsync(bad, bfl.p, sizeof(int), hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  return 0;
}

int g1_ntt_stages(pbf_ctx* ctx, const U256& wm, uint64_t n, uint64_t batch, uint64_t pitch, const G1Work& w,
                  hipStream_t s) {
  const uint32_t log_n = log2_of(n);
  const uint64_t nb = batch * (n / 2);
  const uint64_t* tw = nullptr;
  int rc;
  if ((rc = fr_domain_table(ctx, wm, n, s, &tw))) return rc;
  for (uint32_t lh = 0; lh < log_n; ++lh) {
    const uint64_t step = lh ? w.stride : nb;  // the first stage has no product and no table
    for (uint64_t b0 = 0; b0 < nb; b0 += step) {
      const uint64_t cnt = std::min(step, nb - b0);
      hipLaunchKernelGGL(k_g1_stage, dim3(blocks_of(cnt, GN_T)), dim3(GN_T), 0, s, w.x, tw, w.tbl, w.stride, b0, cnt,
                         lh, log_n, batch * ((n / 2) >> lh), pitch);
    }
  }
  PBF_HIP(hipGetLastError());
  return 0;
}

int g1_ntt_slice(const G1Work& w, uint64_t n, uint64_t batch, hipStream_t s) {
  hipLaunchKernelGGL(k_g1_slice, dim3(blocks_of(batch * n, 256)), dim3(256), 0, s, w.x, batch * n, log2_of(n));
  PBF_HIP(hipGetLastError());
  return 0;
}

int g1_ntt_store(const G1Work& w, uint64_t* d_out, uint64_t n, uint64_t batch, uint64_t pitch, hipStream_t s) {
  hipLaunchKernelGGL(k_g1_store, dim3(blocks_of(batch * n, GN_T)), dim3(GN_T), 0, s, (const Xyzz*)w.x, d_out,
                     (const uint32_t*)nullptr, w.tbl, w.stride, (uint64_t)0, batch * n, log2_of(n), pitch);
  PBF_HIP(hipGetLastError());
  return 0;
}

int g1_ntt_run(pbf_ctx* ctx, const U256& wm, const uint64_t* d_in, uint64_t* d_out, uint64_t n, uint64_t batch,
               int inverse, hipStream_t s) {
  const uint64_t total = batch * n;
  if (n == 1) {
    if (d_in != d_out) PBF_HIP(hipMemcpyAsync(d_out, d_in, total * 64, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  const uint32_t log_n = log2_of(n);
  const uint64_t* tw = nullptr;
  G1Work w;
  int rc;
  if ((rc = fr_domain_table(ctx, wm, n, s, &tw)) || (rc = g1_work(ctx, total, inverse ? total : total / 2, &w)))
    return rc;
  hipLaunchKernelGGL(k_g1_load, dim3(blocks_of(total, 256)), dim3(256), 0, s, d_in, w.x, total, log_n);
  if ((rc = g1_ntt_stages(ctx, wm, n, batch, n, w, s))) return rc;
  if (!inverse) return g1_ntt_store(w, d_out, n, batch, n, s);
  const uint32_t* ninv = (const uint32_t*)(tw + 4 * (n / 2));
  for (uint64_t i0 = 0; i0 < total; i0 += w.stride) {
    const uint64_t cnt = std::min(w.stride, total - i0);
    hipLaunchKernelGGL(k_g1_store, dim3(blocks_of(cnt, GN_T)), dim3(GN_T), 0, s, (const Xyzz*)w.x, d_out, ninv, w.tbl,
                       w.stride, i0, cnt, log_n, n);
  }
  PBF_HIP(hipGetLastError());
  return 0;
}

}  // namespace pbf

extern "C" int pbf_ntt_g1_bn254_batch_dev(pbf_ctx* ctx, const uint64_t* omega, const uint64_t* d_in, uint64_t* d_out,
                                          size_t n, size_t batch, int inverse, void* stream) {
  U256 wm;
  int rc = ntt_args(ctx, omega, d_in, d_out, n, batch, &wm);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  return g1_ntt_run(ctx, wm, d_in, d_out, n, batch, inverse, (hipStream_t)stream);
}

extern "C" int pbf_ntt_g1_bn254_batch(pbf_ctx* ctx, const uint64_t* omega, const uint64_t* in, uint64_t* out, size_t n,
                                      size_t batch, int inverse) {
  U256 wm;
  int rc = ntt_args(ctx, omega, in, out, n, batch, &wm);
  return rc ? rc : ntt_host(ctx, wm, in, out, n, batch, inverse);
}

extern "C" int pbf_ntt_g1_bn254_dev(pbf_ctx* ctx, const uint64_t* omega, const uint64_t* d_in, uint64_t* d_out,
                                    size_t n, int inverse, void* stream) {
  return pbf_ntt_g1_bn254_batch_dev(ctx, omega, d_in, d_out, n, 1, inverse, stream);
}

extern "C" int pbf_ntt_g1_bn254(pbf_ctx* ctx, const uint64_t* omega, const uint64_t* in, uint64_t* out, size_t n,
                                int inverse) {
  return pbf_ntt_g1_bn254_batch(ctx, omega, in, out, n, 1, inverse);
}
