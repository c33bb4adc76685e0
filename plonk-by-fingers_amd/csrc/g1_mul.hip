// The pointwise product over BN254 G1 on gfx950 (include/pbf.h "Every opening at once"):
// out_i = [k_i] P_i, a different point for every scalar. The fixed-base comb (msm.hip) multiplies
// G only and the MSM sums; this is the product FK20 needs between its two G1 transforms
// (kzg.hip), and an entry point of its own.
//
// One lane per product, one wave per workgroup, on the window product of the G1 NTT's butterflies
// (g1_win.hpp): 1P .. 15P into the lane's 15 x 128 B of the context's window table, then 64 windows
// of four doublings and the addition of the entry the digit names. A launch covers at most
// 2^g1ntt.tile_log products; longer vectors run as several launches over the same table.
//
// Unlike a butterfly stage, the lanes of a wave share no scalar, so the skips diverge: the wave
// issues the addition of a window whenever one of its 64 lanes has a nonzero digit there, which at
// 15/16 per lane is every window (64 issued against 60 useful on average, 1.2 % of the product's
// 334 operations), and the doublings below a lane's top digit run while the lanes with a shorter
// scalar idle. The table reads stay one 128 B line per lane, as in the butterflies: the entry
// differs by lane, the number of lines does not. Identity inputs leave at once (their lanes idle).
#include <algorithm>
#include "../../include/pbf.h"
#include "g1_win.hpp"

using namespace pbf;

namespace {

// products [i0, i0 + count): canonical affine in, canonical affine out; out may be pts (a lane
// reads its own point before it writes it)
__global__ void __launch_bounds__(GN_T) __attribute__((amdgpu_waves_per_eu(2))) k_g1_mul(const uint64_t* pts, const uint64_t* sc, uint64_t* out, Xyzz* tbl,
                                                 uint64_t stride, uint64_t i0, uint64_t count) {
  const uint64_t t = (uint64_t)blockIdx.x * GN_T + threadIdx.x;
  if (t >= count) return;
  const uint64_t i = i0 + t;
  const Xyzz p = g1_mul_win(ld_affine(pts + 8 * i), (const uint32_t*)(sc + 4 * i), tbl + t, stride);
  st_affine(out + 8 * i, p);
}

// the same, left as Xyzz at x[bitrev((n - i) mod n)]: no inversion. Past n the vector goes on with
// the next set of n scalars over the same n points, into the next n of x (FK20 of a batch)
__global__ void __launch_bounds__(GN_T) __attribute__((amdgpu_waves_per_eu(2))) k_g1_mul_x(const uint64_t* pts, const uint64_t* sc, Xyzz* x, Xyzz* tbl,
                                                   uint64_t stride, uint64_t i0, uint64_t count, uint64_t n,
                                                   uint32_t log_n) {
  const uint64_t t = (uint64_t)blockIdx.x * GN_T + threadIdx.x;
  if (t >= count) return;
  const uint64_t i = i0 + t, m = i & (n - 1);
  const Xyzz p = g1_mul_win(ld_affine(pts + 8 * m), (const uint32_t*)(sc + 4 * i), tbl + t, stride);
  st_pt(x + (i - m) + (__brevll((n - m) & (n - 1)) >> (64 - log_n)), p);
}

uint32_t blocks_of(uint64_t threads, uint32_t per) { return (uint32_t)((threads + per - 1) / per); }

int mul_run(pbf_ctx* ctx, const uint64_t* d_points, const uint64_t* d_scalars, uint64_t* d_out, uint64_t n,
            hipStream_t s) {
  G1Work w;
  int rc;
  if ((rc = g1_work(ctx, 0, n, &w))) return rc;
  for (uint64_t i0 = 0; i0 < n; i0 += w.stride) {
    const uint64_t cnt = std::min(w.stride, n - i0);
    hipLaunchKernelGGL(k_g1_mul, dim3(blocks_of(cnt, GN_T)), dim3(GN_T), 0, s, d_points, d_scalars, d_out, w.tbl,
                       w.stride, i0, cnt);
  }
  PBF_HIP(hipGetLastError());
  return 0;
}

int mul_args(pbf_ctx* ctx, const uint64_t* points, const uint64_t* scalars, const uint64_t* out, size_t n) {
  if (!ctx || !points || !scalars || !out) return fail(PBF_EINVAL, "null argument");
  if (n == 0 || n > ((size_t)1 << 32)) return fail(PBF_EINVAL, "n must be in 1 .. 2^32");
  return 0;
}

}  // namespace

namespace pbf {

int g1_mul_xyzz_run(const G1Work& w, const uint64_t* d_points, const uint64_t* d_scalars, uint64_t n, uint64_t batch,
                    hipStream_t s) {
  uint32_t log_n = 0;
  while (((uint64_t)1 << log_n) < n) ++log_n;
  const uint64_t total = batch * n;
  for (uint64_t i0 = 0; i0 < total; i0 += w.stride) {
    const uint64_t cnt = std::min(w.stride, total - i0);
    hipLaunchKernelGGL(k_g1_mul_x, dim3(blocks_of(cnt, GN_T)), dim3(GN_T), 0, s, d_points, d_scalars, w.x, w.tbl,
                       w.stride, i0, cnt, n, log_n);
  }
  PBF_HIP(hipGetLastError());
  return 0;
}

}  // namespace pbf

extern "C" int pbf_g1_bn254_mul_dev(pbf_ctx* ctx, const uint64_t* d_points, const uint64_t* d_scalars, uint64_t* d_out,
                                    size_t n, void* stream) {
  int rc = mul_args(ctx, d_points, d_scalars, d_out, n);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  return mul_run(ctx, d_points, d_scalars, d_out, n, (hipStream_t)stream);
}

extern "C" int pbf_g1_bn254_mul(pbf_ctx* ctx, const uint64_t* points, const uint64_t* scalars, uint64_t* out, size_t n) {
  int rc = mul_args(ctx, points, scalars, out, n);
  if (rc) return rc;
  if (!fr_canonical(scalars, n)) return fail(PBF_EINVAL, "scalar not canonical");
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  DevBuf &bio = ctx->buf("g1mul.io"), &bsc = ctx->buf("g1mul.sc");
  if ((rc = bio.ensure(n * 64)) || (rc = bsc.ensure(n * 32))) return rc;
  uint64_t *io = (uint64_t*)bio.p, *sc = (uint64_t*)bsc.p;
  PBF_HIP(hipMemcpyAsync(io, points, n * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(sc, scalars, n * 32, hipMemcpyHostToDevice, s));
  int bad = 0;
  if ((rc = g1_check_run(ctx, io, n, s, &bad))) return rc;
  if (bad) return fail(PBF_EINVAL, "a point is not canonical or not on the curve");
  if ((rc = mul_run(ctx, io, sc, io, n, s))) return rc;
  PBF_HIP(hipMemcpyAsync(out, io, n * 64, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  return PBF_OK;
}
