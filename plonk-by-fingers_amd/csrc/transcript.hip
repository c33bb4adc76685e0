// Fiat-Shamir for the PLONK entry points on gfx950 (include/pbf.h "Fiat-Shamir"):
// the batch kernels over transcript.hpp's Keccak-f[1600] and messages, their host launchers, and
// the entry points that are transcript only (pbf_keccak256_batch*, pbf_plonk_circuit_digest_bn254*,
// pbf_plonk_challenges_bn254). The _fs provers and verifiers live with their plain forms
// (prover.hip, verify.hip, verify_batch.hip) and call in here.
//
// Work split, every kernel one lane per hash chain, workgroups of one wave, the 25-lane state and
// the message in registers (no LDS):
//   k_keccak_batch       lane = message: equal-length byte strings, `pitch` apart
//   k_keccak_tree_level  lane = node: H of up to 4 consecutive 32-byte items of its tree
//   k_plonk_chain        lane = proof: P_i from its tree root, then t1 .. t6 and the six challenges
//   k_plonk_rho          lane = proof: T from the root over the t6, then rho_i
#include <cstring>
#include <vector>
#include "../../include/pbf.h"
#include "plonk_terms.hpp"
#include "prover.hpp"
#include "transcript.hpp"

using namespace pbf;

namespace {

struct FsDigest {
  uint64_t l[4];
};

__global__ void __launch_bounds__(64) k_keccak_batch(const uint8_t* __restrict__ msgs, uint64_t count, uint64_t len,
                                                     uint64_t pitch, uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  uint64_t d[4];
  keccak256_bytes(msgs + i * pitch, len, d);
#pragma unroll
  for (int k = 0; k < 4; ++k) out[4 * i + k] = d[k];
}

// out[tree mo + j] = H(in[tree m + 4 j .. min(4 j + 4, m))), mo = ceil(m / 4), j < mo
template <bool LIMBS>
__global__ void __launch_bounds__(64) k_keccak_tree_level(const uint64_t* __restrict__ in, uint64_t trees, uint64_t m,
                                                          uint64_t mo, uint64_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= trees * mo) return;
  const uint64_t tree = t / mo, j = t % mo;
  const uint32_t k = (uint32_t)(m - 4 * j < 4 ? m - 4 * j : 4);
  const uint64_t* src = in + 4 * (tree * m + 4 * j);
  uint64_t items[16];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int l = 0; l < 4; ++l) items[4 * q + l] = (uint32_t)q < k ? src[4 * q + l] : 0;
  uint64_t d[4];
  fs_tree_node<LIMBS>(items, k, d);
#pragma unroll
  for (int l = 0; l < 4; ++l) out[4 * t + l] = d[l];
}

// roots: count x 4 lanes (the tree roots over each proof's pub), or null with npub = 0
__global__ void __launch_bounds__(64) k_plonk_chain(FsDigest h0, const uint64_t* __restrict__ pts,
                                                    const uint64_t* __restrict__ f, const uint64_t* __restrict__ roots,
                                                    uint64_t npub, uint64_t count, uint64_t* __restrict__ chal,
                                                    uint64_t* __restrict__ u, uint64_t* __restrict__ t6) {
  const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  uint64_t root[4] = {0, 0, 0, 0}, P[4];
  if (npub) {
#pragma unroll
    for (int k = 0; k < 4; ++k) root[k] = roots[4 * i + k];
  }
  fs_tree_close(FS_TAG_PUB, npub, root, P);
  uint64_t c[20], uu[4], t[4];
  fs_proof_chain(h0.l, P, pts + 72 * i, f + 28 * i, c, uu, t);
#pragma unroll
  for (int k = 0; k < 20; ++k) chal[20 * i + k] = c[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) u[4 * i + k] = uu[k], t6[4 * i + k] = t[k];
}

// root: the tree root over the count digests t6 (4 lanes)
__global__ void __launch_bounds__(64) k_plonk_rho(const uint64_t* __restrict__ root, uint64_t count,
                                                  uint64_t* __restrict__ rho) {
  const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  const uint64_t r[4] = {root[0], root[1], root[2], root[3]};
  uint64_t T[4], o[4];
  fs_tree_close(FS_TAG_BATCH, count, r, T);
  fs_rho(T, i, o);
#pragma unroll
  for (int k = 0; k < 4; ++k) rho[4 * i + k] = o[k];
}

constexpr uint64_t FS_MAX_LANES = (uint64_t)0x7fffffff * 64;  // one launch: blocks of 64 below 2^31
inline uint32_t fs_blocks(uint64_t lanes) { return (uint32_t)((lanes + 63) / 64); }

}  // namespace

// ---------------------------------------------------------------- device launchers
int pbf::fs_batch_validate(uint64_t count, uint64_t npub) {
  if (count > FS_MAX_LANES || (npub + 3) / 4 > FS_MAX_LANES / count)
    return fail(PBF_EINVAL, "count x npub exceeds one launch of the transcript's tree kernel");
  return 0;
}
int pbf::fs_tree_run(pbf_ctx* ctx, const uint64_t* d_items, uint64_t trees, uint64_t m, bool limbs, uint64_t* d_roots,
                     hipStream_t s) {
  if (!trees || !m) return fail(PBF_EINVAL, "empty tree");
  if (trees * ((m + 3) / 4) > FS_MAX_LANES) return fail(PBF_EINVAL, "tree level exceeds one launch");
  DevBuf &b0 = ctx->buf("fs.tree0"), &b1 = ctx->buf("fs.tree1");
  const uint64_t m1 = (m + 3) / 4, m2 = (m1 + 3) / 4;
  int rc;
  if ((m1 > 1 && (rc = b0.ensure(trees * m1 * 32))) || (m2 > 1 && (rc = b1.ensure(trees * m2 * 32)))) return rc;
  const uint64_t* in = d_items;
  for (int level = 0;; ++level) {  // levels alternate between the two scratch buffers; the last writes d_roots
    const uint64_t mo = (m + 3) / 4;
    uint64_t* out = mo == 1 ? d_roots : (uint64_t*)(level % 2 ? b1.p : b0.p);
    if (limbs)
      hipLaunchKernelGGL(k_keccak_tree_level<true>, dim3(fs_blocks(trees * mo)), dim3(64), 0, s, in, trees, m, mo, out);
    else
      hipLaunchKernelGGL(k_keccak_tree_level<false>, dim3(fs_blocks(trees * mo)), dim3(64), 0, s, in, trees, m, mo, out);
    PBF_HIP(hipGetLastError());
    if (mo == 1) return 0;
    in = out, m = mo, limbs = false;
  }
}

int pbf::fs_batch_run(pbf_ctx* ctx, const uint64_t h0[4], uint64_t count, const uint64_t* d_pts, const uint64_t* d_f,
                      const uint64_t* d_pub, uint64_t npub, uint64_t* d_chal, uint64_t* d_u, uint64_t* d_rho,
                      hipStream_t s) {
  DevBuf &br = ctx->buf("fs.roots"), &bt = ctx->buf("fs.t6"), &bT = ctx->buf("fs.batch_root");
  int rc;
  if ((rc = br.ensure(npub ? count * 32 : 0)) || (rc = bt.ensure(count * 32)) || (rc = bT.ensure(32))) return rc;
  if (npub && (rc = fs_tree_run(ctx, d_pub, count, npub, true, (uint64_t*)br.p, s))) return rc;
  FsDigest h;
  memcpy(h.l, h0, 32);
  hipLaunchKernelGGL(k_plonk_chain, dim3(fs_blocks(count)), dim3(64), 0, s, h, d_pts, d_f,
                     npub ? (const uint64_t*)br.p : (const uint64_t*)nullptr, npub, count, d_chal, d_u, (uint64_t*)bt.p);
  PBF_HIP(hipGetLastError());
  if (!d_rho) return 0;
  if ((rc = fs_tree_run(ctx, (const uint64_t*)bt.p, 1, count, false, (uint64_t*)bT.p, s))) return rc;
  hipLaunchKernelGGL(k_plonk_rho, dim3(fs_blocks(count)), dim3(64), 0, s, (const uint64_t*)bT.p, count, d_rho);
  PBF_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- entry points
extern "C" int pbf_keccak256_batch_dev(pbf_ctx* ctx, const uint8_t* d_msgs, size_t count, size_t len, size_t pitch,
                                       uint8_t* d_out, void* stream) {
  if (!ctx || !d_out || (!d_msgs && len)) return fail(PBF_EINVAL, "null argument");
  if (count == 0 || count > FS_MAX_LANES) return fail(PBF_EINVAL, "count must be in 1 .. 2^37 - 64");
  if (pitch < len) return fail(PBF_EINVAL, "pitch below len");
  if (((uintptr_t)d_out & 7) != 0) return fail(PBF_EINVAL, "d_out must be 8-byte aligned");
  PBF_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_keccak_batch, dim3(fs_blocks(count)), dim3(64), 0, (hipStream_t)stream, d_msgs, (uint64_t)count,
                     (uint64_t)len, (uint64_t)pitch, (uint64_t*)d_out);
  PBF_HIP(hipGetLastError());
  return 0;
}

extern "C" int pbf_keccak256_batch(pbf_ctx* ctx, const uint8_t* msgs, size_t count, size_t len, size_t pitch,
                                   uint8_t* out) {
  if (!ctx || !out || (!msgs && len)) return fail(PBF_EINVAL, "null argument");
  if (count == 0 || count > FS_MAX_LANES) return fail(PBF_EINVAL, "count must be in 1 .. 2^37 - 64");
  if (pitch < len) return fail(PBF_EINVAL, "pitch below len");
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  DevBuf &bm = ctx->buf("fs.msgs"), &bo = ctx->buf("fs.digests");
  const size_t bytes = len ? (count - 1) * pitch + len : 0;  // the last message ends at its len
  int rc;
  if ((rc = bm.ensure(bytes ? bytes : 8)) || (rc = bo.ensure(count * 32))) return rc;
  if (bytes) PBF_HIP(hipMemcpyAsync(bm.p, msgs, bytes, hipMemcpyHostToDevice, s));
  if ((rc = pbf_keccak256_batch_dev(ctx, (const uint8_t*)bm.p, count, len, pitch, (uint8_t*)bo.p, s))) return rc;
  PBF_HIP(hipMemcpyAsync(out, bo.p, count * 32, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  return 0;
}

extern "C" int pbf_plonk_circuit_digest_bn254_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                                  const uint64_t* d_srs, size_t srs_m, const uint64_t* g2,
                                                  const uint64_t* k1k2, int mode, size_t npub, uint8_t* digest,
                                                  void* stream) {
  int rc, ok = 0;
  if ((rc = verifier_shape({ctx, d_q, d_copies, d_srs, g2, k1k2, digest}, n, srs_m, &ok))) return rc;
  if (npub > n) return fail(PBF_EINVAL, "more public inputs than gates");
  PBF_HIP(hipSetDevice(ctx->device));
  uint64_t pre[8][8], h0[4];
  if ((rc = verifier_vk(ctx, n, plonk_domain(n).omega, d_q, d_copies, d_srs, srs_m, k1k2, (hipStream_t)stream, pre)))
    return rc;
  fs_circuit_digest(mode, n, npub, k1k2, pre, g2, h0);
  memcpy(digest, h0, 32);
  return 0;
}

extern "C" int pbf_plonk_circuit_digest_bn254(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                              const uint64_t* srs, size_t srs_m, const uint64_t* g2,
                                              const uint64_t* k1k2, int mode, size_t npub, uint8_t* digest) {
  int rc, ok = 0;  // every argument error before the uploads
  if ((rc = verifier_shape({ctx, q, copies, srs, g2, k1k2, digest}, n, srs_m, &ok))) return rc;
  if (npub > n) return fail(PBF_EINVAL, "more public inputs than gates");
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  const uint64_t *d_q, *d_copies, *d_srs;
  if ((rc = verifier_upload(ctx, n, q, copies, srs, srs_m, s, &d_q, &d_copies, &d_srs))) return rc;
  return pbf_plonk_circuit_digest_bn254_dev(ctx, n, d_q, d_copies, d_srs, srs_m, g2, k1k2, mode, npub, digest, s);
}

extern "C" int pbf_plonk_challenges_bn254(pbf_ctx* ctx, const uint8_t* digest, size_t count, const uint64_t* proof_pts,
                                          const uint64_t* proof_f, const uint64_t* pub, size_t npub, uint64_t* chal,
                                          uint64_t* u, uint64_t* rho) {
  if (!ctx || !digest || !proof_pts || !proof_f || !chal || !u) return fail(PBF_EINVAL, "null argument");
  if (count == 0 || count > ((size_t)1 << 20)) return fail(PBF_EINVAL, "count must be in 1 .. 2^20");
  if (npub && !pub) return fail(PBF_EINVAL, "null pub with npub > 0");
  if (npub > ((size_t)1 << 26)) return fail(PBF_EINVAL, "more public inputs than any circuit has gates");
  if (npub && !fr_canonical(pub, count * npub)) return fail(PBF_EINVAL, "public input not canonical");
  int rc;
  if ((rc = fs_batch_validate(count, npub))) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  const size_t c = count;
  DevBuf &bp = ctx->buf("fs.pts"), &bf = ctx->buf("fs.f"), &bpub = ctx->buf("fs.pub"), &bc = ctx->buf("fs.chal"),
         &bu = ctx->buf("fs.u"), &br = ctx->buf("fs.rho");
  if ((rc = bp.ensure(9 * c * 64)) || (rc = bf.ensure(7 * c * 32)) || (rc = bpub.ensure(c * npub * 32)) ||
      (rc = bc.ensure(5 * c * 32)) || (rc = bu.ensure(c * 32)) || (rc = br.ensure(c * 32)))
    return rc;
  PBF_HIP(hipMemcpyAsync(bp.p, proof_pts, 9 * c * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(bf.p, proof_f, 7 * c * 32, hipMemcpyHostToDevice, s));
  if (npub) PBF_HIP(hipMemcpyAsync(bpub.p, pub, c * npub * 32, hipMemcpyHostToDevice, s));
  uint64_t h0[4];
  memcpy(h0, digest, 32);
  if ((rc = fs_batch_run(ctx, h0, c, (const uint64_t*)bp.p, (const uint64_t*)bf.p,
                         npub ? (const uint64_t*)bpub.p : nullptr, npub, (uint64_t*)bc.p, (uint64_t*)bu.p,
                         rho ? (uint64_t*)br.p : nullptr, s)))
    return rc;
  PBF_HIP(hipMemcpyAsync(chal, bc.p, 5 * c * 32, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipMemcpyAsync(u, bu.p, c * 32, hipMemcpyDeviceToHost, s));
  if (rho) PBF_HIP(hipMemcpyAsync(rho, br.p, c * 32, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  return 0;
}
