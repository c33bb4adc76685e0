// Plonk::verify over BN254 (src/plonk.rs:468-650): the single-proof verifier and the verification
// key it shares with the batched verifier (verify_batch.hip). No kernel lives here: the key's
// sigma labels come from the prover's launcher (prover.hpp sigma_table_run), the public inputs'
// sum from the batched verifier's (plonk_pi_fraction_run), the 18 + 2 scalars of steps 4-10 from
// plonk_verifier_scalars (plonk_terms.hpp, the batched kernel's formulas run on the host with
// rho = 1); the rest is the Fr INTT, two MSMs and one pairing check.
#include <cstring>
#include <vector>
#include "../../include/pbf.h"
#include "plonk_terms.hpp"
#include "prover.hpp"
#include "transcript.hpp"

using namespace pbf;

static int verify_with_vk(pbf_ctx* ctx, const PlonkDomain& dom, const uint64_t (*pre)[8], const uint64_t* d_srs,
                          const uint64_t* g2, const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* chal,
                          const uint64_t* u_in, const uint64_t* k1k2, int mode, const uint64_t* pi_nd, int* ok,
                          hipStream_t s);

// Plonk::verify (src/plonk.rs:468-650). srs: >= n affine G1 points (g1s, device), g2: [g2_1, g2_s]
// (2 x 16 u64, host); proof as pbf_plonk_prove_bn254 returns it; u the verifier's random
// scalar (rand[0], plonk.rs:519). mode 0 keeps step 7's t_z (plonk.rs:575-581, no alpha on
// the permutation term), mode 1 the paper's. *ok = 1 iff e(E1, [s]G2) == e(E2, G2).
// pub, npub: the public inputs of pbf_plonk_verify_bn254_pi* (host; none: null, 0)
// fs (pbf_plonk_verify_bn254_fs*): chal and u_in are null; the five challenges and u come from the
// transcript (transcript.hpp) of the key's circuit digest, pub and the proof, derived on the host
static int verify_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies, const uint64_t* d_srs,
                      size_t srs_m, const uint64_t* g2, const uint64_t* proof_pts, const uint64_t* proof_f,
                      const uint64_t* pub, size_t npub, const uint64_t* chal, const uint64_t* u_in, const uint64_t* k1k2,
                      int mode, int* ok, void* stream, bool fs = false) {
  int rc;
  if ((rc = verifier_shape({ctx, d_q, d_copies, d_srs, g2, proof_pts, proof_f, k1k2}, n, srs_m, ok)) ||
      (rc = plonk_pub_validate(n, pub, npub, 1)))
    return rc;
  if (!fs && (!chal || !u_in)) return fail(PBF_EINVAL, "null argument");
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  // Step 1-2: proof points on the curve, proof fields canonical (plonk.rs:523-547)
  for (int i = 0; i < 9; ++i)
    if (!on_curve(proof_pts + 8 * i)) return 0;
  for (int i = 0; i < 7; ++i)
    if (Fr::geq_p(u256_from_u64(proof_f + 4 * i))) return 0;
  const PlonkDomain dom = plonk_domain(n);
  uint64_t pre[8][8];
  if ((rc = verifier_vk(ctx, n, dom.omega, d_q, d_copies, d_srs, srs_m, k1k2, s, pre))) return rc;
  uint64_t fs_chal[24];  // alpha beta gamma z v, u
  if (fs) {
    uint64_t h0[4], P[4], t6[4];
    fs_circuit_digest(mode, n, npub, k1k2, pre, g2, h0);
    fs_tree_digest_host(FS_TAG_PUB, pub, npub, P);
    fs_proof_chain(h0, P, proof_pts, proof_f, fs_chal, fs_chal + 20, t6);
    chal = fs_chal;
    u_in = fs_chal + 20;
  }
  // public inputs: sum_j pub_j w^j / (z - w^j) as a fraction (N, D), from the batched verifier's
  // kernels with count = 1
  uint64_t nd[8];  // Montgomery form as stored
  if (npub) {
    DevBuf &dp = ctx->buf("vf.pub"), &dz = ctx->buf("vf.pichal"), &dn = ctx->buf("vf.pind");
    if ((rc = dp.ensure(npub * 32)) || (rc = dz.ensure(5 * 32)) || (rc = dn.ensure(64))) return rc;
    PBF_HIP(hipMemcpyAsync(dp.p, pub, npub * 32, hipMemcpyHostToDevice, s));
    PBF_HIP(hipMemcpyAsync(dz.p, chal, 5 * 32, hipMemcpyHostToDevice, s));
    if ((rc = plonk_pi_fraction_run(ctx, dom.omega, (const uint64_t*)dp.p, npub, (const uint64_t*)dz.p, 1,
                                    (uint64_t*)dn.p, s)))
      return rc;
    PBF_HIP(hipMemcpyAsync(nd, dn.p, sizeof(nd), hipMemcpyDeviceToHost, s));
    PBF_HIP(hipStreamSynchronize(s));
  }
  return verify_with_vk(ctx, dom, pre, d_srs, g2, proof_pts, proof_f, chal, u_in, k1k2, mode, npub ? nd : nullptr, ok, s);
}

extern "C" int pbf_plonk_verify_bn254_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                          const uint64_t* d_srs, size_t srs_m, const uint64_t* g2,
                                          const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* chal,
                                          const uint64_t* u_in, const uint64_t* k1k2, int mode, int* ok, void* stream) {
  return verify_dev(ctx, n, d_q, d_copies, d_srs, srs_m, g2, proof_pts, proof_f, nullptr, 0, chal, u_in, k1k2, mode, ok,
                    stream);
}

extern "C" int pbf_plonk_verify_bn254_pi_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                             const uint64_t* d_srs, size_t srs_m, const uint64_t* g2,
                                             const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* pub,
                                             size_t npub, const uint64_t* chal, const uint64_t* u_in,
                                             const uint64_t* k1k2, int mode, int* ok, void* stream) {
  return verify_dev(ctx, n, d_q, d_copies, d_srs, srs_m, g2, proof_pts, proof_f, pub, npub, chal, u_in, k1k2, mode, ok,
                    stream);
}

// Plonk::verify's preprocessing, shared by the single and the batched verifier
// (verify_batch.hip): pre = the commitments of q_m q_l q_r q_o q_c s_sigma_1..3; omega =
// fr_root_of_unity(log2 n).
int pbf::verifier_vk(pbf_ctx* ctx, size_t n, const U256& omega, const uint64_t* d_q, const uint64_t* d_copies,
                     const uint64_t* d_srs, size_t srs_m, const uint64_t* k1k2, hipStream_t s, uint64_t pre[8][8]) {
  const uint64_t E = 32;
  int rc;
  // preprocessing (plonk.rs:507-517): commitments of q_m q_l q_r q_o q_c, s_sigma_1..3 -- a
  // verification key: kept in the context for this circuit and SRS (q, copies and the SRS
  // compared with device copies of the ones it was built from on every call;
  // option verifier.vk = 0 recomputes them, as the reference does)
  const U256 k1 = hm(k1k2), k2 = hm(k1k2 + 4);
  std::vector<uint64_t> vk_key;
  const bool vk_on = ctx->options.num("verifier.vk", 1) != 0;
  if (vk_on) {
    const SnapItem items[3] = {{"q", d_q, 20 * (uint64_t)n},
                               {"copies", d_copies, 6 * (uint64_t)n},
                               {"g1pts", d_srs, 8 * (uint64_t)srs_m}};
    bool same = false;
    if ((rc = snapshot_check(ctx, "vk", items, 3, s, &same))) return rc;
    if (!same) ctx->vk_key.clear();  // rebuilt below; valid again once complete
    vk_key = {(uint64_t)n, (uint64_t)srs_m};
    for (int i = 0; i < 8; ++i) vk_key.push_back(k1k2[i]);
  }
  if (vk_on && ctx->vk_key == vk_key && ctx->vk_pts.size() == 64) {
    memcpy(pre, ctx->vk_pts.data(), 64 * sizeof(uint64_t));
  } else {
  DevBuf &hp = ctx->buf("vf.hpow"), &sg = ctx->buf("vf.sigma"), &cf = ctx->buf("vf.coef"), &fl = ctx->buf("vf.flag");
  if ((rc = hp.ensure(n * E)) || (rc = sg.ensure(3 * n * E)) || (rc = cf.ensure(8 * n * E)) || (rc = fl.ensure(64)))
    return rc;
  uint64_t w_plain[4];
  hout(w_plain, omega);
  PBF_HIP(hipMemsetAsync(fl.p, 0, sizeof(int), s));
  if ((rc = sigma_table_run(n, omega, k1, k2, d_copies, (uint64_t*)hp.p, (uint64_t*)sg.p, (int*)fl.p, s))) return rc;
  uint64_t* c = (uint64_t*)cf.p;
  // slots: 0 q_m 1 q_l 2 q_r 3 q_o 4 q_c 5 s1 6 s2 7 s3  (q columns: q_l q_r q_o q_m q_c)
  const int qcol[5] = {3, 0, 1, 2, 4};
  for (int k = 0; k < 5; ++k)
    PBF_HIP(hipMemcpyAsync(c + 4 * n * k, d_q + 4 * n * qcol[k], n * E, hipMemcpyDeviceToDevice, s));
  PBF_HIP(hipMemcpyAsync(c + 4 * n * 5, sg.p, 3 * n * E, hipMemcpyDeviceToDevice, s));
  if ((rc = pbf_ntt_fr256_batch_dev(ctx, w_plain, c, c, n, 8, 1, s))) return rc;
  const Affine* tbl = nullptr;  // the SRS window table, when a prove on this context built it
  if ((rc = msm_fixed_lookup(ctx, d_srs, srs_m, s, &tbl))) return rc;
  if (tbl) {
    DevBuf& vs = ctx->buf("vf.commits");
    if ((rc = vs.ensure(8 * sizeof(Xyzz)))) return rc;
    for (int k = 0; k < 8; ++k)
      if ((rc = msm_fixed_device(ctx, tbl, srs_m, 0, c + 4 * n * k, n, s, (Xyzz*)vs.p + k))) return rc;
    if ((rc = msm_fixed_wait(ctx, s))) return rc;
    Xyzz h[8];
    PBF_HIP(hipMemcpyAsync(h, vs.p, sizeof(h), hipMemcpyDeviceToHost, s));
    PBF_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < 8; ++k) xyzz_to_affine_u64(h[k], pre[k]);
  } else {
    for (int k = 0; k < 8; ++k)
      if ((rc = pbf_msm_g1_bn254_dev(ctx, d_srs, c + 4 * n * k, n, pre[k], s))) return rc;
  }
  int bad = 0;
  PBF_HIP(hipMemcpyAsync(&bad, fl.p, sizeof(int), hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  if (bad) return fail(PBF_EINVAL, "bad copy constraint label");
  if (vk_on) {
    ctx->vk_key = vk_key;
    ctx->vk_pts.assign(&pre[0][0], &pre[0][0] + 64);
  }
  }
  return 0;
}

// Plonk::verify steps 4-12 for one proof whose points and fields passed steps 1-2. pi_nd: null, or
// the public inputs' fraction (N, D) of plonk_pi_fraction_run: step 7 then takes r_z + PI(z)
static int verify_with_vk(pbf_ctx* ctx, const PlonkDomain& dom, const uint64_t (*pre)[8], const uint64_t* d_srs,
                          const uint64_t* g2, const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* chal,
                          const uint64_t* u_in, const uint64_t* k1k2, int mode, const uint64_t* pi_nd, int* ok,
                          hipStream_t s) {
  int rc;
  const PlonkChallenges ch{hm(chal), hm(chal + 4), hm(chal + 8), hm(chal + 12), hm(chal + 16), hm(k1k2), hm(k1k2 + 4)};
  PlonkEvals e;  // Proof order: a b c s1 s2 r zw
  e.a_z = hm(proof_f), e.b_z = hm(proof_f + 4), e.c_z = hm(proof_f + 8), e.s1_z = hm(proof_f + 12);
  e.s2_z = hm(proof_f + 16), e.r_z = hm(proof_f + 20), e.zw_z = hm(proof_f + 24);
  const PlonkVerifierArgs g{hm(u_in), fr_one_m(), dom, mode};
  // Steps 4-10 as two linear combinations of points: sc on the 18 bases of E2, then 1, u on W_z, W_zw
  // bases: proof a b c z t_lo t_mid t_hi w_z w_zw | q_m q_l q_r q_o q_c s1 s2 s3 | G
  uint64_t bases[18 * 8], sc[20 * 4];
  const auto store = [&](int j, const U256& m) { hout(sc + 4 * (j < 9 ? j : j < 11 ? j + 9 : j - 2), m); };
  // Z_H(z) = 0: the reference's .unwrap() would panic (plonk.rs:581)
  if (!plonk_verifier_scalars(ch, e, g, pi_nd, store)) return 0;
  memcpy(bases, proof_pts, 9 * 64);
  memcpy(bases + 8 * 9, pre, 8 * 64);
  PBF_HIP(hipMemcpyAsync(bases + 8 * 17, d_srs, 64, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  DevBuf &db = ctx->buf("vf.bases"), &ds = ctx->buf("vf.scalars");
  if ((rc = db.ensure(18 * 64)) || (rc = ds.ensure(18 * 32))) return rc;
  PBF_HIP(hipMemcpyAsync(db.p, bases, 18 * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(ds.p, sc, 18 * 32, hipMemcpyHostToDevice, s));
  uint64_t e2[8], e1[8];
  if ((rc = pbf_msm_g1_bn254_dev(ctx, (const uint64_t*)db.p, (const uint64_t*)ds.p, 18, e2, s))) return rc;
  // E1 = w_z + u w_zw
  PBF_HIP(hipMemcpyAsync(db.p, proof_pts + 8 * 7, 2 * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(ds.p, sc + 4 * 18, 2 * 32, hipMemcpyHostToDevice, s));
  if ((rc = pbf_msm_g1_bn254_dev(ctx, (const uint64_t*)db.p, (const uint64_t*)ds.p, 2, e1, s))) return rc;
  return pairing_tail(ctx, e1, e2, g2, ok, s);  // e(E1, [s]G2) == e(E2, G2)
}

extern "C" int pbf_plonk_verify_bn254(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                      const uint64_t* srs, size_t srs_m, const uint64_t* g2, const uint64_t* proof_pts,
                                      const uint64_t* proof_f, const uint64_t* chal, const uint64_t* u,
                                      const uint64_t* k1k2, int mode, int* ok) {
  return pbf_plonk_verify_bn254_pi(ctx, n, q, copies, srs, srs_m, g2, proof_pts, proof_f, nullptr, 0, chal, u, k1k2, mode,
                                   ok);
}

// the host forms: every argument error before the uploads
static int verify_host(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies, const uint64_t* srs,
                       size_t srs_m, const uint64_t* g2, const uint64_t* proof_pts, const uint64_t* proof_f,
                       const uint64_t* pub, size_t npub, const uint64_t* chal, const uint64_t* u, const uint64_t* k1k2,
                       int mode, int* ok, bool fs) {
  int rc;
  if ((rc = verifier_shape({ctx, q, copies, srs, g2, proof_pts, proof_f, k1k2}, n, srs_m, ok)) ||
      (rc = plonk_pub_validate(n, pub, npub, 1)))
    return rc;
  if (!fs && (!chal || !u)) return fail(PBF_EINVAL, "null argument");
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  const uint64_t *d_q, *d_copies, *d_srs;
  if ((rc = verifier_upload(ctx, n, q, copies, srs, srs_m, s, &d_q, &d_copies, &d_srs))) return rc;
  return verify_dev(ctx, n, d_q, d_copies, d_srs, srs_m, g2, proof_pts, proof_f, pub, npub, chal, u, k1k2, mode, ok, s,
                    fs);
}

extern "C" int pbf_plonk_verify_bn254_pi(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                         const uint64_t* srs, size_t srs_m, const uint64_t* g2,
                                         const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* pub,
                                         size_t npub, const uint64_t* chal, const uint64_t* u, const uint64_t* k1k2,
                                         int mode, int* ok) {
  return verify_host(ctx, n, q, copies, srs, srs_m, g2, proof_pts, proof_f, pub, npub, chal, u, k1k2, mode, ok, false);
}

// Fiat-Shamir (pbf.h): no chal, no u
extern "C" int pbf_plonk_verify_bn254_fs(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                         const uint64_t* srs, size_t srs_m, const uint64_t* g2,
                                         const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* pub,
                                         size_t npub, const uint64_t* k1k2, int mode, int* ok) {
  return verify_host(ctx, n, q, copies, srs, srs_m, g2, proof_pts, proof_f, pub, npub, nullptr, nullptr, k1k2, mode, ok,
                     true);
}

extern "C" int pbf_plonk_verify_bn254_fs_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies,
                                             const uint64_t* d_srs, size_t srs_m, const uint64_t* g2,
                                             const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* pub,
                                             size_t npub, const uint64_t* k1k2, int mode, int* ok, void* stream) {
  return verify_dev(ctx, n, d_q, d_copies, d_srs, srs_m, g2, proof_pts, proof_f, pub, npub, nullptr, nullptr, k1k2, mode,
                    ok, stream, true);
}
