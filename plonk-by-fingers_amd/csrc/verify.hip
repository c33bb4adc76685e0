// Plonk::verify over BN254 (src/plonk.rs:468-650): the single-proof verifier and the verification
// key it shares with the batched verifier (verify_batch.hip). No kernel lives here: the key's
// sigma labels come from the prover's launcher (prover.hpp sigma_table_run), the public inputs'
// sum from the batched verifier's (plonk_pi_fraction_run), everything else is
// host Fr arithmetic, the Fr INTT, two MSMs and one pairing check.
#include <cstring>
#include <vector>
#include "../../include/pbf.h"
#include "prover.hpp"

using namespace pbf;

static int verify_with_vk(pbf_ctx* ctx, size_t n, const U256& omega, const uint64_t (*pre)[8], const uint64_t* d_srs,
                          const uint64_t* g2, const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* chal,
                          const uint64_t* u_in, const uint64_t* k1k2, int mode, const U256* pi_nd, int* ok,
                          hipStream_t s);

// Plonk::verify (src/plonk.rs:468-650). srs: >= n affine G1 points (g1s, device), g2: [g2_1, g2_s]
// (2 x 16 u64, host); proof as pbf_plonk_prove_bn254 returns it; u the verifier's random
// scalar (rand[0], plonk.rs:519). mode 0 keeps step 7's t_z (plonk.rs:575-581, no alpha on
// the permutation term), mode 1 the paper's. *ok = 1 iff e(E1, [s]G2) == e(E2, G2).
// pub, npub: the public inputs of pbf_plonk_verify_bn254_pi* (host; none: null, 0)
static int verify_dev(pbf_ctx* ctx, size_t n, const uint64_t* d_q, const uint64_t* d_copies, const uint64_t* d_srs,
                      size_t srs_m, const uint64_t* g2, const uint64_t* proof_pts, const uint64_t* proof_f,
                      const uint64_t* pub, size_t npub, const uint64_t* chal, const uint64_t* u_in, const uint64_t* k1k2,
                      int mode, int* ok, void* stream) {
  if (!ctx || !d_q || !d_copies || !d_srs || !g2 || !proof_pts || !proof_f || !chal || !u_in || !k1k2 || !ok)
    return fail(PBF_EINVAL, "null argument");
  *ok = 0;
  if (n < 8 || (n & (n - 1))) return fail(PBF_EINVAL, "n must be a power of two >= 8");
  if (srs_m < n) return fail(PBF_EINVAL, "SRS too short");
  int rc;
  if ((rc = plonk_pub_validate(n, pub, npub, 1))) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  uint32_t log_n = 0;
  while ((1ull << log_n) < n) ++log_n;
  hipStream_t s = (hipStream_t)stream;
  // Step 1-2: proof points on the curve, proof fields canonical (plonk.rs:523-547)
  for (int i = 0; i < 9; ++i)
    if (!on_curve(proof_pts + 8 * i)) return 0;
  for (int i = 0; i < 7; ++i)
    if (Fr::geq_p(u256_from_u64(proof_f + 4 * i))) return 0;
  const U256 omega = fr_root_of_unity(log_n);
  uint64_t pre[8][8];
  if ((rc = verifier_vk(ctx, n, omega, d_q, d_copies, d_srs, srs_m, k1k2, s, pre))) return rc;
  // public inputs: sum_j pub_j w^j / (z - w^j) as a fraction (N, D), from the batched verifier's
  // kernels with count = 1
  U256 nd[2];
  if (npub) {
    DevBuf &dp = ctx->buf("vf.pub"), &dz = ctx->buf("vf.pichal"), &dn = ctx->buf("vf.pind");
    if ((rc = dp.ensure(npub * 32)) || (rc = dz.ensure(5 * 32)) || (rc = dn.ensure(64))) return rc;
    PBF_HIP(hipMemcpyAsync(dp.p, pub, npub * 32, hipMemcpyHostToDevice, s));
    PBF_HIP(hipMemcpyAsync(dz.p, chal, 5 * 32, hipMemcpyHostToDevice, s));
    if ((rc = plonk_pi_fraction_run(ctx, omega, (const uint64_t*)dp.p, npub, (const uint64_t*)dz.p, 1, (uint64_t*)dn.p, s)))
      return rc;
    uint64_t h[8];
    PBF_HIP(hipMemcpyAsync(h, dn.p, sizeof(h), hipMemcpyDeviceToHost, s));
    PBF_HIP(hipStreamSynchronize(s));
    nd[0] = u256_from_u64(h);  // Montgomery form as stored
    nd[1] = u256_from_u64(h + 4);
  }
  return verify_with_vk(ctx, n, omega, pre, d_srs, g2, proof_pts, proof_f, chal, u_in, k1k2, mode, npub ? nd : nullptr,
                        ok, s);
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
static int verify_with_vk(pbf_ctx* ctx, size_t n, const U256& omega, const uint64_t (*pre)[8], const uint64_t* d_srs,
                          const uint64_t* g2, const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* chal,
                          const uint64_t* u_in, const uint64_t* k1k2, int mode, const U256* pi_nd, int* ok,
                          hipStream_t s) {
  const U256 one = fr_one_m();
  const U256 k1 = hm(k1k2), k2 = hm(k1k2 + 4);
  int rc;
  const U256 alpha = hm(chal), beta = hm(chal + 4), gamma = hm(chal + 8), zc = hm(chal + 12), v = hm(chal + 16);
  const U256 u = hm(u_in);
  const U256 a_z = hm(proof_f), b_z = hm(proof_f + 4), c_z = hm(proof_f + 8), s1_z = hm(proof_f + 12),
             s2_z = hm(proof_f + 16), r_z = hm(proof_f + 20), zw_z = hm(proof_f + 24);
  // Step 4-5: Z_H(z) = z^n - 1, L_1(z) = n^-1 sum_{i<n} z^i (the interpolated Lagrange poly)
  const U256 zn = fr_pow(zc, n);
  const U256 z_h_z = Fr::sub(zn, one);
  U256 l1 = u256_zero(), zp = one;
  for (uint64_t i = 0; i < n && i < 64; ++i) { l1 = Fr::add(l1, zp); zp = Fr::mul(zp, zc); }
  if (n > 64) {  // geometric sum (z^n - 1)/(z - 1) for z != 1
    const U256 zm1 = Fr::sub(zc, one);
    l1 = Fr::is_zero(zm1) ? hm64(n) : Fr::mul(z_h_z, fr_inv(zm1));
  }
  l1 = Fr::mul(l1, fr_inv(hm64(n)));
  if (Fr::is_zero(z_h_z)) return 0;  // the reference's .unwrap() would panic (plonk.rs:581)
  // Step 7: t_z
  const U256 alpha2 = Fr::mul(alpha, alpha);
  U256 perm = Fr::mul(Fr::mul(Fr::add(Fr::add(a_z, Fr::mul(beta, s1_z)), gamma),
                              Fr::add(Fr::add(b_z, Fr::mul(beta, s2_z)), gamma)),
                      Fr::mul(Fr::add(c_z, gamma), zw_z));
  if (mode == 1) perm = Fr::mul(perm, alpha);
  U256 rpi_z = r_z;  // r_z + PI(z), PI(z) = -Z_H(z) n^-1 N / D (D != 0: z is not in H here)
  if (pi_nd) rpi_z = Fr::sub(r_z, Fr::mul(Fr::mul(Fr::mul(z_h_z, fr_inv(hm64(n))), pi_nd[0]), fr_inv(pi_nd[1])));
  const U256 t_z = Fr::mul(Fr::sub(Fr::sub(rpi_z, perm), Fr::mul(l1, alpha2)), fr_inv(z_h_z));
  // Steps 8-10 as one linear combination of points (bases / scalars)
  U256 vp[7];
  vp[0] = one;
  for (int i = 1; i < 7; ++i) vp[i] = Fr::mul(vp[i - 1], v);
  const U256 d2 = Fr::add(Fr::add(Fr::mul(Fr::mul(Fr::mul(Fr::mul(Fr::mul(Fr::add(Fr::add(a_z, Fr::mul(beta, zc)), gamma),
      Fr::add(Fr::add(b_z, Fr::mul(Fr::mul(beta, k1), zc)), gamma)), Fr::add(Fr::add(c_z, Fr::mul(Fr::mul(beta, k2), zc)), gamma)),
      alpha), v), one), Fr::mul(Fr::mul(l1, alpha2), v)), u);
  const U256 d3 = Fr::mul(Fr::mul(Fr::mul(Fr::mul(Fr::mul(Fr::add(Fr::add(a_z, Fr::mul(beta, s1_z)), gamma),
      Fr::add(Fr::add(b_z, Fr::mul(beta, s2_z)), gamma)), alpha), v), beta), zw_z);
  U256 ecoef = Fr::add(t_z, Fr::mul(v, r_z));
  ecoef = Fr::add(ecoef, Fr::mul(vp[2], a_z));
  ecoef = Fr::add(ecoef, Fr::mul(vp[3], b_z));
  ecoef = Fr::add(ecoef, Fr::mul(vp[4], c_z));
  ecoef = Fr::add(ecoef, Fr::mul(vp[5], s1_z));
  ecoef = Fr::add(ecoef, Fr::mul(vp[6], s2_z));
  ecoef = Fr::add(ecoef, Fr::mul(u, zw_z));
  const U256 omega_m = omega;
  // bases: proof a b c z t_lo t_mid t_hi w_z w_zw | q_m q_l q_r q_o q_c s1 s2 s3 | G
  std::vector<uint64_t> bases(18 * 8), sc(18 * 4);
  for (int i = 0; i < 9; ++i) memcpy(&bases[8 * i], proof_pts + 8 * i, 64);
  for (int k = 0; k < 8; ++k) memcpy(&bases[8 * (9 + k)], pre[k], 64);
  std::vector<uint64_t> g0(8);
  PBF_HIP(hipMemcpyAsync(g0.data(), d_srs, 64, hipMemcpyDeviceToHost, s));
  PBF_HIP(hipStreamSynchronize(s));
  memcpy(&bases[8 * 17], g0.data(), 64);
  U256 scal[18];
  scal[0] = vp[2];                                       // a_s
  scal[1] = vp[3];                                       // b_s
  scal[2] = vp[4];                                       // c_s
  scal[3] = d2;                                          // z_s
  scal[4] = one;                                         // t_lo
  scal[5] = fr_pow(zc, n + 2);                           // t_mid
  scal[6] = fr_pow(zc, 2 * n + 4);                       // t_hi
  scal[7] = zc;                                          // w_z * z
  scal[8] = Fr::mul(Fr::mul(u, zc), omega_m);            // w_zw * u z w
  scal[9] = Fr::mul(Fr::mul(a_z, b_z), v);               // q_m
  scal[10] = Fr::mul(a_z, v);                            // q_l
  scal[11] = Fr::mul(b_z, v);                            // q_r
  scal[12] = Fr::mul(c_z, v);                            // q_o
  scal[13] = v;                                          // q_c
  scal[14] = vp[5];                                      // s1
  scal[15] = vp[6];                                      // s2
  scal[16] = Fr::sub(u256_zero(), d3);                   // - s3 d3
  scal[17] = Fr::sub(u256_zero(), ecoef);                // - E
  for (int i = 0; i < 18; ++i) hout(&sc[4 * i], scal[i]);
  DevBuf &db = ctx->buf("vf.bases"), &ds = ctx->buf("vf.scalars");
  if ((rc = db.ensure(18 * 64)) || (rc = ds.ensure(18 * 32))) return rc;
  PBF_HIP(hipMemcpyAsync(db.p, bases.data(), 18 * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(ds.p, sc.data(), 18 * 32, hipMemcpyHostToDevice, s));
  uint64_t e2[8], e1[8];
  if ((rc = pbf_msm_g1_bn254_dev(ctx, (const uint64_t*)db.p, (const uint64_t*)ds.p, 18, e2, s))) return rc;
  // E1 = w_z + u w_zw
  U256 one_u[2] = {one, u};
  std::vector<uint64_t> sc1(8);
  hout(&sc1[0], one_u[0]);
  hout(&sc1[4], one_u[1]);
  PBF_HIP(hipMemcpyAsync(db.p, proof_pts + 8 * 7, 2 * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(ds.p, sc1.data(), 2 * 32, hipMemcpyHostToDevice, s));
  if ((rc = pbf_msm_g1_bn254_dev(ctx, (const uint64_t*)db.p, (const uint64_t*)ds.p, 2, e1, s))) return rc;
  // e(E1, [s]G2) == e(E2, G2)  <=>  e(E1, [s]G2) e(-E2, G2) == 1  (plonk.rs:646-650)
  uint64_t g1s[16], g2s[32];
  memcpy(g1s, e1, 64);
  neg_g1(e2, g1s + 8);
  memcpy(g2s, g2 + 16, 128);  // [s]G2
  memcpy(g2s + 16, g2, 128);  // G2
  return pairing_check_on_stream(ctx, g1s, g2s, 2, ok, s);
}

extern "C" int pbf_plonk_verify_bn254(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                      const uint64_t* srs, size_t srs_m, const uint64_t* g2, const uint64_t* proof_pts,
                                      const uint64_t* proof_f, const uint64_t* chal, const uint64_t* u,
                                      const uint64_t* k1k2, int mode, int* ok) {
  return pbf_plonk_verify_bn254_pi(ctx, n, q, copies, srs, srs_m, g2, proof_pts, proof_f, nullptr, 0, chal, u, k1k2, mode,
                                   ok);
}

extern "C" int pbf_plonk_verify_bn254_pi(pbf_ctx* ctx, size_t n, const uint64_t* q, const uint64_t* copies,
                                         const uint64_t* srs, size_t srs_m, const uint64_t* g2,
                                         const uint64_t* proof_pts, const uint64_t* proof_f, const uint64_t* pub,
                                         size_t npub, const uint64_t* chal, const uint64_t* u, const uint64_t* k1k2,
                                         int mode, int* ok) {
  if (!ctx || !q || !copies || !srs) return fail(PBF_EINVAL, "null argument");
  int rc0 = plonk_pub_validate(n, pub, npub, 1);  // before the uploads
  if (rc0) return rc0;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  DevBuf &dq = ctx->buf("vf.q"), &dc = ctx->buf("vf.copies"), &dsrs = ctx->buf("vf.srs");
  int rc;
  if ((rc = dq.ensure(5 * n * 32)) || (rc = dc.ensure(3 * n * 16)) || (rc = dsrs.ensure(srs_m * 64))) return rc;
  PBF_HIP(hipMemcpyAsync(dq.p, q, 5 * n * 32, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(dc.p, copies, 3 * n * 16, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(dsrs.p, srs, srs_m * 64, hipMemcpyHostToDevice, s));
  return verify_dev(ctx, n, (const uint64_t*)dq.p, (const uint64_t*)dc.p, (const uint64_t*)dsrs.p, srs_m, g2, proof_pts,
                    proof_f, pub, npub, chal, u, k1k2, mode, ok, s);
}
