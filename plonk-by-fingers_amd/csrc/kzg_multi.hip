// Multi-point KZG openings over BN254 on gfx950 (include/pbf.h "Multi-point KZG openings"): the
// scheme of Boneh, Drake, Fisch and Gabizon, "Efficient polynomial commitment schemes for multiple
// points and polynomials" (2020), section 4. `batch` polynomials p_b, each opened on its own
// subset S_b of the point set T; two G1 points prove all of it.
//
//   open     y[b][j] = p_b(t_j) for j in S_b, W = commit(h), h = sum_b gamma^b (p_b - r_b) / Z_{S_b}.
//            The polynomials are grouped by equal set: h = sum over distinct S of quot(c_S, Z_S),
//            c_S = sum_{b: S_b = S} gamma^b p_b (the quotient does not depend on the subtracted
//            r_b, as in kzg.hip), and by partial fractions
//              quot(c, Z_S) = sum_{j in S} lambda_j quot(c, x - t_j),  lambda_j = 1 / prod_{m != j} (t_j - t_m):
//            |S| runs of the recurrence of k_hs1..3 over one read of c_S, summed into h (k_kzm_div1..3)
//   finish   W' = commit(quot(sum_b gamma^b Z_{T \ S_b}(z) p_b - Z_T(z) h, x - z)): h again (the call is
//            stateless), one weighted sum, one linear combination with h, one division by (x - z)
//   verify   F_i = sum_b gamma_i^b Z_{T \ S_b}(z_i) (C_ib - r_ib(z_i) G) - Z_T(z_i) W_i and
//            e(sum_i rho_i W'_i, [s]G2) e(-sum_i rho_i (F_i + z_i W'_i), G2) == 1: one MSM over count
//            points, one over count (batch + 2) + 1, one pairing check
// Everything is conversion-free where it touches coefficients, as in kzg.hip.
#include <map>
#include "kzg.hpp"

using namespace pbf;

namespace {

constexpr size_t KM_MAX_PTS = 32;
// per point of a division, in the device table: z, lambda, z^HS_BLK, (z^HS_BLK)^per (per: the
// blocks one thread of k_kzm_div2 takes), then z^(HS_PER 2^j); all in Montgomery form
constexpr int KM_Z = 0, KM_LAM = 1, KM_ZB = 2, KM_ZBP = 3, KM_ZS = 4, KM_TAB = KM_ZS + HS_LOG_T;

// ---------------------------------------------------------------- division by Z_S
// h (+)= sum_j lambda_j quot(c, x - t_j), block-local: the nq = L - 1 quotient coefficients in
// blocks of HS_BLK steps k (h[nq - 1 - k] = s_k, s_k = c[L - 1 - k] + t s_(k-1)), every lane HS_PER
// steps. The lane's coefficients u and its output o are read and written once and stay put while
// the points go by; a point's running values are not kept: the recurrence runs once from 0 for the
// lane's total and, after the Hillis-Steele pass over the lanes, again from the lane's incoming
// value, which costs the product that k_hs1 spends on z^m times the carry. totals[j nb + block] =
// the block's total for point j.
__global__ void __launch_bounds__(HS_T) k_kzm_div1(const uint64_t* c, uint64_t L, const U256* tab, uint32_t np,
                                                   uint64_t nb, uint64_t* h, uint64_t* totals, int accum) {
  __shared__ U256 sh[HS_T];
  const int t = threadIdx.x;
  const uint64_t nq = L - 1, k0 = (uint64_t)blockIdx.x * HS_BLK + (uint64_t)t * HS_PER;
  U256 u[HS_PER], o[HS_PER];
#pragma unroll
  for (int m = 0; m < HS_PER; ++m) {
    const uint64_t k = k0 + m;
    u[m] = k < nq ? u256_from_u64(c + 4 * (L - 1 - k)) : u256_zero();
    o[m] = accum && k < nq ? u256_from_u64(h + 4 * (nq - 1 - k)) : u256_zero();
  }
  for (uint32_t j = 0; j < np; ++j) {
    const U256* pt = tab + (uint64_t)j * KM_TAB;
    const U256 z = pt[KM_Z];
    U256 acc = u256_zero();
#pragma unroll
    for (int m = 0; m < HS_PER; ++m) acc = Fr::add(u[m], Fr::mul_tp(z, acc));
    __syncthreads();  // the previous point's incoming values have been read
    sh[t] = acc;
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < HS_LOG_T; ++i) {
      const int off = 1 << i;
      U256 x = sh[t];
      if (t >= off) x = Fr::add(x, Fr::mul_tp(pt[KM_ZS + i], sh[t - off]));
      __syncthreads();
      sh[t] = x;
      __syncthreads();
    }
    U256 s = t ? sh[t - 1] : u256_zero();
    if (t == HS_T - 1) u256_to_u64(sh[t], totals + 4 * ((uint64_t)j * nb + blockIdx.x));
    const U256 lam = pt[KM_LAM];
#pragma unroll
    for (int m = 0; m < HS_PER; ++m) {
      s = Fr::add(u[m], Fr::mul_tp(z, s));
      o[m] = Fr::add(o[m], Fr::mul_tp(lam, s));
    }
  }
#pragma unroll
  for (int m = 0; m < HS_PER; ++m) {
    const uint64_t k = k0 + m;
    if (k < nq) u256_to_u64(o[m], h + 4 * (nq - 1 - k));
  }
}
// totals[j nb + b] <- lambda_j times the s of point j entering block b (0 for b = 0): k_hs2, one
// block per point
__global__ void __launch_bounds__(HS_T) k_kzm_div2(uint64_t* totals, uint64_t nb, const U256* tab) {
  __shared__ U256 sh[HS_T];
  const int t = threadIdx.x;
  const U256* pt = tab + (uint64_t)blockIdx.x * KM_TAB;
  uint64_t* tot = totals + 4 * (uint64_t)blockIdx.x * nb;
  const U256 zb = pt[KM_ZB], lam = pt[KM_LAM];
  const uint64_t per = (nb + HS_T - 1) / HS_T;
  const uint64_t b0 = (uint64_t)t * per;
  U256 acc = u256_zero();
  for (uint64_t k = 0; k < per; ++k)
    if (b0 + k < nb) acc = Fr::add(u256_from_u64(tot + 4 * (b0 + k)), Fr::mul_tp(zb, acc));
  sh[t] = acc;
  __syncthreads();
  U256 m = pt[KM_ZBP];
  for (int off = 1; off < HS_T; off <<= 1) {
    U256 x = sh[t];
    if (t >= off) x = Fr::add(x, Fr::mul_tp(m, sh[t - off]));
    __syncthreads();
    sh[t] = x;
    __syncthreads();
    m = Fr::mul_tp(m, m);
  }
  U256 cin = t ? sh[t - 1] : u256_zero();
  for (uint64_t k = 0; k < per; ++k) {
    if (b0 + k >= nb) break;
    const U256 x = u256_from_u64(tot + 4 * (b0 + k));
    u256_to_u64(Fr::mul_tp(lam, cin), tot + 4 * (b0 + k));
    cin = Fr::add(x, Fr::mul_tp(zb, cin));
  }
}
// h[nq - 1 - k] += sum_j t_j^(k - k_b + 1) totals[j nb + b]: the fix-up of every point in one read
// and one write of h
__global__ void __launch_bounds__(HS_T) k_kzm_div3(uint64_t* h, uint64_t L, const U256* tab, uint32_t np, uint64_t nb,
                                                   const uint64_t* totals) {
  const uint64_t b = blockIdx.x + 1;  // block 0 enters with s = 0
  const uint64_t nq = L - 1, k0 = b * HS_BLK + (uint64_t)threadIdx.x * HS_PER;
  if (k0 >= nq) return;
  U256 o[HS_PER];
#pragma unroll
  for (int m = 0; m < HS_PER; ++m) o[m] = k0 + m < nq ? u256_from_u64(h + 4 * (nq - 1 - (k0 + m))) : u256_zero();
  for (uint32_t j = 0; j < np; ++j) {
    const U256* pt = tab + (uint64_t)j * KM_TAB;
    const U256 z = pt[KM_Z], cin = u256_from_u64(totals + 4 * ((uint64_t)j * nb + b));
    U256 zk = z;  // z^(t HS_PER + 1) over t's bits
#pragma unroll 1
    for (int i = 0; i < HS_LOG_T; ++i)
      if ((threadIdx.x >> i) & 1) zk = Fr::mul_tp(zk, pt[KM_ZS + i]);
#pragma unroll
    for (int m = 0; m < HS_PER; ++m) {
      o[m] = Fr::add(o[m], Fr::mul_tp(zk, cin));
      zk = Fr::mul_tp(zk, z);
    }
  }
#pragma unroll
  for (int m = 0; m < HS_PER; ++m)
    if (k0 + m < nq) u256_to_u64(o[m], h + 4 * (nq - 1 - (k0 + m)));
}

// ---------------------------------------------------------------- the shape of a call
// T, the sets and gamma of one opening, checked; the polynomials grouped by equal set
struct Group {
  uint64_t mask;
  std::vector<uint64_t> members;  // ascending
};
struct Shape {
  size_t npts;
  std::vector<U256> t;     // Montgomery form
  std::vector<U256> gpow;  // gamma^b, Montgomery form (0^0 = 1)
  std::vector<Group> groups;  // in the order of their first members
};

int mask_check(const uint64_t* sets, size_t batch, size_t npts) {
  const uint64_t all = (1ull << npts) - 1;  // npts <= 32
  for (size_t b = 0; b < batch; ++b)
    if (sets[b] == 0 || (sets[b] & ~all)) return fail(PBF_EINVAL, "a set must be a non-empty subset of the points");
  return 0;
}
// npts canonical, pairwise distinct points
int points_check(const uint64_t* pts, size_t npts) {
  if (!fr_canonical(pts, npts)) return fail(PBF_EINVAL, "pts must be canonical");
  for (size_t j = 1; j < npts; ++j)
    for (size_t m = 0; m < j; ++m)
      if (!memcmp(pts + 4 * j, pts + 4 * m, 32)) return fail(PBF_EINVAL, "pts must be distinct");
  return 0;
}
int shape_args(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* polys, size_t len, size_t pitch,
               size_t batch, const uint64_t* pts, size_t npts, const uint64_t* sets, const uint64_t* gamma,
               Shape* sh) {
  if (!pts || !sets || !gamma) return fail(PBF_EINVAL, "null argument");
  int rc = poly_args(ctx, srs, srs_m, polys, len, pitch, batch, len ? len - 1 : 0);
  if (rc) return rc;
  if (npts == 0 || npts > KM_MAX_PTS) return fail(PBF_EINVAL, "npts must be in 1 .. 32");
  if ((rc = points_check(pts, npts)) || (rc = mask_check(sets, batch, npts))) return rc;
  if (!fr_canonical(gamma)) return fail(PBF_EINVAL, "gamma must be canonical");
  sh->npts = npts;
  sh->t.resize(npts);
  for (size_t j = 0; j < npts; ++j) sh->t[j] = hm(pts + 4 * j);
  const U256 g = hm(gamma);
  sh->gpow.resize(batch);
  std::map<uint64_t, size_t> at;
  for (size_t b = 0; b < batch; ++b) {
    sh->gpow[b] = b ? Fr::mul(sh->gpow[b - 1], g) : fr_one_m();
    auto it = at.find(sets[b]);
    if (it == at.end()) {
      it = at.emplace(sets[b], sh->groups.size()).first;
      sh->groups.push_back({sets[b], {}});
    }
    sh->groups[it->second].members.push_back(b);
  }
  return 0;
}

// prod_{j in mask} (x - t_j), Montgomery form
U256 vanish(const Shape& sh, uint64_t mask, const U256& x) {
  U256 r = fr_one_m();
  for (size_t j = 0; j < sh.npts; ++j)
    if ((mask >> j) & 1) r = Fr::mul(r, Fr::sub(x, sh.t[j]));
  return r;
}

// ---------------------------------------------------------------- h
// The device table of every (group, point of its set), group g's points from entry first[g] on;
// per: the blocks one thread of k_kzm_div2 takes
struct DivTabs {
  std::vector<U256> tab;
  std::vector<size_t> first;
};
void div_tables(const Shape& sh, uint64_t per, DivTabs* dt) {
  for (const Group& g : sh.groups) {
    dt->first.push_back(dt->tab.size() / KM_TAB);
    std::vector<size_t> js;
    for (size_t j = 0; j < sh.npts; ++j)
      if ((g.mask >> j) & 1) js.push_back(j);
    // lambda_j = 1 / prod_{m != j} (t_j - t_m): one Fermat inverse per group
    std::vector<U256> den(js.size()), pre(js.size());
    U256 run = fr_one_m();
    for (size_t a = 0; a < js.size(); ++a) {
      den[a] = vanish(sh, g.mask & ~(1ull << js[a]), sh.t[js[a]]);
      pre[a] = run;
      run = Fr::mul(run, den[a]);
    }
    U256 inv = fr_inv(run);
    for (size_t a = js.size(); a-- > 0;) {
      pre[a] = Fr::mul(inv, pre[a]);  // lambda_a
      inv = Fr::mul(inv, den[a]);
    }
    for (size_t a = 0; a < js.size(); ++a) {
      const size_t at = dt->tab.size();
      dt->tab.resize(at + KM_TAB);
      const U256& z = sh.t[js[a]];
      dt->tab[at + KM_Z] = z;
      dt->tab[at + KM_LAM] = pre[a];
      dt->tab[at + KM_ZB] = fr_pow(z, HS_BLK);
      dt->tab[at + KM_ZBP] = fr_pow(dt->tab[at + KM_ZB], per);
      for (int i = 0; i < HS_LOG_T; ++i) dt->tab[at + KM_ZS + i] = fr_pow(z, (uint64_t)HS_PER << i);
    }
  }
}
// h (+)= quot(c, Z_S) on len - 1 coefficients for the np points at d_tab: k_kzm_div1..3
int div_zs_run(const uint64_t* c, uint64_t len, const U256* d_tab, uint32_t np, uint64_t* h, uint64_t* totals,
               int accum, hipStream_t s) {
  const uint64_t nb = (len - 1 + HS_BLK - 1) / HS_BLK;
  hipLaunchKernelGGL(k_kzm_div1, dim3((uint32_t)nb), dim3(HS_T), 0, s, c, len, d_tab, np, nb, h, totals, accum);
  if (nb > 1) {
    hipLaunchKernelGGL(k_kzm_div2, dim3(np), dim3(HS_T), 0, s, totals, nb, d_tab);
    hipLaunchKernelGGL(k_kzm_div3, dim3((uint32_t)(nb - 1)), dim3(HS_T), 0, s, h, len, d_tab, np, nb,
                       (const uint64_t*)totals);
  }
  PBF_HIP(hipGetLastError());
  return 0;
}
// h = sum over the groups of quot(c_S, Z_S) on len - 1 coefficients (len >= 2): per group the
// weighted sum of its members (kzg_comb_of), then the division adding into h. dt is the caller's:
// the table is uploaded from it, so it lives until the caller has synchronised the stream
int multi_h(pbf_ctx* ctx, const uint64_t* d_polys, uint64_t len, uint64_t pitch, const Shape& sh, DivTabs& dt,
            uint64_t* h, hipStream_t s) {
  const uint64_t nb = (len - 1 + HS_BLK - 1) / HS_BLK;
  div_tables(sh, (nb + HS_T - 1) / HS_T, &dt);
  DevBuf &bt = ctx->buf("kzm.tab"), &btot = ctx->buf("kzm.totals"), &bc = ctx->buf("kzg.comb");
  int rc;
  if ((rc = bt.ensure(dt.tab.size() * sizeof(U256))) || (rc = btot.ensure(sh.npts * nb * 32)) ||
      (rc = bc.ensure(len * 32)))
    return rc;
  PBF_HIP(hipMemcpyAsync(bt.p, dt.tab.data(), dt.tab.size() * sizeof(U256), hipMemcpyHostToDevice, s));
  uint64_t* comb = (uint64_t*)bc.p;
  for (size_t gi = 0; gi < sh.groups.size(); ++gi) {
    const Group& g = sh.groups[gi];
    std::vector<U256> c(g.members.size());
    for (size_t a = 0; a < c.size(); ++a) c[a] = sh.gpow[g.members[a]];
    if ((rc = kzg_comb_of([&](uint64_t a) { return d_polys + 4 * g.members[a] * pitch; }, len, c.size(), c.data(),
                          comb, s)))
      return rc;
    if ((rc = div_zs_run(comb, len, (const U256*)bt.p + dt.first[gi] * KM_TAB, (uint32_t)__builtin_popcountll(g.mask),
                         h, (uint64_t*)btot.p, gi ? 1 : 0, s)))
      return rc;
  }
  return 0;
}

// ---------------------------------------------------------------- evaluations
// y[b][j] = p_b(t_j) for j in S_b into the host array out_y (zero elsewhere), which is written
// after the stream has been synchronised by the caller: fill() does it. fr_eval_run holds two
// distinct points per launch and 12 (polynomial, point) entries, so the points of a polynomial go
// in pairs: it enters ceil(|S_b| / 2) launches. Pairs of equal points fill a launch together.
struct Evals {
  std::vector<std::pair<uint64_t, uint32_t>> where;  // entry -> (b, j)
  std::vector<uint64_t> host;
  void fill(size_t npts, uint64_t* out_y) const {
    for (size_t e = 0; e < where.size(); ++e)
      memcpy(out_y + 4 * (where[e].first * npts + where[e].second), host.data() + 4 * e, 32);
  }
};
int multi_evals(pbf_ctx* ctx, const uint64_t* d_polys, uint64_t len, uint64_t pitch, uint64_t batch,
                const uint64_t* sets, const Shape& sh, Evals* ev, hipStream_t s) {
  struct Task {
    uint32_t j0, j1;  // j1 = npts: a single point
    uint64_t b;
  };
  std::vector<Task> tasks;
  const uint32_t none = (uint32_t)sh.npts;
  for (uint64_t b = 0; b < batch; ++b) {
    uint32_t held = none;
    for (uint32_t j = 0; j < sh.npts; ++j) {
      if (!((sets[b] >> j) & 1)) continue;
      if (held == none) {
        held = j;
      } else {
        tasks.push_back({held, j, b});
        held = none;
      }
    }
    if (held != none) tasks.push_back({held, none, b});
  }
  std::stable_sort(tasks.begin(), tasks.end(), [](const Task& a, const Task& b) {
    return a.j0 != b.j0 ? a.j0 < b.j0 : a.j1 < b.j1;
  });
  size_t entries = 0;
  for (const Task& t : tasks) entries += t.j1 == none ? 1 : 2;
  DevBuf& by = ctx->buf("kzg.y");
  int rc = by.ensure(entries * 32);
  if (rc) return rc;
  ev->host.resize(4 * entries);
  for (size_t i = 0; i < tasks.size();) {
    const uint64_t* polys[12];
    uint64_t lens[12];
    U256 xs[12];
    uint32_t held[2];
    int np = 0, nx = 0;
    for (; i < tasks.size(); ++i) {
      const Task& t = tasks[i];
      const int want = t.j1 == none ? 1 : 2;
      int nx2 = nx;
      uint32_t h2[4] = {nx > 0 ? held[0] : none, nx > 1 ? held[1] : none, none, none};
      for (int q = 0; q < want; ++q) {
        const uint32_t j = q ? t.j1 : t.j0;
        bool have = false;
        for (int r = 0; r < nx2; ++r) have = have || h2[r] == j;
        if (!have) h2[nx2++] = j;
      }
      if (np + want > 12 || nx2 > 2) break;
      for (nx = 0; nx < nx2; ++nx) held[nx] = h2[nx];
      for (int q = 0; q < want; ++q) {
        const uint32_t j = q ? t.j1 : t.j0;
        polys[np] = d_polys + 4 * t.b * pitch;
        lens[np] = len;
        xs[np++] = sh.t[j];
        ev->where.push_back({t.b, j});
      }
    }
    const size_t e0 = ev->where.size() - np;
    if ((rc = fr_eval_run(polys, lens, xs, np, 0, ctx->partial, (uint64_t*)by.p + 4 * e0, s))) return rc;
  }
  PBF_HIP(hipMemcpyAsync(ev->host.data(), by.p, entries * 32, hipMemcpyDeviceToHost, s));
  return 0;
}

// the commitment of the len - 1 coefficients at q against the table, to out (host, after a sync)
int commit_quotient(pbf_ctx* ctx, const Affine* tbl, size_t srs_m, const uint64_t* q, size_t len, Xyzz* hw,
                    hipStream_t s) {
  DevBuf& res = ctx->buf("kzg.w");
  int rc;
  if ((rc = res.ensure(sizeof(Xyzz)))) return rc;
  if ((rc = msm_fixed_device(ctx, tbl, srs_m, 0, q, len - 1, s, (Xyzz*)res.p))) return rc;
  if ((rc = msm_fixed_wait(ctx, s))) return rc;
  PBF_HIP(hipMemcpyAsync(hw, res.p, sizeof(Xyzz), hipMemcpyDeviceToHost, s));
  return 0;
}

// ---------------------------------------------------------------- the verifier's scalars
// den[(i batch + b) npts + j] = prod_{m in S_b, m != j} (t_ij - t_im), canonical, for j in S_b, and 1
// elsewhere (fr_inv_batch_run takes every entry); tm: the points in Montgomery form
__global__ void __launch_bounds__(256) k_kzm_vden(const uint64_t* tm, const uint64_t* sets, uint32_t count,
                                                  uint32_t batch, uint32_t npts, uint64_t* den) {
  const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (e >= (uint64_t)count * batch) return;
  const uint64_t mask = sets[e % batch];
  const uint64_t* t = tm + 4 * (e / batch) * npts;
  for (uint32_t j = 0; j < npts; ++j) {
    U256 d = fr_one_m();
    if ((mask >> j) & 1) {
      const U256 tj = u256_from_u64(t + 4 * j);
      for (uint32_t m = 0; m < npts; ++m)
        if (m != j && ((mask >> m) & 1)) d = Fr::mul(d, Fr::sub(tj, u256_from_u64(t + 4 * m)));
    }
    u256_to_u64(Fr::from_mont(d), den + 4 * (e * npts + j));
  }
}
// One lane per (opening i, polynomial b), e = i batch + b: C_ib into pts[2 count + e] with the
// scalar rho_i gamma_i^b Z_{T \ S_b}(z_i); part[block] = the block's sum of that scalar times
// r_ib(z_i) = sum_{j in S_b} y_ibj prod_{m in S_b, m != j} (z_i - t_im) / (t_ij - t_im), idn the inverses
// of k_kzm_vden's products. gm, zm, tm: Montgomery form; y and rho canonical.
__global__ void __launch_bounds__(256) k_kzm_vpoly(const uint64_t* commits, const uint64_t* tm, const uint64_t* sets,
                                                   const uint64_t* y, const uint64_t* idn, const uint64_t* gm,
                                                   const uint64_t* zm, const uint64_t* rho, uint32_t count,
                                                   uint32_t batch, uint32_t npts, uint64_t* pts, uint64_t* sc,
                                                   uint64_t* part, int* flag) {
  __shared__ U256 sh[256];
  const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  U256 ry = u256_zero();
  if (e < (uint64_t)count * batch) {
    const uint64_t i = e / batch, b = e % batch, mask = sets[b];
    const uint64_t *t = tm + 4 * i * npts, *ye = y + 4 * e * npts, *ie = idn + 4 * e * npts;
    const U256 z = u256_from_u64(zm + 4 * i);
    U256 zb = fr_one_m(), r = u256_zero();
    for (uint32_t j = 0; j < npts; ++j) {
      if (!((mask >> j) & 1)) {
        zb = Fr::mul(zb, Fr::sub(z, u256_from_u64(t + 4 * j)));
        continue;
      }
      U256 term = Fr::mul(u256_from_u64(ye + 4 * j), u256_from_u64(ie + 4 * j));
      for (uint32_t m = 0; m < npts; ++m)
        if (m != j && ((mask >> m) & 1)) term = Fr::mul(term, Fr::sub(z, u256_from_u64(t + 4 * m)));
      r = Fr::add(r, term);
    }
    const U256 g = fr_pow(u256_from_u64(gm + 4 * i), b);
    const U256 scal = Fr::mul(Fr::mul(u256_from_u64(rho + 4 * i), g), zb);
    const uint64_t* c = commits + 8 * e;
    if (g1_bad(c)) atomicOr(flag, 1);
    uint64_t* pc = pts + 8 * (2 * (uint64_t)count + e);
#pragma unroll
    for (int k = 0; k < 8; ++k) pc[k] = c[k];
    u256_to_u64(scal, sc + 4 * (2 * (uint64_t)count + e));
    ry = Fr::mul(Fr::to_mont(scal), r);
  }
  const U256 sum = fr_block_sum(sh, ry);
  if (threadIdx.x == 0) u256_to_u64(sum, part + 4 * (uint64_t)blockIdx.x);
}
// One lane per opening i: pts = [W'_0.. | W_0.. | .], sc = [rho_i z_i | -rho_i Z_T(z_i) | .] and
// rho_i into sc_rho, the scalars of the W' alone
__global__ void __launch_bounds__(256) k_kzm_vopen(const uint64_t* w2, const uint64_t* w, const uint64_t* tm,
                                                   const uint64_t* zm, const uint64_t* rho, uint32_t count,
                                                   uint32_t npts, uint64_t* pts, uint64_t* sc, uint64_t* sc_rho,
                                                   int* flag) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  kzg_vpoints(w2, w, count, i, pts, flag);
  const U256 r = u256_from_u64(rho + 4 * (uint64_t)i), z = u256_from_u64(zm + 4 * (uint64_t)i);
  U256 zt = fr_one_m();
  for (uint32_t j = 0; j < npts; ++j) zt = Fr::mul(zt, Fr::sub(z, u256_from_u64(tm + 4 * ((uint64_t)i * npts + j))));
  u256_to_u64(Fr::mul(r, z), sc + 4 * (uint64_t)i);
  u256_to_u64(Fr::sub(u256_zero(), Fr::mul(r, zt)), sc + 4 * ((uint64_t)count + i));
  u256_to_u64(r, sc_rho + 4 * (uint64_t)i);
}

// what open and finish share past their checks: the stream's buffers and h
struct MultiBufs {
  uint64_t *h, *q;
};
int multi_bufs(pbf_ctx* ctx, size_t len, MultiBufs* mb) {
  DevBuf &bh = ctx->buf("kzm.h"), &bq = ctx->buf("kzg.q"), &br = ctx->buf("kzg.rem");
  const size_t bytes = std::max<size_t>(len - 1, 1) * 32;
  int rc;
  if ((rc = bh.ensure(bytes)) || (rc = bq.ensure(bytes)) || (rc = br.ensure(32))) return rc;
  *mb = {(uint64_t*)bh.p, (uint64_t*)bq.p};
  return 0;
}
void put_point(bool some, const Xyzz& hw, uint64_t* out) {
  if (some) xyzz_to_affine_u64(hw, out);
  else for (int i = 0; i < 8; ++i) out[i] = 0;  // the empty quotient: the identity
}

}  // namespace

// ---------------------------------------------------------------- open
extern "C" int pbf_kzg_open_multi_bn254_dev(pbf_ctx* ctx, const uint64_t* d_srs, size_t srs_m,
                                            const uint64_t* d_polys, size_t len, size_t pitch, size_t batch,
                                            const uint64_t* pts, size_t npts, const uint64_t* sets,
                                            const uint64_t* gamma, uint64_t* out_y, uint64_t* out_w, void* stream) {
  if (!out_y || !out_w) return fail(PBF_EINVAL, "null argument");
  Shape sh;
  int rc = shape_args(ctx, d_srs, srs_m, d_polys, len, pitch, batch, pts, npts, sets, gamma, &sh);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  MultiBufs mb;
  if ((rc = multi_bufs(ctx, len, &mb))) return rc;
  const bool with_msm = len > 1;  // a constant polynomial's quotients are empty: W = the identity
  const Affine* tbl = nullptr;    // validated (one stream sync) before the sweeps are enqueued
  if (with_msm && (rc = msm_fixed_table(ctx, d_srs, srs_m, s, &tbl))) return rc;
  Evals ev;
  if ((rc = multi_evals(ctx, d_polys, len, pitch, batch, sets, sh, &ev, s))) return rc;
  Xyzz hw;
  DivTabs dt;
  if (with_msm) {
    if ((rc = multi_h(ctx, d_polys, len, pitch, sh, dt, mb.h, s))) return rc;
    if ((rc = commit_quotient(ctx, tbl, srs_m, mb.h, len, &hw, s))) return rc;
  }
  PBF_HIP(hipStreamSynchronize(s));
  memset(out_y, 0, batch * npts * 32);
  ev.fill(npts, out_y);
  put_point(with_msm, hw, out_w);
  return PBF_OK;
}

extern "C" int pbf_kzg_open_multi_bn254(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* polys,
                                        size_t len, size_t pitch, size_t batch, const uint64_t* pts, size_t npts,
                                        const uint64_t* sets, const uint64_t* gamma, uint64_t* out_y,
                                        uint64_t* out_w) {
  if (!out_y || !out_w) return fail(PBF_EINVAL, "null argument");
  Shape sh;
  int rc = shape_args(ctx, srs, srs_m, polys, len, pitch, batch, pts, npts, sets, gamma, &sh);
  if (rc) return rc;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  if ((rc = upload_polys(ctx, srs, srs_m, polys, len, pitch, batch, s))) return rc;
  return pbf_kzg_open_multi_bn254_dev(ctx, (const uint64_t*)ctx->buf("kzg.srs").p, srs_m,
                                      (const uint64_t*)ctx->buf("kzg.polys").p, len, len, batch, pts, npts, sets,
                                      gamma, out_y, out_w, s);
}

// ---------------------------------------------------------------- finish
extern "C" int pbf_kzg_open_multi_finish_bn254_dev(pbf_ctx* ctx, const uint64_t* d_srs, size_t srs_m,
                                                   const uint64_t* d_polys, size_t len, size_t pitch, size_t batch,
                                                   const uint64_t* pts, size_t npts, const uint64_t* sets,
                                                   const uint64_t* gamma, const uint64_t* z, uint64_t* out_w2,
                                                   void* stream) {
  if (!z || !out_w2) return fail(PBF_EINVAL, "null argument");
  Shape sh;
  int rc = shape_args(ctx, d_srs, srs_m, d_polys, len, pitch, batch, pts, npts, sets, gamma, &sh);
  if (rc) return rc;
  if (!fr_canonical(z)) return fail(PBF_EINVAL, "z must be canonical");
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  if (len == 1) {  // every quotient is empty
    put_point(false, Xyzz{}, out_w2);
    return PBF_OK;
  }
  MultiBufs mb;
  if ((rc = multi_bufs(ctx, len, &mb))) return rc;
  const Affine* tbl = nullptr;
  if ((rc = msm_fixed_table(ctx, d_srs, srs_m, s, &tbl))) return rc;
  DivTabs dt;
  if ((rc = multi_h(ctx, d_polys, len, pitch, sh, dt, mb.h, s))) return rc;
  // f = sum_b gamma^b Z_{T \ S_b}(z) p_b - Z_T(z) h, in the buffer of the weighted sums
  const U256 zm = hm(z);
  const uint64_t all = (1ull << npts) - 1;
  std::vector<U256> c(batch);
  for (size_t b = 0; b < batch; ++b) c[b] = Fr::mul(sh.gpow[b], vanish(sh, all & ~sets[b], zm));
  uint64_t* f = (uint64_t*)ctx->buf("kzg.comb").p;  // multi_h has sized it
  if ((rc = kzg_comb(d_polys, len, pitch, batch, c.data(), f, s))) return rc;
  const uint64_t* in[2] = {f, mb.h};
  const uint64_t lens[2] = {len, len - 1};
  const U256 ck[2] = {fr_one_m(), Fr::sub(u256_zero(), vanish(sh, all, zm))};
  if ((rc = fr_lincomb_run(2, in, lens, ck, u256_zero(), f, len, s))) return rc;
  HsArgs ha;
  ha.p = f;
  ha.L = len;
  ha.y = u256_zero();
  hs_set_point(ha, zm);
  if ((rc = hs_div_run(ctx, ha, mb.q, (uint64_t*)ctx->buf("kzg.rem").p, s))) return rc;
  Xyzz hw;
  if ((rc = commit_quotient(ctx, tbl, srs_m, mb.q, len, &hw, s))) return rc;
  PBF_HIP(hipStreamSynchronize(s));
  put_point(true, hw, out_w2);
  return PBF_OK;
}

extern "C" int pbf_kzg_open_multi_finish_bn254(pbf_ctx* ctx, const uint64_t* srs, size_t srs_m, const uint64_t* polys,
                                               size_t len, size_t pitch, size_t batch, const uint64_t* pts,
                                               size_t npts, const uint64_t* sets, const uint64_t* gamma,
                                               const uint64_t* z, uint64_t* out_w2) {
  if (!z || !out_w2) return fail(PBF_EINVAL, "null argument");
  Shape sh;
  int rc = shape_args(ctx, srs, srs_m, polys, len, pitch, batch, pts, npts, sets, gamma, &sh);
  if (rc) return rc;
  if (!fr_canonical(z)) return fail(PBF_EINVAL, "z must be canonical");
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  if ((rc = upload_polys(ctx, srs, srs_m, polys, len, pitch, batch, s))) return rc;
  return pbf_kzg_open_multi_finish_bn254_dev(ctx, (const uint64_t*)ctx->buf("kzg.srs").p, srs_m,
                                             (const uint64_t*)ctx->buf("kzg.polys").p, len, len, batch, pts, npts,
                                             sets, gamma, z, out_w2, s);
}

// ---------------------------------------------------------------- verify
extern "C" int pbf_kzg_verify_multi_bn254(pbf_ctx* ctx, const uint64_t* g2, size_t count, size_t batch, size_t npts,
                                          const uint64_t* sets, const uint64_t* commits, const uint64_t* pts,
                                          const uint64_t* y, const uint64_t* gamma, const uint64_t* z,
                                          const uint64_t* w, const uint64_t* w2, const uint64_t* rho, int* ok) {
  if (!ctx || !g2 || !sets || !commits || !pts || !y || !gamma || !z || !w || !w2 || !rho || !ok)
    return fail(PBF_EINVAL, "null argument");
  if (batch == 0 || batch > ((size_t)1 << 16)) return fail(PBF_EINVAL, "batch must be in 1 .. 2^16");
  if (count == 0 || count > ((size_t)1 << 20) / batch) return fail(PBF_EINVAL, "count * batch must be in 1 .. 2^20");
  if (npts == 0 || npts > KM_MAX_PTS) return fail(PBF_EINVAL, "npts must be in 1 .. 32");
  int rc = mask_check(sets, batch, npts);
  if (rc) return rc;
  for (size_t i = 0; i < count; ++i)
    if ((rc = points_check(pts + 4 * npts * i, npts))) return rc;
  if (!fr_canonical(gamma, count) || !fr_canonical(z, count)) return fail(PBF_EINVAL, "gamma and z must be canonical");
  for (size_t e = 0; e < count * batch; ++e)  // y outside the sets is not read
    for (size_t j = 0; j < npts; ++j)
      if (((sets[e % batch] >> j) & 1) && !fr_canonical(y + 4 * (e * npts + j)))
        return fail(PBF_EINVAL, "y must be canonical");
  if ((rc = kzg_rho_check(rho, count))) return rc;
  *ok = 0;
  PBF_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->host_stream();
  const size_t c = count, cb = count * batch, total = c * (batch + 2) + 1;
  const uint32_t nparts = (uint32_t)((cb + 255) / 256);
  // inputs: W', W (8 words each per opening), C (8 per polynomial), the points, gamma, z (Montgomery
  // form, 4 each), rho (4), y (4 npts per polynomial), the sets
  std::vector<uint64_t> mont(4 * c * (npts + 2));
  uint64_t *h_tm = mont.data(), *h_gm = h_tm + 4 * c * npts, *h_zm = h_gm + 4 * c;
  for (size_t i = 0; i < c * npts; ++i) u256_to_u64(hm(pts + 4 * i), h_tm + 4 * i);
  for (size_t i = 0; i < c; ++i) {
    u256_to_u64(hm(gamma + 4 * i), h_gm + 4 * i);
    u256_to_u64(hm(z + 4 * i), h_zm + 4 * i);
  }
  KzgVerify v;
  // scalars: the `total` of the second MSM, then rho for the first
  if ((rc = kzg_verify_bufs(ctx, c, total - c, 16 * c + 8 * cb + mont.size() + 4 * c + 4 * cb * npts + batch, nparts,
                            &v)))
    return rc;
  DevBuf& bden = ctx->buf("kzm.den");
  if ((rc = bden.ensure(cb * npts * 32))) return rc;
  uint64_t *d_c = v.in + 16 * c, *d_tm = d_c + 8 * cb, *d_gm = d_tm + 4 * c * npts, *d_zm = d_gm + 4 * c,
           *d_rho = d_zm + 4 * c, *d_y = d_rho + 4 * c, *d_sets = d_y + 4 * cb * npts, *den = (uint64_t*)bden.p;
  if ((rc = kzg_verify_upload(v, c, w2, w, rho, d_rho, s))) return rc;
  PBF_HIP(hipMemcpyAsync(d_c, commits, cb * 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(d_tm, mont.data(), mont.size() * 8, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(d_y, y, cb * npts * 32, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemcpyAsync(d_sets, sets, batch * 8, hipMemcpyHostToDevice, s));
  static const uint64_t G1_GEN[8] = {1, 0, 0, 0, 2, 0, 0, 0};
  PBF_HIP(hipMemcpyAsync(v.pts + 8 * (total - 1), G1_GEN, 64, hipMemcpyHostToDevice, s));
  PBF_HIP(hipMemsetAsync(v.flag, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_kzm_vden, dim3(nparts), dim3(256), 0, s, (const uint64_t*)d_tm, (const uint64_t*)d_sets,
                     (uint32_t)c, (uint32_t)batch, (uint32_t)npts, den);
  // never zero after the distinctness check; a zero would flag the batch
  if ((rc = fr_inv_batch_run(ctx, den, den, cb * npts, v.flag, s))) return rc;
  hipLaunchKernelGGL(k_kzm_vpoly, dim3(nparts), dim3(256), 0, s, (const uint64_t*)d_c, (const uint64_t*)d_tm,
                     (const uint64_t*)d_sets, (const uint64_t*)d_y, (const uint64_t*)den, (const uint64_t*)d_gm,
                     (const uint64_t*)d_zm, (const uint64_t*)d_rho, (uint32_t)c, (uint32_t)batch, (uint32_t)npts, v.pts,
                     v.sc, v.part, v.flag);
  hipLaunchKernelGGL(k_kzm_vopen, dim3((uint32_t)((c + 255) / 256)), dim3(256), 0, s, (const uint64_t*)v.in,
                     (const uint64_t*)(v.in + 8 * c), (const uint64_t*)d_tm, (const uint64_t*)d_zm,
                     (const uint64_t*)d_rho, (uint32_t)c, (uint32_t)npts, v.pts, v.sc, v.sc + 4 * total, v.flag);
  if ((rc = kzg_vsum_run(v.part, nparts, v.sc + 4 * (total - 1), s))) return rc;
  return kzg_verify_tail_at(ctx, v, v.pts, v.sc + 4 * total, c, total, g2, ok, s);
}
