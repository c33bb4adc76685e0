// Kernel instantiation, NTT planning and launchers for libpbf.so (gfx950).
#include <cstdlib>
#include <cstring>
#include <mutex>
#include "internal.hpp"
#include "ntt_gl.hpp"

namespace pbf {

// ---------------------------------------------------------------- plans
bool hinv(uint64_t a, uint64_t m, uint64_t* out) {
  // extended gcd in i128 (u64field.rs:10-25 uses i64; the inverse is unique)
  __int128 s = 0, old_s = 1, r = m, old_r = a % m;
  while (r != 0) {
    __int128 q = old_r / r, t;
    t = old_r - q * r; old_r = r; r = t;
    t = old_s - q * s; old_s = s; s = t;
  }
  if (old_r != 1) return false;
  if (old_s < 0) old_s += m;
  *out = (uint64_t)old_s;
  return true;
}

bool field_for(uint64_t m, FieldKind* kind, FieldArgs* fa) {
  fa->m = m;
  fa->mu = 0;
  if (m == GOLDILOCKS) { *kind = FIELD_GOLDILOCKS; return true; }
  if (m >= 3 && m < (1ull << 32) && (m & 1)) {
    *kind = FIELD_MOD32;
    fa->mu = (uint64_t)(((u128)1 << 64) / m);
    return true;
  }
  return false;
}

int DevBuf::ensure(size_t need) {
  if (need <= bytes) return 0;
  if (p) (void)hipFree(p);
  p = nullptr;
  bytes = 0;
  hipError_t e = hipMalloc(&p, need);
  if (e != hipSuccess) { p = nullptr; return fail(3, std::string("hipMalloc: ") + hipGetErrorString(e)); }
  bytes = need;
  return 0;
}
void DevBuf::release() {
  if (p) (void)hipFree(p);
  p = nullptr;
  bytes = 0;
}
DevBuf::~DevBuf() { release(); }

static int upload(DevBuf& b, const std::vector<uint64_t>& v) {
  int rc = b.ensure(v.size() * 8);
  if (rc) return rc;
  PBF_HIP(hipMemcpy(b.p, v.data(), v.size() * 8, hipMemcpyHostToDevice));
  return 0;
}

// ---------------------------------------------------------------- host twiddle tables
// Every table of this file is built here, on the host, as plain words; the caller uploads it.
typedef std::vector<uint64_t> Table;

// c s^i, i < count
static Table geometric(uint64_t c, uint64_t s, uint64_t count, uint64_t m) {
  Table t(count);
  uint64_t x = c % m;
  for (uint64_t i = 0; i < count; ++i) { t[i] = x; x = hmul(x, s, m); }
  return t;
}

// Two-level table of c root^i, i < len: first[i] = c root^i (i < 2^bits), second[i] = root^(i << bits),
// so that c root^i = first[i mod 2^bits] * second[i >> bits]
static std::pair<Table, Table> two_level_tabs(uint64_t root, uint64_t len, uint32_t bits, uint64_t c, uint64_t m) {
  return {geometric(c, root, 1ull << bits, m),
          geometric(1, hpow(root, 1ull << bits, m), ((len - 1) >> bits) + 1, m)};
}

// Stage-C table of ntt_gl_pass_kernel: tc[r2][k1] = scale * w_R^(r2 k1), r2 < C = R/64, k1 < 64
static Table stage_c_tab(uint64_t w_r, uint64_t C, uint64_t scale, uint64_t m) {
  Table tc(C * 64);
  for (uint64_t r2 = 0; r2 < C; ++r2)
    for (uint64_t k1 = 0; k1 < 64; ++k1) tc[r2 * 64 + k1] = hmul(hpow(w_r, r2 * k1, m), scale, m);
  return tc;
}

// Per-pass table T[r][k] = w_p^(r k), r < R, k < ns (w_p = w^(n/(ns R)), the pass's twiddle root)
static Table pass_tab(uint64_t w_p, uint64_t R, uint64_t ns, uint64_t m) {
  Table t;
  t.reserve(R * ns);
  for (uint64_t r = 0; r < R; ++r) {
    const Table row = geometric(1, hpow(w_p, r, m), ns, m);
    t.insert(t.end(), row.begin(), row.end());
  }
  return t;
}

// The [r][k] table of the second pass of a 2^10 x 2^10 plan (pass_tab(w, 1024, 1024): entry
// w^(j k) for the first pass's output y(j, k)) in the order of the tile-major intermediate
// (ntt_gl.hpp SP 2): entry (j, k) at (k >> 3) * pitch + j * 8 + (k & 7), so that the first pass's
// store index is its table index. The pad of a block (pitch > 8192) is never read.
static Table pass_tab_blocked(uint64_t w, uint64_t pitch, uint64_t m) {
  Table t(128 * pitch, 0);
  for (uint64_t k = 0; k < 1024; ++k) {
    const Table col = geometric(1, hpow(w, k, m), 1024, m);
    for (uint64_t j = 0; j < 1024; ++j) t[(k >> 3) * pitch + j * 8 + (k & 7)] = col[j];
  }
  return t;
}

// The same twiddles split for a last pass: w_p^(r k) = B[kb][r] * A[r][c] for k = kb W + c, with
// A[r][c] = w_p^(r c) (R x W) and B[kb][r] = w_p^(r kb W) (ns/W x R)
static std::pair<Table, Table> split_tabs(uint64_t w_p, uint64_t R, uint64_t W, uint64_t ns, uint64_t m) {
  Table ta = pass_tab(w_p, R, W, m), tb((ns / W) * R);
  for (uint64_t r = 0; r < R; ++r) {
    const Table col = geometric(1, hpow(w_p, r * W, m), ns / W, m);
    for (uint64_t kb = 0; kb < ns / W; ++kb) tb[kb * R + r] = col[kb];
  }
  return {ta, tb};
}

// radix bits per pass: option "ntt.passes" (e.g. "12,12"; every radix family the planner can
// pick, tests/test_ntt_gpu.py), else passes of at most 2^10 as equal as possible
static std::vector<int> default_passes(uint32_t log_n, const Options& o) {
  const char* env = o.get("ntt.passes");
  if (env && *env) {
    std::vector<int> v;
    int sum = 0;
    for (const char* c = env; *c;) {
      int x = atoi(c);
      v.push_back(x);
      sum += x;
      while (*c && *c != ',') ++c;
      if (*c == ',') ++c;
    }
    bool ok = sum == (int)log_n;
    for (int x : v) ok = ok && x >= 6 && x <= 12;
    if (ok) return v;
  }
  int p = (log_n + 9) / 10;
  std::vector<int> v(p, log_n / p);
  for (int i = 0; i < (int)(log_n % p); ++i) v[i] += 1;
  return v;
}

// Tile of R x W elements per workgroup of ntt_gl_pass_kernel: radix 2^10 8192 (W = 8: 64-B runs
// in HBM, two workgroups per CU), smaller radices 4096 (W >= 16; four or five workgroups per CU).
// Wider tiles (W = 16 at 2^10: one workgroup per CU) measured slower in round 4.
static constexpr int gl_tile(int logr) { return logr >= 10 ? 8192 : 4096; }

int make_plan(uint64_t m, uint64_t omega, uint64_t n, int inverse, NttPlan* p) {
  if (!field_for(m, &p->kind, &p->fa)) return fail(5, "unsupported modulus");
  if (n == 0 || (n & (n - 1))) return fail(1, "n must be a power of two");
  if (n > (1ull << 32)) return fail(1, "n too large");
  if (omega >= m) return fail(1, "omega not canonical");
  uint32_t log_n = 0;
  while ((1ull << log_n) < n) ++log_n;
  if (n > 1) {
    // omega must have order exactly n (the reference assumes it; fft.rs:55-65)
    if (hpow(omega, n, m) != 1 || hpow(omega, n / 2, m) == 1) return fail(1, "omega does not have order n");
  }
  p->m = m; p->omega = omega; p->n = n; p->inverse = inverse; p->log_n = log_n;
  p->root = omega;
  if (inverse) {
    if (!hinv(n % m, m, &p->n_inv)) return fail(2, "n has no inverse modulo M (fft.rs:73 unwrap)");
    if (!hinv(omega, m, &p->root)) return fail(1, "omega not invertible");
  }
  const uint64_t w = p->root;
  const long long tm = p->opts.num("ntt.twmax_log", 24);
  p->twmax_log = (int)(tm < 0 ? 0 : (tm > 30 ? 30 : tm));
  if (n <= 4096) return upload(p->small_tw, geometric(1, w, n, m));
  p->logr = default_passes(log_n, p->opts);
  p->tw_bits = (log_n + 1) / 2;
  // standard Goldilocks root => shift twiddles in the register sub-DFTs
  p->e64 = -1;
  if (p->kind == FIELD_GOLDILOCKS) {
    const uint64_t w64 = hpow(w, n / 64, m);
    if (w64 == hpow(2, 39, m)) p->e64 = 39;
    else if (w64 == hpow(2, 153, m)) p->e64 = 153;
  }
  // ntt_gl_pass_kernel runs the plans of standard Goldilocks roots and radices 2^6..2^10,
  // ntt_pass_kernel every other
  p->gl = p->e64 >= 0;
  for (int lr : p->logr) p->gl = p->gl && lr >= 6 && lr <= 10;
  // regrouped 2^24 plan (default for 8,8,8 standard-root plans; option ntt.no_rg=1 keeps the
  // round-2 passes, the tests' cross-check): three twiddle layers of order 4096, 2^18 and 2^24
  // 
  p->rg = p->gl && log_n == 24 && p->logr == std::vector<int>{8, 8, 8} && p->opts.num("ntt.no_rg", 0) == 0;

  int rc;
  const auto tw = two_level_tabs(w, n, p->tw_bits, 1, m);
  if ((rc = upload(p->tw0, tw.first)) || (rc = upload(p->tw1, tw.second))) return rc;
  const size_t P = p->logr.size();
  uint64_t ns = 1;
  for (size_t i = 0; i < P; ++i) {
    const uint64_t R = 1ull << p->logr[i], w_p = hpow(w, n / (ns * R), m);
    // per-pass [r][k] twiddle tables while R*Ns <= 2^ntt.twmax_log (default 24: the last
    // pass of a 2^24 transform reads a 128 MiB table, shared by every polynomial of a batch,
    // in 128-B runs like its data; the two-level table's two random gathers per element were
    // bound by the texture unit: 2^24 x 2 0.545 -> 0.490 ms); larger passes
    // use the two-level table
    p->twpass.push_back(std::make_shared<DevBuf>());
    if (ns > 1 && R * ns <= (1ull << p->twmax_log) && (rc = upload(*p->twpass[i], pass_tab(w_p, R, ns, m)))) return rc;
    // the last pass of a standard-root plan whose [r][k] table is not built: split table
    // (option ntt.twsplit=1 also replaces a built one, =0 keeps the two-level table: the
    // paths of n > 2^24 exercised at test sizes)
    const long long ts = p->opts.num("ntt.twsplit", -1);
    const uint64_t W = (uint64_t)gl_tile(p->logr[i]) >> p->logr[i];
    if (i + 1 == P && ns > 1 && p->e64 >= 0 && ts != 0 && p->logr[i] >= 6 && p->logr[i] <= 10 &&
        (!p->twpass[i]->p || ts == 1) && ns % W == 0) {
      if (ts == 1) p->twpass[i] = std::make_shared<DevBuf>();
      const auto ab = split_tabs(w_p, R, W, ns, m);
      p->tws_a = std::make_shared<DevBuf>();
      p->tws_b = std::make_shared<DevBuf>();
      if ((rc = upload(*p->tws_a, ab.first)) || (rc = upload(*p->tws_b, ab.second))) return rc;
      p->tws_w = (int)W;
    }
    ns *= R;
  }
  // forward "10,10" plans keep their intermediate tile-major (gl_blocked): the second pass's
  // table once more, in that order, for the first pass's stores. twpass[1] stays: the split-store
  // and coset runs of this plan read it.
  if (p->gl && !inverse && p->e64 == 39 && p->logr == std::vector<int>{10, 10} && p->twpass[1]->p &&
      (rc = upload(p->post_blk, pass_tab_blocked(w, GL_BLK_PITCH, m))))
    return rc;
  for (size_t i = 0; i < P; ++i) {
    const uint64_t R = 1ull << p->logr[i], w_r = hpow(w, n / R, m);
    auto b = std::make_shared<DevBuf>();
    if (p->gl) {
      // stage-C table of ntt_gl_pass_kernel; the last pass of an inverse carries n^-1
      rc = upload(*b, stage_c_tab(w_r, R / 64, (inverse && i + 1 == P) ? p->n_inv : 1, m));
      p->tc.push_back(b);
    } else {
      // w_R^m, m < R: the in-workgroup stage twiddles of ntt_pass_kernel
      rc = upload(*b, geometric(1, w_r, R, m));
      p->rtab.push_back(b);
    }
    if (rc) return rc;
  }
  return 0;
}

// ---------------------------------------------------------------- dispatch
// Calls fn(F{}) with F the device field type of `k`, so that a kernel's launch is written once
// for both fields: with_field(k, [&](auto F) { ... kernel<decltype(F)> ... })
template <class Fn>
static auto with_field(FieldKind k, Fn&& fn) {
  return k == FIELD_GOLDILOCKS ? fn(Goldilocks{}) : fn(Mod32{});
}

typedef void (*PassFn)(PassArgs);

// W columns per workgroup of ntt_pass_kernel, one tile per workgroup (the LDS-DMA double-buffered
// and register-prefetching persistent forms of rounds 1-2 measured slower and were removed in
// round 6: DESIGN.md §3.2)
static constexpr int cols_for(int logr) {
  // radix 2^10: 8 columns (64-KiB tile, two workgroups per CU overlap each other's HBM
  // and arithmetic phases; measured 0.548 vs 0.585 ms for 16 columns at 2^20 x 32)
  return logr < 10 ? 16 : (logr == 10 ? 8 : (logr == 11 ? 8 : 4));
}

template <class F, int E>
static PassFn pass_fn_e(int logr) {
#define PBF_PASS(LR) \
  case LR: return ntt_pass_kernel<F, LR, cols_for(LR), ((cols_for(LR) << LR) >> NTT_LQ), E>;
  switch (logr) {
    PBF_PASS(6) PBF_PASS(7) PBF_PASS(8) PBF_PASS(9) PBF_PASS(10) PBF_PASS(11) PBF_PASS(12)
    default: return nullptr;
  }
#undef PBF_PASS
}

static PassFn pass_fn(FieldKind k, int e64, int logr) {
  if (k == FIELD_MOD32) return pass_fn_e<Mod32, -1>(logr);
  if (e64 == 39) return pass_fn_e<Goldilocks, 39>(logr);
  if (e64 == 153) return pass_fn_e<Goldilocks, 153>(logr);
  return pass_fn_e<Goldilocks, -1>(logr);
}

// A coset transform on the ntt_gl_pass_kernel passes (run_plan_coset): the factor table and,
// forward, the compact input's length
struct GlCoset {
  const CosetTabs* tabs;
  uint64_t in_len;
};

static int run_plan_impl(const NttPlan& p, const uint64_t* d_in, uint64_t* d_out, size_t batch, DevBuf& s0,
                         DevBuf& s1, hipStream_t stream, uint32_t split_log, ForkSet* fork = nullptr,
                         const GlCoset* cs = nullptr);

int run_plan(const NttPlan& p, const uint64_t* d_in, uint64_t* d_out, size_t batch, DevBuf& s0, DevBuf& s1,
             hipStream_t stream, ForkSet* fork) {
  return run_plan_impl(p, d_in, d_out, batch, s0, s1, stream, 0, fork);
}

// Split a natural-order batch [b][g*S + kk] into the send layout [g][b][kk].
__global__ void shard_split_kernel(const uint64_t* in, uint64_t* out, uint64_t s, uint64_t nl, uint32_t batch) {
  const uint64_t total = nl * batch;
  for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total;
       id += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t b = id / nl, k = id % nl;
    out[((k / s) * batch + b) * s + (k % s)] = in[id];
  }
}

static uint64_t grid_for(uint64_t count) {
  uint64_t b = (count + 255) / 256;
  return b > 8192 ? 8192 : (b ? b : 1);
}

int run_plan_split(const NttPlan& p, const uint64_t* d_in, uint64_t* d_send, size_t batch, uint32_t G, DevBuf& s0,
                   DevBuf& s1, DevBuf& s2, hipStream_t stream) {
  const uint64_t S = p.n / G;
  uint32_t sl = 0;
  while ((1ull << sl) < S) ++sl;
  // the last Stockham pass can store the send layout directly when S >= its W columns
  if (!p.logr.empty() && S >= 16 && p.logr.size() >= 2) return run_plan_impl(p, d_in, d_send, batch, s0, s1, stream, sl);
  int rc = s2.ensure(batch * p.n * 8);
  if (rc) return rc;
  if ((rc = run_plan_impl(p, d_in, (uint64_t*)s2.p, batch, s0, s1, stream, 0))) return rc;
  hipLaunchKernelGGL(shard_split_kernel, dim3(grid_for(p.n * batch)), dim3(256), 0, stream, (const uint64_t*)s2.p,
                     d_send, S, p.n, (uint32_t)batch);
  PBF_HIP(hipGetLastError());
  return 0;
}

int launch_shard_unsplit(const uint64_t* recv, uint64_t* out, uint64_t nl, uint32_t batch, uint32_t G,
                         hipStream_t s) {
  hipLaunchKernelGGL(shard_unsplit_kernel, dim3(grid_for(nl * batch)), dim3(256), 0, s, recv, out, nl / G, nl, batch,
                     G);
  PBF_HIP(hipGetLastError());
  return 0;
}

int make_two_level(uint64_t m, uint64_t root, uint64_t n, TwoLevel* t) {
  uint32_t log_n = 0;
  while ((1ull << log_n) < n) ++log_n;
  t->bits = (log_n + 1) / 2;
  t->root = root;
  const auto tw = two_level_tabs(root, n, t->bits, 1, m);
  int rc = upload(t->t0, tw.first);
  return rc ? rc : upload(t->t1, tw.second);
}

template <class F>
static int combine_typed(const FieldArgs& fa, const TwoLevel& tl, uint32_t G, uint64_t rank, const uint64_t* in,
                         uint64_t* out, uint64_t nl, uint32_t batch, int inverse, hipStream_t s) {
  CombineArgs a;
  a.recv = in; a.out = out;
  a.tw0 = (const uint64_t*)tl.t0.p; a.tw1 = (const uint64_t*)tl.t1.p; a.tw_bits = tl.bits;
  a.nl = nl; a.s = nl / G; a.rank = rank; a.n_mask = (uint64_t)G * nl - 1; a.batch = batch; a.f = fa;
  a.scale = 1;
  if (inverse) {
    uint64_t ginv;
    if (!hinv(G % fa.m, fa.m, &ginv)) return fail(2, "G has no inverse");
    a.scale = ginv;
  }
  for (int i = 0; i < 8; ++i) a.wg[i] = 0;
  const uint64_t wG = hpow(tl.root, nl, fa.m);  // primitive G-th root (direction-specific)
  uint64_t x = 1 % fa.m;
  for (uint32_t i = 0; i < G; ++i) { a.wg[i] = x; x = hmul(x, wG, fa.m); }
  const uint64_t total = (nl / G) * batch;
  void (*fn)(CombineArgs) = nullptr;
  switch (G) {
    case 2: fn = inverse ? shard_split_inv_kernel<F, 2> : shard_combine_kernel<F, 2>; break;
    case 4: fn = inverse ? shard_split_inv_kernel<F, 4> : shard_combine_kernel<F, 4>; break;
    case 8: fn = inverse ? shard_split_inv_kernel<F, 8> : shard_combine_kernel<F, 8>; break;
    default: return fail(1, "world size must be 2, 4 or 8");
  }
  hipLaunchKernelGGL(fn, dim3(grid_for(total)), dim3(256), 0, s, a);
  PBF_HIP(hipGetLastError());
  return 0;
}

int launch_shard_combine(FieldKind k, const FieldArgs& fa, const TwoLevel& tl, uint32_t G, uint64_t rank,
                         const uint64_t* in, uint64_t* out, uint64_t nl, uint32_t batch, int inverse, hipStream_t s) {
  return with_field(k, [&](auto F) {
    return combine_typed<decltype(F)>(fa, tl, G, rank, in, out, nl, batch, inverse, s);
  });
}

typedef void (*GlPassFn)(GlPassArgs);

// Which ntt_gl_* kernel one pass of a plan runs (the template parameters of ntt_gl.hpp); the
// tile is gl_tile(logr).
struct GlPassDesc {
  int logr;
  bool first;
  int rg;  // regrouped 2^24 plan: pass 1, 2 (ntt_gl_rg2_kernel) or 3; 0 = not regrouped
  int cs;  // coset variant: 1 = scales its loads, 2 = scales its stores
  int sp;  // plain forward two-pass plan: 1 = its specialised second pass; 2 = either pass of "10,10"
};

// Two-pass plans apply the second pass's twiddle w^(j k) at the first pass's stores (post_tw,
// gl_pass_args), when that pass has its [r][k] table and stores no split layout
static bool two_pass_tw(const NttPlan& p, uint32_t split_log) {
  return p.logr.size() == 2 && split_log == 0 && p.twpass[1]->p;
}

// Plain forward "10,10" runs keep the intermediate between their passes tile-major (ntt_gl.hpp
// SP 2): both passes are the SP 2 pair, the scratch takes gl_scratch_pitch per polynomial
static bool gl_blocked(const NttPlan& p, bool coset, uint32_t split_log) {
  return two_pass_tw(p, split_log) && !coset && p.post_blk.p != nullptr;
}

// Elements of intermediate scratch per polynomial
static uint64_t gl_scratch_pitch(const NttPlan& p, bool coset, uint32_t split_log) {
  return gl_blocked(p, coset, split_log) ? 128 * GL_BLK_PITCH : p.n;
}

static GlPassDesc gl_pass_desc(const NttPlan& p, size_t i, bool coset, uint32_t split_log) {
  const size_t P = p.logr.size();
  GlPassDesc d{p.logr[i], i == 0, 0, 0, 0};
  // the regrouped plan stores no split layout
  if (p.rg && P == 3 && split_log == 0) d.rg = (int)i + 1;
  // coset: a forward transform's first pass scales its loads, an inverse's last pass its stores
  if (coset && !p.inverse && i == 0) d.cs = 1;
  if (coset && p.inverse && i == P - 1) d.cs = 2;
  // plain forward two-pass plans whose second pass is radix 2^10 and skips its twiddle: that
  // pass compiled with only what such a plan executes (ntt_gl.hpp SP); instantiated for the
  // forward standard root only. Both passes of the 2^20 default "10,10": the tile-major pair.
  if (gl_blocked(p, coset, split_log)) d.sp = 2;
  else if (two_pass_tw(p, split_log) && i == 1 && !coset && !p.inverse && p.e64 == 39 && d.logr == 10) d.sp = 1;
  return d;
}

// The kernel of a descriptor: exactly the instantiations gl_pass_desc can ask for.
template <int E, int LR>
static GlPassFn gl_kernel_lr(const GlPassDesc& d) {
  constexpr int T = gl_tile(LR);
  if (d.first) return d.cs ? ntt_gl_pass_kernel<LR, E, true, T, 0, 1> : ntt_gl_pass_kernel<LR, E, true, T>;
  return d.cs ? ntt_gl_pass_kernel<LR, E, false, T, 0, 2> : ntt_gl_pass_kernel<LR, E, false, T>;
}

template <int E>
static GlPassFn gl_kernel_e(const GlPassDesc& d) {
  if (d.rg == 1) return d.cs ? ntt_gl_pass_kernel<8, E, true, 4096, 1, 1> : ntt_gl_pass_kernel<8, E, true, 4096, 1>;
  if (d.rg == 2) return ntt_gl_rg2_kernel<E>;
  if (d.rg == 3) return d.cs ? ntt_gl_pass_kernel<8, E, false, 4096, 3, 2> : ntt_gl_pass_kernel<8, E, false, 4096, 3>;
  if constexpr (E == 39) {
    if (d.sp == 1) return ntt_gl_pass_kernel<10, E, false, 8192, 0, 0, 1>;
    if (d.sp == 2) return d.first ? ntt_gl_pass_kernel<10, E, true, 8192, 0, 0, 2> : ntt_gl_pass_kernel<10, E, false, 8192, 0, 0, 2>;
  }
  switch (d.logr) {
    case 6: return gl_kernel_lr<E, 6>(d);
    case 7: return gl_kernel_lr<E, 7>(d);
    case 8: return gl_kernel_lr<E, 8>(d);
    case 9: return gl_kernel_lr<E, 9>(d);
    case 10: return gl_kernel_lr<E, 10>(d);
    default: return nullptr;
  }
}

static GlPassFn gl_kernel(const GlPassDesc& d, int e64) {
  return e64 == 39 ? gl_kernel_e<39>(d) : gl_kernel_e<153>(d);
}

// Passes of a standard-root Goldilocks plan through ntt_gl_pass_kernel (ntt_gl.hpp).
static int run_gl_group(const NttPlan& p, const uint64_t* d_in, uint64_t* d_out, size_t batch, DevBuf& s0,
                        DevBuf& s1, hipStream_t stream, uint32_t split_log, size_t soff = 0,
                        const GlCoset* cs = nullptr);

int ForkSet::ensure(int streams) {
  if (streams > GL_MAX_STREAMS) streams = GL_MAX_STREAMS;
  // The events order kernels of one device against each other, so they carry no system-scope
  // fence: what the host sees is settled by the caller's own synchronisation or copy on their
  // stream (the argument and the measurement)
  const unsigned flags = hipEventDisableTiming | hipEventDisableSystemFence;
  if (streams > 1 && !fork) PBF_HIP(hipEventCreateWithFlags(&fork, flags));
  for (int i = 1; i < streams; ++i) {
    if (!aux[i]) PBF_HIP(hipStreamCreateWithFlags(&aux[i], hipStreamNonBlocking));
    if (!join[i]) PBF_HIP(hipEventCreateWithFlags(&join[i], flags));
  }
  return 0;
}

ForkSet::~ForkSet() {
  (void)hipSetDevice(device);
  for (int i = 1; i < GL_MAX_STREAMS; ++i) {
    if (aux[i]) {
      (void)hipStreamSynchronize(aux[i]);
      (void)hipStreamDestroy(aux[i]);
    }
    if (join[i]) (void)hipEventDestroy(join[i]);
  }
  if (fork) (void)hipEventDestroy(fork);
}

// The group schedule of a batched Goldilocks plan: G polynomials per group (0: the whole batch
// is one group) over ns streams.
// default schedule (measured best at 2^20 x 32): groups of 4 polynomials
// alternating over the caller's stream and a second one once the batch has at least 8, so the
// passes of two groups run concurrently and their load / compute / store phases interleave
// (options ntt.group = polynomials per group, ntt.streams = streams; 0 or >= batch: one group).
// The tile-major "10,10" pair (gl_blocked) takes groups of 8 once the batch has 16: its kernels
// fit three workgroups per CU (ntt_gl.hpp split exchange), and a launch of 4 polynomials is 512
// workgroups, two per CU: the third slot fills only with 1024 per launch
static void gl_schedule(const NttPlan& p, size_t batch, bool coset, uint32_t split_log, const ForkSet* fork, size_t* G,
                        int* ns) {
  const long long go = p.opts.num("ntt.group", -1);
  const size_t dflt = gl_blocked(p, coset, split_log) && batch >= 16 ? 8 : 4;
  *G = go >= 0 ? (size_t)go : (batch >= 8 ? dflt : batch);
  if (split_log != 0 || *G >= batch) *G = 0;
  *ns = (int)p.opts.num("ntt.streams", 2);
  *ns = *ns < 1 ? 1 : (*ns > GL_MAX_STREAMS ? GL_MAX_STREAMS : *ns);
  if (!fork || *G == 0) *ns = 1;
}

// Polynomials of intermediate scratch that schedule needs. The groups of one stream run one
// after another, so they share one slot of G polynomials (run_gl_passes): the intermediates of
// a 2^20 x 32 batch take 64 MiB, not 256 MiB, and stay within the 256 MiB Infinity Cache.
static size_t gl_scratch_polys(const NttPlan& p, size_t batch, bool coset, uint32_t split_log, const ForkSet* fork) {
  size_t G;
  int ns;
  gl_schedule(p, batch, coset, split_log, fork, &G, &ns);
  return (G == 0 || G * ns > batch) ? batch : G * ns;
}

static int run_gl_passes(const NttPlan& p, const uint64_t* d_in, uint64_t* d_out, size_t batch, DevBuf& s0,
                         DevBuf& s1, hipStream_t stream, uint32_t split_log, ForkSet* fork, const GlCoset* cs) {
  size_t G;
  int ns;
  gl_schedule(p, batch, cs != nullptr, split_log, fork, &G, &ns);
  if (G == 0) return run_gl_group(p, d_in, d_out, batch, s0, s1, stream, split_log, 0, cs);
  // a forward coset transform reads compact polynomials of in_len coefficients
  const size_t in_pitch = (cs && !p.inverse) ? cs->in_len : p.n;
  hipStream_t sts[GL_MAX_STREAMS];
  sts[0] = stream;
  // Fork and join by events: a stream waiting on an event waits in the command processor
  // (a barrier packet), so it cannot hold the GPU against the work it waits for. Round 5's
  // stream memory-operation joins (hipStreamWaitValue64: a spinning wait kernel) measured 1-4 %
  // faster but never resumed when the queues were serialised (rocprofv3 counter collection,
  // profiles/r05/memop_prof.log); removed in round 6.
  if (ns > 1) {
    int rc = fork->ensure(ns);
    if (rc) return rc;
    for (int i = 1; i < ns; ++i) sts[i] = fork->aux[i];
    PBF_HIP(hipEventRecord(fork->fork, stream));
    for (int i = 1; i < ns; ++i) PBF_HIP(hipStreamWaitEvent(sts[i], fork->fork, 0));
  }
  int gi = 0;
  for (size_t g0 = 0; g0 < batch; g0 += G, ++gi) {
    const size_t b = batch - g0 < G ? batch - g0 : G;
    // scratch ring: one slot of G polynomials per stream (a stream's groups are serialised)
    const int rc = run_gl_group(p, d_in + g0 * in_pitch, d_out + g0 * p.n, b, s0, s1, sts[gi % ns], 0,
                                (size_t)(gi % ns) * G * gl_scratch_pitch(p, cs != nullptr, split_log), cs);
    if (rc) return rc;
  }
  for (int i = 1; i < ns; ++i) {
    PBF_HIP(hipEventRecord(fork->join[i], sts[i]));
    PBF_HIP(hipStreamWaitEvent(stream, fork->join[i], 0));
  }
  return 0;
}

// The regrouped plan's twiddle tables, built on the first run that takes the regrouped path:
// tc1[a2l][r2][k1] (4096), t2[a1][K] (2^18), and the last pass's C[r2][X] = w^(r2 X) (n^-1
// folded in for the inverse), D[X] = w^(4 X) (X < 2^18: 10 MiB)
static int ensure_rg_tables(const NttPlan& p) {
  if (p.rg_built) return 0;
  const uint64_t m = p.m, n = p.n;
  const uint64_t w = p.root;
  int rc;
  const uint64_t w4096 = hpow(w, n / 4096, m);
  std::vector<uint64_t> tc1(4096);
  for (uint64_t a2l = 0; a2l < 16; ++a2l)
    for (uint64_t r2 = 0; r2 < 4; ++r2)
      for (uint64_t k1 = 0; k1 < 64; ++k1)
        tc1[a2l * 256 + r2 * 64 + k1] = hpow(w4096, ((a2l + 16 * r2) * k1) % 4096, m);
  const Table t2 = pass_tab(hpow(w, 64, m), 64, 4096, m);  // t2[a1][K] = w^(64 a1 K)
  // the last pass's twiddle w^(a0 X) (a0 = r2 + 4 s2, X = 65536 f + j) as C[r2][X] D[X]^s2 (round
  // 5: from 10 MiB instead of a 2^24-entry, 128 MiB table T3[f][a0][j], profiles/r05/t3geo_ab.log)
  const uint64_t scale = p.inverse ? p.n_inv : 1;
  std::vector<uint64_t> tgc(4ull << 18), tgb(1ull << 18);
  {
    const uint64_t w4 = hpow(w, 4, m);
    uint64_t x1 = 1, x4 = 1;
    for (uint64_t X = 0; X < (1ull << 18); ++X) {
      tgb[X] = x4;
      uint64_t c = scale;
      for (uint64_t r2 = 0; r2 < 4; ++r2) {
        tgc[(r2 << 18) + X] = c;
        c = hmul(c, x1, m);
      }
      x1 = hmul(x1, w, m);
      x4 = hmul(x4, w4, m);
    }
  }
  if ((rc = upload(p.rg_tc1, tc1)) || (rc = upload(p.rg_t2, t2)) || (rc = upload(p.rg_tgc, tgc)) ||
      (rc = upload(p.rg_tgb, tgb)))
    return rc;
  p.rg_built = true;
  return 0;
}

// The arguments of pass i (descriptor d, log_ns = log2 of the product of the earlier radices) over
// `batch` polynomials from `in` to `out`.
static GlPassArgs gl_pass_args(const NttPlan& p, size_t i, const GlPassDesc& d, uint32_t log_ns, const uint64_t* in,
                               uint64_t* out, size_t batch, uint32_t split_log, const GlCoset* cs) {
  const bool last = i == p.logr.size() - 1;
  const uint64_t W = (uint64_t)gl_tile(d.logr) >> d.logr;
  GlPassArgs a;
  a.in = in;
  a.out = out;
  a.in_pitch = a.out_pitch = p.n;
  a.twpass = (const uint64_t*)p.twpass[i]->p;
  a.tw0 = (const uint64_t*)p.tw0.p;
  a.tw1 = (const uint64_t*)p.tw1.p;
  a.tc = (const uint64_t*)p.tc[i]->p;
  const bool tws = !a.twpass && last && p.tws_a && (uint64_t)p.tws_w == W;
  a.tws_a = tws ? (const uint64_t*)p.tws_a->p : nullptr;
  a.tws_b = tws ? (const uint64_t*)p.tws_b->p : nullptr;
  a.n = p.n;
  a.log_n = p.log_n;
  a.log_ns = log_ns;
  a.tw_bits = p.tw_bits;
  a.blocks_per_poly = (uint32_t)((p.n >> d.logr) / W);
  a.batch = (uint32_t)batch;
  a.scaled = (p.inverse && last) ? 1 : 0;
  a.out_split_log = last ? split_log : 0;
  const uint64_t tiles = (uint64_t)a.blocks_per_poly * batch;
  // tile order (gl_tile_coords): later passes XCD k-major (the pass-twiddle table's slices
  // fetched into each XCD's L2 once per pass, not once per polynomial)
  a.xcd_kmajor = (log_ns > 0 && batch > 1 && tiles % 8 == 0) ? 1 : 0;
  // two-pass plans apply the second pass's twiddle w^(j k) at the first pass's stores (the
  // first pass hides the product under its memory phase: 2^20 x 32 0.400 -> 0.386 ms,
  // DESIGN.md §3.1), reading that table by column in XCD k-major order too (round 4: 2^20 x 32
  // 0.354-0.357 ms against 0.368-0.371 linear, profiles/r04/ntt_orders_sweep.log)
  a.post_tw = nullptr;
  a.skip_pass_tw = 0;
  if (two_pass_tw(p, split_log)) {
    if (i == 0) a.post_tw = (const uint64_t*)p.twpass[1]->p;
    else a.skip_pass_tw = 1;
  }
  if (a.post_tw && batch > 1 && tiles % 8 == 0) a.xcd_kmajor = 1;
  a.blk_pitch = 0;
  if (d.sp == 2) {
    a.blk_pitch = GL_BLK_PITCH;
    if (i == 0) {
      a.post_tw = (const uint64_t*)p.post_blk.p;
      a.out_pitch = 128 * GL_BLK_PITCH;
    } else {
      // the second pass reads no table, so k-major buys nothing, and its tiles lie one after
      // another: linear order, neighbouring workgroups on neighbouring blocks (round 9: 0.2994
      // against 0.3022 ms k-major at steady clocks, XCD-blocked 0.3033)
      a.in_pitch = 128 * GL_BLK_PITCH;
      a.xcd_kmajor = 0;
    }
  }
  a.cs_tab = a.cs_tab1 = nullptr;
  a.cs_bits = 0;
  a.cs_len = 0;
  if (d.cs) {
    a.cs_tab = (const uint64_t*)cs->tabs->t0.p;
    a.cs_tab1 = (const uint64_t*)cs->tabs->t1.p;
    a.cs_bits = cs->tabs->bits;
    if (d.cs == 1) {
      a.cs_len = cs->in_len;
      a.in_pitch = cs->in_len;
    } else if (!d.rg) {
      a.tc = (const uint64_t*)cs->tabs->tc_last.p;  // n^-1 rides in the factor table
      a.scaled = 0;
    }  // (the regrouped plan's last pass keeps n^-1 in its own table: ensure_rg_tables)
  }
  if (d.rg) {
    if (d.rg == 1) a.tc = (const uint64_t*)p.rg_tc1.p;
    if (d.rg == 2) a.twpass = (const uint64_t*)p.rg_t2.p;
    if (d.rg == 3) {
      a.twpass = nullptr;
      a.tws_a = (const uint64_t*)p.rg_tgc.p;
      a.tws_b = (const uint64_t*)p.rg_tgb.p;
    }
    // XCD-blocked order in every pass of the regrouped plan (round 4: 2 x 2^24 0.433-0.437 ms
    // against 0.447-0.453 k-major, 0.462-0.466 linear, profiles/r04/ntt_order24_ab.log; round
    // 5 with the geometric last pass 0.3867-0.3868 against 0.3918-0.3930, order_geo.log)
    if (tiles % 8 == 0) a.xcd_kmajor = 2;
  }
  return a;
}

static int run_gl_group(const NttPlan& p, const uint64_t* d_in, uint64_t* d_out, size_t batch, DevBuf& s0,
                        DevBuf& s1, hipStream_t stream, uint32_t split_log, size_t soff, const GlCoset* cs) {
  const size_t P = p.logr.size();
  if (cs && (split_log != 0 || P < 2)) return fail(1, "coset transform: unsupported plan");
  if (gl_pass_desc(p, 0, cs != nullptr, split_log).rg) {
    const int rc = ensure_rg_tables(p);
    if (rc) return rc;
  }
  uint32_t log_ns = 0;
  for (size_t i = 0; i < P; ++i) {
    const GlPassDesc d = gl_pass_desc(p, i, cs != nullptr, split_log);
    const GlPassFn fn = gl_kernel(d, p.e64);
    if (!fn) return fail(1, "no Goldilocks pass kernel for this radix");
    const int tile = gl_tile(d.logr);
    if ((p.n >> d.logr) % (tile >> d.logr)) return fail(1, "transform too small for the pass tile");
    const uint64_t* in = (i == 0) ? d_in : (const uint64_t*)(((i - 1) & 1) ? s1.p : s0.p) + soff;
    uint64_t* out = (i == P - 1) ? d_out : (uint64_t*)((i & 1) ? s1.p : s0.p) + soff;
    const GlPassArgs a = gl_pass_args(p, i, d, log_ns, in, out, batch, split_log, cs);
    const uint64_t tiles = (uint64_t)a.blocks_per_poly * batch;
    if (tiles > 0x7fffffffull) return fail(1, "batch too large");
    hipLaunchKernelGGL(fn, dim3((uint32_t)tiles), dim3(tile / 16), 0, stream, a);
    PBF_HIP(hipGetLastError());
    log_ns += d.logr;
  }
  return 0;
}

static int run_plan_impl(const NttPlan& p, const uint64_t* d_in, uint64_t* d_out, size_t batch, DevBuf& s0,
                         DevBuf& s1, hipStream_t stream, uint32_t split_log, ForkSet* fork, const GlCoset* cs) {
  if (batch == 0) return 0;
  if (p.n == 1) {
    if (d_in != d_out) PBF_HIP(hipMemcpyAsync(d_out, d_in, batch * 8, hipMemcpyDeviceToDevice, stream));
    return 0;  // size-1 DFT is the identity; n^-1 = 1
  }
  if (p.logr.empty()) {
    with_field(p.kind, [&](auto F) {
      hipLaunchKernelGGL(ntt_small_kernel<decltype(F)>, dim3(batch), dim3(256), 0, stream, d_in, d_out,
                         (const uint64_t*)p.small_tw.p, p.log_n, p.n_inv, (uint32_t)p.inverse, p.fa);
    });
    PBF_HIP(hipGetLastError());
    return 0;
  }
  const size_t P = p.logr.size();
  const size_t bytes = p.gl ? gl_scratch_polys(p, batch, cs != nullptr, split_log, fork) * gl_scratch_pitch(p, cs != nullptr, split_log) * 8
                            : batch * p.n * 8;
  int rc = s0.ensure(bytes);
  if (!rc && P > 2) rc = s1.ensure(bytes);
  if (rc) return rc;
  uint32_t log_ns = 0;
  if (p.gl) return run_gl_passes(p, d_in, d_out, batch, s0, s1, stream, split_log, fork, cs);
  if (cs) return fail(1, "coset transform: not a Goldilocks standard-root plan");
  for (size_t i = 0; i < P; ++i) {
    const int lr = p.logr[i];
    const PassFn fn = pass_fn(p.kind, p.e64, lr);
    if (!fn) return fail(1, "no kernel for this radix");
    const int W = cols_for(lr);
    PassArgs a;
    a.in = (i == 0) ? d_in : (const uint64_t*)(((i - 1) & 1) ? s1.p : s0.p);
    a.out = (i == P - 1) ? d_out : (uint64_t*)((i & 1) ? s1.p : s0.p);
    a.tw0 = (const uint64_t*)p.tw0.p;
    a.tw1 = (const uint64_t*)p.tw1.p;
    a.rtab = (const uint64_t*)p.rtab[i]->p;
    a.twpass = (const uint64_t*)p.twpass[i]->p;
    a.n = p.n;
    a.n_inv = p.n_inv;
    a.log_n = p.log_n;
    a.log_ns = log_ns;
    a.tw_bits = p.tw_bits;
    a.blocks_per_poly = (uint32_t)((p.n >> lr) / W);
    a.scale = (p.inverse && i == P - 1) ? 1 : 0;
    a.out_split_log = (i == P - 1) ? split_log : 0;
    a.batch = (uint32_t)batch;
    a.f = p.fa;
    const int nt = (W << lr) >> NTT_LQ;
    const uint64_t blocks = (uint64_t)a.blocks_per_poly * batch;
    if (blocks > 0x7fffffffull) return fail(1, "batch too large");
    const uint32_t grid = (uint32_t)blocks;
    a.xcd_kmajor = (log_ns > 0 && batch > 1 && grid % 8 == 0) ? 1 : 0;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(nt), 0, stream, a);
    PBF_HIP(hipGetLastError());
    log_ns += lr;
  }
  return 0;
}

// ---------------------------------------------------------------- coset transforms
static uint32_t log2_ceil(uint64_t x) {
  uint32_t l = 0;
  while ((1ull << l) < x) ++l;
  return l;
}

// The factor table of (plan, shift) with at least `len` entries (internal.hpp CosetTabs), from
// the plan's cache or built on the host like make_plan's tables. An evicted table is freed by
// hipFree, which waits for the kernels still reading it; a forward table that a longer input
// outgrows is rebuilt after a device synchronisation.
static int coset_tabs(const NttPlan& p, uint64_t shift, uint64_t len, const CosetTabs** out) {
  const uint64_t m = p.m;
  CosetTabs* t = nullptr;
  for (auto& c : p.coset)
    if (c->shift == shift) t = c.get();
  if (t && t->len >= len) {
    t->stamp = ++p.coset_clock;
    *out = t;
    return 0;
  }
  if (!t) {
    if (p.coset.size() >= COSET_SHIFTS_PER_PLAN) {
      size_t old = 0;
      for (size_t i = 1; i < p.coset.size(); ++i)
        if (p.coset[i]->stamp < p.coset[old]->stamp) old = i;
      p.coset.erase(p.coset.begin() + old);
    }
    p.coset.emplace_back(new CosetTabs());
    t = p.coset.back().get();
    t->shift = shift;
  } else {
    PBF_HIP(hipDeviceSynchronize());  // rebuilt longer, in place: no kernel may still read it
  }
  t->len = 0;  // not valid until every upload below has succeeded
  uint64_t s = shift, c = 1 % m;
  if (p.inverse) {
    if (!hinv(shift, m, &s)) return fail(1, "shift has no inverse");
    if (p.gl && !p.rg) c = p.n_inv;
  }
  int rc;
  if (len <= (1ull << p.twmax_log)) {
    t->bits = 0;
    t->t1.release();
    if ((rc = upload(t->t0, geometric(c, s, len, m)))) return rc;
  } else {
    t->bits = (log2_ceil(len) + 1) / 2;
    const auto tw = two_level_tabs(s, len, t->bits, c, m);
    if ((rc = upload(t->t0, tw.first)) || (rc = upload(t->t1, tw.second))) return rc;
  }
  if (p.gl && !p.rg && p.inverse && !t->tc_last.p) {
    const uint64_t R = 1ull << p.logr.back();
    if ((rc = upload(t->tc_last, stage_c_tab(hpow(p.root, p.n / R, m), R / 64, 1, m)))) return rc;
  }
  t->len = len;
  t->stamp = ++p.coset_clock;
  *out = t;
  return 0;
}

// out[b*n + i] = i < in_len ? in[b*in_len + i] * factor(i) : 0 (the scaling pass of the plans
// that do not fuse it; in may equal out when in_len = n)
template <class F>
__global__ void coset_scale_kernel(const uint64_t* in, uint64_t in_len, uint64_t* out, uint64_t n, uint64_t batch,
                                   const uint64_t* t0, const uint64_t* t1, uint32_t bits, FieldArgs f) {
  const uint64_t total = n * batch;
  for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total;
       id += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t b = id / n, i = id % n;
    uint64_t y = 0;
    if (i < in_len) {
      const uint64_t tw = t1 ? F::mul(t0[i & ((1ull << bits) - 1)], t1[i >> bits], f) : t0[i];
      y = F::mul(in[b * in_len + i], tw, f);
    }
    out[id] = y;
  }
}

static int launch_coset_scale(const NttPlan& p, const CosetTabs& t, const uint64_t* in, uint64_t in_len, uint64_t* out,
                              uint64_t batch, hipStream_t s) {
  const dim3 grid((uint32_t)grid_for(p.n * batch));
  with_field(p.kind, [&](auto F) {
    hipLaunchKernelGGL(coset_scale_kernel<decltype(F)>, grid, dim3(256), 0, s, in, in_len, out, p.n, batch,
                       (const uint64_t*)t.t0.p, (const uint64_t*)t.t1.p, t.bits, p.fa);
  });
  PBF_HIP(hipGetLastError());
  return 0;
}

int run_plan_coset(const NttPlan& p, uint64_t shift, const uint64_t* d_in, size_t in_len, uint64_t* d_out,
                   size_t batch, DevBuf& s0, DevBuf& s1, hipStream_t stream, ForkSet* fork) {
  if (batch == 0) return 0;
  // n = 1 has the one factor shift^0; shift 1 on whole polynomials is the plain transform
  if (p.n == 1 || (shift == 1 && in_len == p.n)) return run_plan_impl(p, d_in, d_out, batch, s0, s1, stream, 0, fork);
  const CosetTabs* t;
  int rc = coset_tabs(p, shift, p.inverse ? p.n : in_len, &t);
  if (rc) return rc;
  if (p.gl) {
    const GlCoset cs{t, in_len};
    return run_plan_impl(p, d_in, d_out, batch, s0, s1, stream, 0, fork, &cs);
  }
  if (p.inverse) {
    if ((rc = run_plan_impl(p, d_in, d_out, batch, s0, s1, stream, 0, fork))) return rc;
    return launch_coset_scale(p, *t, d_out, p.n, d_out, batch, stream);
  }
  if ((rc = launch_coset_scale(p, *t, d_in, in_len, d_out, batch, stream))) return rc;
  return run_plan_impl(p, d_out, d_out, batch, s0, s1, stream, 0, fork);
}

// ---------------------------------------------------------------- pointwise
int launch_pointwise_mul(FieldKind k, const FieldArgs& fa, const uint64_t* a, const uint64_t* b, uint64_t* c,
                         uint64_t count, hipStream_t s) {
  uint64_t blocks = (count + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks == 0) return 0;
  with_field(k, [&](auto F) {
    hipLaunchKernelGGL(pointwise_mul_kernel<decltype(F)>, dim3(blocks), dim3(256), 0, s, a, b, c, count, fa);
  });
  PBF_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- poly eval
// Poly::eval (poly.rs:71-79): y = sum_j c_j x^j. Block (point, chunk) computes
// x^start * Horner(chunk) and tree-reduces; a second kernel sums the chunks.
template <class F>
__device__ uint64_t dpow(uint64_t x, uint64_t e, const FieldArgs& f) {
  uint64_t r = 1 % f.m;
  while (e) {
    if (e & 1) r = F::mul(r, x, f);
    x = F::mul(x, x, f);
    e >>= 1;
  }
  return r;
}

constexpr int EVAL_PER_THREAD = 64;
constexpr int EVAL_THREADS = 256;

template <class F>
__global__ void __launch_bounds__(EVAL_THREADS) poly_eval_partial(const uint64_t* c, uint64_t n, const uint64_t* xs,
                                                                  uint64_t chunks, uint64_t* partial, FieldArgs f) {
  __shared__ uint64_t red[EVAL_THREADS];
  const uint64_t pt = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  const uint64_t x = xs[pt];
  const uint64_t start = (ch * EVAL_THREADS + threadIdx.x) * EVAL_PER_THREAD;
  uint64_t acc = 0;
  if (start < n) {
    uint64_t end = start + EVAL_PER_THREAD;
    if (end > n) end = n;
    for (uint64_t j = end; j-- > start;) acc = F::add(F::mul(acc, x, f), c[j], f);
    acc = F::mul(acc, dpow<F>(x, start, f), f);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = EVAL_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = F::add(red[threadIdx.x], red[threadIdx.x + s], f);
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

template <class F>
__global__ void poly_eval_final(const uint64_t* partial, uint64_t chunks, uint64_t nx, uint64_t* ys, FieldArgs f) {
  uint64_t pt = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pt >= nx) return;
  uint64_t acc = 0;
  for (uint64_t i = 0; i < chunks; ++i) acc = F::add(acc, partial[pt * chunks + i], f);
  ys[pt] = acc;
}

int launch_poly_eval(FieldKind k, const FieldArgs& fa, const uint64_t* d_coeffs, uint64_t n, const uint64_t* d_xs,
                     uint64_t nx, uint64_t* d_ys, DevBuf& partial, hipStream_t s) {
  const uint64_t per_block = (uint64_t)EVAL_THREADS * EVAL_PER_THREAD;
  const uint64_t chunks = (n + per_block - 1) / per_block;
  int rc = partial.ensure(chunks * nx * 8);
  if (rc) return rc;
  with_field(k, [&](auto F) {
    hipLaunchKernelGGL(poly_eval_partial<decltype(F)>, dim3(chunks * nx), dim3(EVAL_THREADS), 0, s, d_coeffs, n,
                       d_xs, chunks, (uint64_t*)partial.p, fa);
    hipLaunchKernelGGL(poly_eval_final<decltype(F)>, dim3((nx + 255) / 256), dim3(256), 0, s,
                       (const uint64_t*)partial.p, chunks, nx, d_ys, fa);
  });
  PBF_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- synthetic inputs
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Element i: z = mix(seed + (i+1)*golden); Goldilocks rejects z >= p by re-mixing
// z + golden; Mod32 reduces z % M. Mirrors tests/golden/gen_golden.py:splitmix_field.
__global__ void fill_random_kernel(uint64_t seed, uint64_t* out, uint64_t count, FieldArgs f, int gold) {
  const uint64_t G = 0x9E3779B97F4A7C15ull;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t z = splitmix64(seed + (i + 1) * G);
    if (gold) {
      while (z >= f.m) z = splitmix64(z + G);
    } else {
      z %= f.m;
    }
    out[i] = z;
  }
}

int launch_fill_random(const FieldArgs& fa, FieldKind k, uint64_t seed, uint64_t* d_out, uint64_t count,
                       hipStream_t s) {
  if (count == 0) return 0;
  uint64_t blocks = (count + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(fill_random_kernel, dim3(blocks), dim3(256), 0, s, seed, d_out, count, fa,
                     k == FIELD_GOLDILOCKS ? 1 : 0);
  PBF_HIP(hipGetLastError());
  return 0;
}

}  // namespace pbf
