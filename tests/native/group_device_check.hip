// Test-only device harness for the BN254 G1 group law of csrc/ (tests/test_group_device_gpu.py).
//
// Every kernel here runs ONE point function of ec_bn254.hpp (G1::, G1Quad::) or one composition
// of msm_l29.hpp's accumulator functions that the kernels of csrc/msm.hip use, per thread (per
// quad for G1Quad) on operands the caller chose, and stores what it returned: the arithmetic
// itself lives only in the two headers, which are included unchanged. The Python test compares
// the outputs with the group (oracle/bn254.py) and with integer restatements of the EFD
// formulas, bit for bit. Never linked into libpbf.so.
//
//   int gdc_run(int op, uint64_t p0, uint64_t p1, const void* a, const void* b, void* out, size_t count)
//
// takes host pointers; allocates, copies in, presets the output to 0xA5, launches (256-thread
// blocks), synchronises, copies out, frees; returns the HIP error code (0 = success), -1 for an
// unknown op or a parameter out of range. gdc_layout reports the 64-bit words per element of a,
// b and out. Field elements cross as canonical plain 256-bit values (4 words, little-endian);
// the harness converts with Fq::to_mont / Fq::from_mont. An XYZZ point is X, Y, ZZ, ZZZ (16
// words), an affine point x, y (8 words). A Montgomery result that is not below q is stored as
// all-ones, so the caller's "every coordinate below q" check sees it.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../plonk-by-fingers_amd/csrc/ec_bn254.hpp"
#include "../../plonk-by-fingers_amd/csrc/msm_l29.hpp"

namespace {
using namespace pbf;

enum Op : int {
  // one thread per element
  G_MDBL = 0,   // a: affine                 out: xyzz
  G_DBL,        // a: xyzz                   out: xyzz
  G_DBL2,       // a: xyzz                   out: xyzz
  G_MADD,       // a: xyzz, b: affine        out: xyzz
  G_MADD_TP,    // a: xyzz, b: affine        out: xyzz
  G_ADD,        // a: xyzz, b: xyzz          out: xyzz
  G_ADD2,       // a: xyzz, b: xyzz          out: xyzz
  G_MUL_SMALL,  // a: xyzz, p0 = k < 2^32    out: xyzz
  G_TO_AFFINE,  // a: xyzz                   out: affine (to_affine_plain, which runs G1::inv)
  // one quad per element: 4 * count threads, the four lanes of a quad load the same operands and
  // each stores its own copy of the result
  Q_ADD = 20,   // a: xyzz, b: xyzz          out: 4 x xyzz
  Q_DBL,        // a: xyzz                   out: 4 x xyzz
  // the MSM's 29-bit-limb accumulator; a: xyzz, not the identity. out: the round trip of
  // acc = from_xyzz(a), then the same accumulator's with acc.id = true
  ACC_XYZZ = 30,  // to_xyzz(acc)
  ACC_RAW,        // raw_to_xyzz(store_raw(acc))
  // a: p0 = K affine points (1 <= K <= 43 = MSM_CH), none the identity. The loop body of
  // msm_chunk_acc_l29r from acc.id = true. out: to_xyzz(acc), raw_to_xyzz(store_raw(acc)), the
  // K-bit mask of the steps at which l29::madd returned true, the K-bit mask of acc.id after
  // each step
  ACC_CHAIN,
  G_CHAIN  // the same points through acc = G1::madd(acc, p) from G1::identity(); out: xyzz
};
constexpr uint32_t CHAIN_MAX = 43;

struct Ctx {
  const uint64_t* a;
  const uint64_t* b;
  uint64_t* out;
  size_t n;
  uint32_t k;
};

__device__ __forceinline__ U256 ld_m(const uint64_t* p) { return Fq::to_mont(u256_from_u64(p)); }
__device__ __forceinline__ void st_p(uint64_t* p, const U256& v) {
  if (Fq::geq_p(v)) {
    for (int i = 0; i < 4; ++i) p[i] = ~0ull;
    return;
  }
  u256_to_u64(Fq::from_mont(v), p);
}
__device__ __forceinline__ Xyzz ld_xyzz(const uint64_t* p) {
  Xyzz r;
  r.X = ld_m(p), r.Y = ld_m(p + 4), r.ZZ = ld_m(p + 8), r.ZZZ = ld_m(p + 12);
  return r;
}
__device__ __forceinline__ Affine ld_aff(const uint64_t* p) {
  Affine r;
  r.x = ld_m(p), r.y = ld_m(p + 4);
  return r;
}
__device__ __forceinline__ void st_xyzz(uint64_t* p, const Xyzz& v) {
  st_p(p, v.X), st_p(p + 4, v.Y), st_p(p + 8, v.ZZ), st_p(p + 12, v.ZZZ);
}
__device__ __forceinline__ Xyzz raw_round_trip(const l29::Acc& acc) {
  __attribute__((aligned(16))) uint32_t raw[36];
  l29::store_raw(acc, raw);
  return l29::raw_to_xyzz(raw);
}

template <int OP>
__global__ void __launch_bounds__(256) gdc_kernel(Ctx c) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= c.n) return;
  if constexpr (OP == G_MDBL) st_xyzz(c.out + 16 * i, G1::mdbl(ld_aff(c.a + 8 * i)));
  if constexpr (OP == G_DBL) st_xyzz(c.out + 16 * i, G1::dbl(ld_xyzz(c.a + 16 * i)));
  if constexpr (OP == G_DBL2) st_xyzz(c.out + 16 * i, G1::dbl2(ld_xyzz(c.a + 16 * i)));
  if constexpr (OP == G_MADD) st_xyzz(c.out + 16 * i, G1::madd(ld_xyzz(c.a + 16 * i), ld_aff(c.b + 8 * i)));
  if constexpr (OP == G_MADD_TP) st_xyzz(c.out + 16 * i, G1::madd_tp(ld_xyzz(c.a + 16 * i), ld_aff(c.b + 8 * i)));
  if constexpr (OP == G_ADD) st_xyzz(c.out + 16 * i, G1::add(ld_xyzz(c.a + 16 * i), ld_xyzz(c.b + 16 * i)));
  if constexpr (OP == G_ADD2) st_xyzz(c.out + 16 * i, G1::add2(ld_xyzz(c.a + 16 * i), ld_xyzz(c.b + 16 * i)));
  if constexpr (OP == G_MUL_SMALL) st_xyzz(c.out + 16 * i, G1::mul_small(ld_xyzz(c.a + 16 * i), c.k));
  if constexpr (OP == G_TO_AFFINE) {
    U256 x, y;
    G1::to_affine_plain(ld_xyzz(c.a + 16 * i), &x, &y);
    u256_to_u64(x, c.out + 8 * i);
    u256_to_u64(y, c.out + 8 * i + 4);
  }
  if constexpr (OP == ACC_XYZZ || OP == ACC_RAW) {
    l29::Acc acc = l29::from_xyzz(ld_xyzz(c.a + 16 * i));
    st_xyzz(c.out + 32 * i, OP == ACC_XYZZ ? l29::to_xyzz(acc) : raw_round_trip(acc));
    acc.id = true;
    st_xyzz(c.out + 32 * i + 16, OP == ACC_XYZZ ? l29::to_xyzz(acc) : raw_round_trip(acc));
  }
  if constexpr (OP == ACC_CHAIN) {
    const uint64_t* pts = c.a + 8 * (size_t)c.k * i;
    l29::Acc acc{};
    acc.id = true;
    uint64_t dbl_mask = 0, id_mask = 0;
    for (uint32_t j = 0; j < c.k; ++j) {
      const Affine p = ld_aff(pts + 8 * j);
      if (l29::madd(acc, l29::from_u256(p.x), l29::from_u256(p.y))) {
        const Affine q = ld_aff(pts + 8 * j);  // P + P: the doubled point, from the point reloaded
        acc = l29::from_xyzz(G1::mdbl(q));
        dbl_mask |= 1ull << j;
      }
      if (acc.id) id_mask |= 1ull << j;
    }
    uint64_t* o = c.out + 34 * i;
    st_xyzz(o, l29::to_xyzz(acc));
    st_xyzz(o + 16, raw_round_trip(acc));
    o[32] = dbl_mask;
    o[33] = id_mask;
  }
  if constexpr (OP == G_CHAIN) {
    const uint64_t* pts = c.a + 8 * (size_t)c.k * i;
    Xyzz acc = G1::identity();
    for (uint32_t j = 0; j < c.k; ++j) acc = G1::madd(acc, ld_aff(pts + 8 * j));
    st_xyzz(c.out + 16 * i, acc);
  }
}

// c.n elements, 4 c.n threads: a block holds 64 whole quads, so a quad is active or absent as one
template <int OP>
__global__ void __launch_bounds__(256) gdc_quad_kernel(Ctx c) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, i = t >> 2;
  if (i >= c.n) return;
  const Xyzz p = ld_xyzz(c.a + 16 * i);
  Xyzz r;
  if constexpr (OP == Q_ADD) r = G1Quad::add(p, ld_xyzz(c.b + 16 * i));
  else r = G1Quad::dbl(p);
  st_xyzz(c.out + 16 * t, r);
}

// ---- host side --------------------------------------------------------------------------------
struct Layout {
  int aw, bw, ow, quad;
};
bool layout_of(int op, uint64_t p0, Layout* l) {
  switch (op) {
    case G_MDBL: *l = {8, 0, 16, 0}; return true;
    case G_DBL:
    case G_DBL2: *l = {16, 0, 16, 0}; return true;
    case G_MADD:
    case G_MADD_TP: *l = {16, 8, 16, 0}; return true;
    case G_ADD:
    case G_ADD2: *l = {16, 16, 16, 0}; return true;
    case G_MUL_SMALL: *l = {16, 0, 16, 0}; return p0 <= 0xffffffffull;
    case G_TO_AFFINE: *l = {16, 0, 8, 0}; return true;
    case Q_ADD: *l = {16, 16, 64, 1}; return true;
    case Q_DBL: *l = {16, 0, 64, 1}; return true;
    case ACC_XYZZ:
    case ACC_RAW: *l = {16, 0, 32, 0}; return true;
    case ACC_CHAIN: *l = {(int)(8 * p0), 0, 34, 0}; return p0 >= 1 && p0 <= CHAIN_MAX;
    case G_CHAIN: *l = {(int)(8 * p0), 0, 16, 0}; return p0 >= 1 && p0 <= CHAIN_MAX;
    default: return false;
  }
}

template <int OP>
void launch(const Ctx& c) {
  hipLaunchKernelGGL(gdc_kernel<OP>, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, 0, c);
}
template <int OP>
void launch_quad(const Ctx& c) {
  hipLaunchKernelGGL(gdc_quad_kernel<OP>, dim3((unsigned)((4 * c.n + 255) / 256)), dim3(256), 0, 0, c);
}
void dispatch(int op, const Ctx& c) {
  switch (op) {
    case G_MDBL: return launch<G_MDBL>(c);
    case G_DBL: return launch<G_DBL>(c);
    case G_DBL2: return launch<G_DBL2>(c);
    case G_MADD: return launch<G_MADD>(c);
    case G_MADD_TP: return launch<G_MADD_TP>(c);
    case G_ADD: return launch<G_ADD>(c);
    case G_ADD2: return launch<G_ADD2>(c);
    case G_MUL_SMALL: return launch<G_MUL_SMALL>(c);
    case G_TO_AFFINE: return launch<G_TO_AFFINE>(c);
    case Q_ADD: return launch_quad<Q_ADD>(c);
    case Q_DBL: return launch_quad<Q_DBL>(c);
    case ACC_XYZZ: return launch<ACC_XYZZ>(c);
    case ACC_RAW: return launch<ACC_RAW>(c);
    case ACC_CHAIN: return launch<ACC_CHAIN>(c);
    case G_CHAIN: return launch<G_CHAIN>(c);
  }
}

int run(int op, uint64_t p0, const void* a, const void* b, void* out, size_t count) {
  Layout l;
  if (!layout_of(op, p0, &l)) return -1;
  if (count == 0) return 0;
  if (!a || !out || (l.bw && !b)) return -1;
  const size_t na = count * l.aw * 8, nb = count * l.bw * 8, no = count * l.ow * 8;
  void *da = nullptr, *db = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc(&da, na);
  if (e == hipSuccess && nb) e = hipMalloc(&db, nb);
  if (e == hipSuccess) e = hipMalloc(&dout, no);
  if (e == hipSuccess) e = hipMemcpy(da, a, na, hipMemcpyHostToDevice);
  if (e == hipSuccess && nb) e = hipMemcpy(db, b, nb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0xA5, no);
  if (e == hipSuccess) {
    dispatch(op, Ctx{(const uint64_t*)da, (const uint64_t*)db, (uint64_t*)dout, count, (uint32_t)p0});
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, no, hipMemcpyDeviceToHost);
  if (da) (void)hipFree(da);
  if (db) (void)hipFree(db);
  if (dout) (void)hipFree(dout);
  return (int)e;
}
}  // namespace

extern "C" {
// p0: k of G_MUL_SMALL, K of the chains; p1 is unused (the signature of fdc_run)
int gdc_run(int op, uint64_t p0, uint64_t p1, const void* a, const void* b, void* out, size_t count) {
  (void)p1;
  return run(op, p0, a, b, out, count);
}
// 64-bit words per element of a, b, out, and 1 for a quad op (out holds the four lanes' copies)
int gdc_layout(int op, uint64_t p0, uint64_t p1, int* layout4) {
  (void)p1;
  Layout l;
  if (!layout4 || !layout_of(op, p0, &l)) return -1;
  layout4[0] = l.aw, layout4[1] = l.bw, layout4[2] = l.ow, layout4[3] = l.quad;
  return 0;
}
}
