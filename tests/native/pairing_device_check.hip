// Test-only device harness for the Fq2 / Fq6 / Fq12 tower of csrc/pairing.hip
// (tests/test_pairing_device_gpu.py).
//
// csrc/pairing.hip is included unchanged, as one unit: every kernel here calls ONE of its device
// functions (or one step of its final-exponentiation interpreter) on operands the caller chose and
// stores what it returned, so the arithmetic lives only in that file. The unit's own make_consts()
// and ensure_inv2k() fill this unit's copy of the constants and of g_inv2k. The three host symbols
// the unit leaves undefined (pbf::fail, pbf::DevBuf::ensure, pbf::DevBuf::~DevBuf) come from
// libpbf.so, which the harness is linked against; -Bsymbolic binds everything else (g_inv2k's
// host shadow among it) to this unit's own definitions. Never linked into libpbf.so.
//
//   int pdc_run(int op, uint64_t p0, uint64_t p1, const void* a, const void* b, void* out, size_t count)
//
// takes host pointers; allocates, copies in, presets the output to 0xA5, launches, synchronises,
// copies out, frees; returns the HIP error code (0 = success), -1 for an unknown op or a parameter
// out of range. pdc_layout reports the 64-bit words per element of a, b and out. Field elements
// cross as canonical plain 256-bit values (4 words, little-endian) and are converted with
// Fq::to_mont / Fq::from_mont, except where an op is marked "raw": there the four words are the
// very value the function sees and returns. A 9-limb lazy sum (L9) is 5 words, the top 32 bits
// ignored. A stored result that is not below q is written as all-ones.
//
// Lane ops: one thread per element (64-thread blocks, as pairing_lane_kernel); Fq6 is c0, c1, c2
// and Fq12 the ABI's tower order c0.a0 c0.a1 c0.a2 c1.a0 c1.a1 c1.a2. Workgroup ops: one
// 256-thread workgroup per element with a __shared__ PL after load_consts; an Fq12 crosses in the
// flat w-basis (6 Fq2, coefficient of w^k at k) and is loaded into a register of L.reg with its xi
// half made by w_fill_xi; the output is all 12 slots of the destination register.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../plonk-by-fingers_amd/csrc/pairing.hip"

namespace {
using namespace pbf;

enum Op : int {
  // ---- one thread per element
  F2_MUL = 0,     // a: Fq2, b: Fq2              out: Fq2
  F2_SQR,         // a: Fq2                      out: Fq2
  F2_MUL_XI,      // a: Fq2                      out: Fq2
  F2_INV,         // a: Fq2 (not 0)              out: Fq2
  F2_NEG,         // a: Fq2                      out: Fq2
  F2_CONJ,        // a: Fq2                      out: Fq2
  F2_MULS,        // a: Fq2, b: Fq               out: Fq2
  FQ_INV_RAW,     // a: raw                      out: raw (fq_inv of the value as it is)
  FQ_MUL_RAW,     // a: raw < 2q, b: raw < 2q    out: raw (Fq::mul as wm_r1 calls it)
  L9_REDUCE,      // a: L9                       out: raw
  F6_MUL,         // a: Fq6, b: Fq6              out: Fq6
  F6_MUL_01,      // a: Fq6, b: b0, b1           out: Fq6
  F6_INV,         // a: Fq6 (not 0)              out: Fq6
  F12_MUL,        // a: Fq12, b: Fq12            out: Fq12
  F12_SQR,        // a: Fq12                     out: Fq12
  F12_MUL_LINE,   // a: Fq12, b: A0, B0, B1      out: Fq12
  F12_CONJ,       // a: Fq12                     out: Fq12
  F12_FROB1,      // a: Fq12                     out: Fq12
  F12_FROB2,      // a: Fq12                     out: Fq12
  F12_CSQR,       // a: Fq12 (cyclotomic)        out: Fq12
  F12_FINAL_EXP,  // a: Fq12 (not 0)             out: Fq12, through a local Fq12 R[FE_SEQ_REGS]
  // ---- one workgroup per element. Products: a = x | y, b unused; p0 = which registers coincide:
  //   0 dst, x, y distinct    1 dst == x    2 dst == y    3 dst == x == y (y on the wire ignored)
  // y's coefficients beyond the shape's (W_LINE: 3, at w^0, w^1, w^3; W_FIVE: 5) are loaded as
  // they come and must not matter.
  W_MUL_DENSE = 40,  // out: 12 slots
  W_MUL_LINE,
  W_MUL_FIVE,
  // Two products in one set of rounds: a = xA | yA, b = xB | yB, out: dA's 12 slots | dB's 12 slots.
  // p0 as above for both products at once, and
  //   4 dA == xB, the rest distinct
  //   5 dA == xA == yA == yB, dB == xB (the square-and-multiply round of make_fe_prog's powu;
  //     yA and yB on the wire ignored)
  W_DUAL,            // w_mul_dual<false>
  W_DUAL_NEG,        // w_mul_dual<true>
  W_PAIR_DENSE_FIVE, // w_mul_pair<W_DENSE, W_FIVE>
  // One operand, a: flat Fq12, out: 12 slots; p0 = 0 dst distinct, 1 dst == x
  W_FROB1 = 50,
  W_FROB2,
  W_CONJ,
  W_ONE,    // the register holds a before w_one overwrites it
  W_INVN,   // fq6_inv_flat on slots 0, 2, 4 (1, 3, 5 as they come), then w_fill_xi: the FE_INVN step
  WM_R3,    // a: S0, S1, S2 (3 x L9), placed at every k: out raw, slot k = (wave 0, wave 1),
            // slot 6 + k = (wave 2, wave 3)
  W_FINAL_EXP,  // final_exp_w on reg[0]
};

struct Ctx {
  const uint64_t* a;
  const uint64_t* b;
  uint64_t* out;
  size_t n;
  uint32_t p0;
  PairingConsts k;
};

__device__ __forceinline__ U256 ld_m(const uint64_t* p) { return Fq::to_mont(u256_from_u64(p)); }
__device__ __forceinline__ void st_raw(uint64_t* p, const U256& v) {
  if (Fq::geq_p(v)) {
    for (int i = 0; i < 4; ++i) p[i] = ~0ull;
    return;
  }
  u256_to_u64(v, p);
}
__device__ __forceinline__ void st_p(uint64_t* p, const U256& v) {
  if (Fq::geq_p(v)) {
    for (int i = 0; i < 4; ++i) p[i] = ~0ull;
    return;
  }
  u256_to_u64(Fq::from_mont(v), p);
}
__device__ __forceinline__ Fq2 ld_f2(const uint64_t* p) { return Fq2{ld_m(p), ld_m(p + 4)}; }
__device__ __forceinline__ void st_f2(uint64_t* p, const Fq2& v) { st_p(p, v.c0), st_p(p + 4, v.c1); }
__device__ __forceinline__ Fq6 ld_f6(const uint64_t* p) { return Fq6{ld_f2(p), ld_f2(p + 8), ld_f2(p + 16)}; }
__device__ __forceinline__ void st_f6(uint64_t* p, const Fq6& v) { st_f2(p, v.c0), st_f2(p + 8, v.c1), st_f2(p + 16, v.c2); }
__device__ __forceinline__ Fq12 ld_f12(const uint64_t* p) { return Fq12{ld_f6(p), ld_f6(p + 24)}; }
__device__ __forceinline__ void st_f12(uint64_t* p, const Fq12& v) { st_f6(p, v.c0), st_f6(p + 24, v.c1); }
__device__ __forceinline__ L9 ld_l9(const uint64_t* p) {
  L9 r;
#pragma unroll
  for (int l = 0; l < 9; ++l) r.w[l] = (uint32_t)(p[l >> 1] >> (32 * (l & 1)));
  return r;
}

template <int OP>
__global__ void __launch_bounds__(64) pdc_lane_kernel(Ctx c) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= c.n) return;
  if constexpr (OP == F2_MUL) st_f2(c.out + 8 * i, f2_mul(ld_f2(c.a + 8 * i), ld_f2(c.b + 8 * i)));
  if constexpr (OP == F2_SQR) st_f2(c.out + 8 * i, f2_sqr(ld_f2(c.a + 8 * i)));
  if constexpr (OP == F2_MUL_XI) st_f2(c.out + 8 * i, f2_mul_xi(ld_f2(c.a + 8 * i)));
  if constexpr (OP == F2_INV) st_f2(c.out + 8 * i, f2_inv(ld_f2(c.a + 8 * i), c.k));
  if constexpr (OP == F2_NEG) st_f2(c.out + 8 * i, f2_neg(ld_f2(c.a + 8 * i)));
  if constexpr (OP == F2_CONJ) st_f2(c.out + 8 * i, f2_conj(ld_f2(c.a + 8 * i)));
  if constexpr (OP == F2_MULS) st_f2(c.out + 8 * i, f2_muls(ld_f2(c.a + 8 * i), ld_m(c.b + 4 * i)));
  if constexpr (OP == FQ_INV_RAW) st_raw(c.out + 4 * i, fq_inv(u256_from_u64(c.a + 4 * i), c.k));
  if constexpr (OP == FQ_MUL_RAW) st_raw(c.out + 4 * i, Fq::mul(u256_from_u64(c.a + 4 * i), u256_from_u64(c.b + 4 * i)));
  if constexpr (OP == L9_REDUCE) st_raw(c.out + 4 * i, l9_reduce(ld_l9(c.a + 5 * i)));
  if constexpr (OP == F6_MUL) st_f6(c.out + 24 * i, f6_mul(ld_f6(c.a + 24 * i), ld_f6(c.b + 24 * i)));
  if constexpr (OP == F6_MUL_01)
    st_f6(c.out + 24 * i, f6_mul_01(ld_f6(c.a + 24 * i), ld_f2(c.b + 16 * i), ld_f2(c.b + 16 * i + 8)));
  if constexpr (OP == F6_INV) st_f6(c.out + 24 * i, f6_inv(ld_f6(c.a + 24 * i), c.k));
  if constexpr (OP == F12_MUL) st_f12(c.out + 48 * i, f12_mul(ld_f12(c.a + 48 * i), ld_f12(c.b + 48 * i)));
  if constexpr (OP == F12_SQR) st_f12(c.out + 48 * i, f12_sqr(ld_f12(c.a + 48 * i)));
  if constexpr (OP == F12_MUL_LINE) {
    const uint64_t* l = c.b + 24 * i;
    st_f12(c.out + 48 * i, f12_mul_line(ld_f12(c.a + 48 * i), ld_f2(l), ld_f2(l + 8), ld_f2(l + 16)));
  }
  if constexpr (OP == F12_CONJ) st_f12(c.out + 48 * i, f12_conj(ld_f12(c.a + 48 * i)));
  if constexpr (OP == F12_FROB1) st_f12(c.out + 48 * i, f12_frob1(ld_f12(c.a + 48 * i), c.k));
  if constexpr (OP == F12_FROB2) st_f12(c.out + 48 * i, f12_frob2(ld_f12(c.a + 48 * i), c.k));
  if constexpr (OP == F12_CSQR) st_f12(c.out + 48 * i, f12_csqr(ld_f12(c.a + 48 * i)));
  if constexpr (OP == F12_FINAL_EXP) {
    Fq12 R[FE_SEQ_REGS];
    R[0] = ld_f12(c.a + 48 * i);
    f12_final_exp(R, c.k);
    st_f12(c.out + 48 * i, R[0]);
  }
}

// a flat Fq12 from the wire into a register, xi half included (all threads; ends with a barrier)
__device__ __forceinline__ void load_reg(Fq2* d, const uint64_t* p, int tid) {
  if (tid < 6) d[tid] = ld_f2(p + 8 * tid);
  bsync();
  w_fill_xi(d, tid);
}
__device__ __forceinline__ void store_reg(uint64_t* o, const Fq2* d, int tid, bool raw = false) {
  if (tid < 24) {
    const Fq2& s = d[tid >> 1];
    const U256 v = (tid & 1) ? s.c1 : s.c0;
    if (raw) st_raw(o + 4 * tid, v);
    else st_p(o + 4 * tid, v);
  }
}

template <int OP>
__global__ void __launch_bounds__(PT) pdc_wg_kernel(Ctx c) {
  __shared__ PL L;
  const int tid = threadIdx.x;
  const size_t i = blockIdx.x;
  if (i >= c.n) return;  // uniform
  load_consts(c.k, L, tid);
  const uint32_t al = c.p0;
  if constexpr (OP == W_MUL_DENSE || OP == W_MUL_LINE || OP == W_MUL_FIVE) {
    const uint64_t* a = c.a + 96 * i;
    Fq2* x = L.reg[0];
    Fq2* y = al == 3 ? x : L.reg[1];
    Fq2* d = al == 0 ? L.reg[2] : (al == 2 ? y : x);
    load_reg(x, a, tid);
    if (al != 3) load_reg(y, a + 48, tid);
    if constexpr (OP == W_MUL_DENSE) w_mul<W_DENSE>(d, x, y, L, tid);
    if constexpr (OP == W_MUL_LINE) w_mul<W_LINE>(d, x, y, L, tid);
    if constexpr (OP == W_MUL_FIVE) w_mul<W_FIVE>(d, x, y, L, tid);
    store_reg(c.out + 96 * i, d, tid);
  }
  if constexpr (OP == W_DUAL || OP == W_DUAL_NEG || OP == W_PAIR_DENSE_FIVE) {
    const uint64_t* a = c.a + 96 * i;
    const uint64_t* b = c.b + 96 * i;
    Fq2 *xA = L.reg[0], *yA = L.reg[1], *xB = L.reg[2], *yB = L.reg[3], *dA = L.reg[4], *dB = L.reg[5];
    if (al == 1) dA = xA, dB = xB;
    if (al == 2) dA = yA, dB = yB;
    if (al == 3) yA = xA, dA = xA, yB = xB, dB = xB;
    if (al == 4) dA = xB;
    if (al == 5) yA = xA, dA = xA, yB = xA, dB = xB;
    load_reg(L.reg[0], a, tid);
    load_reg(L.reg[1], a + 48, tid);
    load_reg(L.reg[2], b, tid);
    load_reg(L.reg[3], b + 48, tid);
    if constexpr (OP == W_DUAL) w_mul_dual<false>(dA, xA, yA, dB, xB, yB, L, tid);
    if constexpr (OP == W_DUAL_NEG) w_mul_dual<true>(dA, xA, yA, dB, xB, yB, L, tid);
    if constexpr (OP == W_PAIR_DENSE_FIVE) w_mul_pair<W_DENSE, W_FIVE>(dA, xA, yA, dB, xB, yB, L, tid);
    store_reg(c.out + 192 * i, dA, tid);
    store_reg(c.out + 192 * i + 96, dB, tid);
  }
  if constexpr (OP == W_FROB1 || OP == W_FROB2 || OP == W_CONJ || OP == W_ONE || OP == W_INVN) {
    Fq2* x = L.reg[0];
    Fq2* d = al == 1 ? x : L.reg[1];
    load_reg(x, c.a + 48 * i, tid);
    if constexpr (OP == W_FROB1) w_frob1(d, x, L, tid);
    if constexpr (OP == W_FROB2) w_frob2(d, x, L, tid);
    if constexpr (OP == W_CONJ) w_conj(d, x, tid);
    if constexpr (OP == W_ONE) {
      d = x;
      w_one(d, c.k, tid);
    }
    if constexpr (OP == W_INVN) {  // final_exp_w's FE_INVN step, in place
      d = x;
      if (tid == 0) fq6_inv_flat(d, c.k);
      bsync();
      w_fill_xi(d, tid);
    }
    store_reg(c.out + 96 * i, d, tid);
  }
  if constexpr (OP == WM_R3) {
    if (tid < 18) {
      const int k = tid / 3, s = tid - 3 * k;
      st16_l9(&L.acc[0][k][s], ld_l9(c.a + 15 * i + 5 * s));
    }
    bsync();
    const int wv = tid >> 6, k = tid & 63;
    if (k < 6) wm_r3(L.reg[0], L.acc[0], wv, k);
    bsync();
    store_reg(c.out + 96 * i, L.reg[0], tid, true);
  }
  if constexpr (OP == W_FINAL_EXP) {
    load_reg(L.reg[0], c.a + 48 * i, tid);
    final_exp_w(c.k, L, tid);
    store_reg(c.out + 96 * i, L.reg[0], tid);
  }
}

// ---- host side --------------------------------------------------------------------------------
struct Layout {
  int aw, bw, ow, wg;
};
bool layout_of(int op, uint64_t p0, Layout* l) {
  switch (op) {
    case F2_MUL: *l = {8, 8, 8, 0}; return true;
    case F2_SQR:
    case F2_MUL_XI:
    case F2_INV:
    case F2_NEG:
    case F2_CONJ: *l = {8, 0, 8, 0}; return true;
    case F2_MULS: *l = {8, 4, 8, 0}; return true;
    case FQ_INV_RAW: *l = {4, 0, 4, 0}; return true;
    case FQ_MUL_RAW: *l = {4, 4, 4, 0}; return true;
    case L9_REDUCE: *l = {5, 0, 4, 0}; return true;
    case F6_MUL: *l = {24, 24, 24, 0}; return true;
    case F6_MUL_01: *l = {24, 16, 24, 0}; return true;
    case F6_INV: *l = {24, 0, 24, 0}; return true;
    case F12_MUL: *l = {48, 48, 48, 0}; return true;
    case F12_MUL_LINE: *l = {48, 24, 48, 0}; return true;
    case F12_SQR:
    case F12_CONJ:
    case F12_FROB1:
    case F12_FROB2:
    case F12_CSQR:
    case F12_FINAL_EXP: *l = {48, 0, 48, 0}; return true;
    case W_MUL_DENSE:
    case W_MUL_LINE:
    case W_MUL_FIVE: *l = {96, 0, 96, 1}; return p0 <= 3;
    case W_DUAL:
    case W_DUAL_NEG:
    case W_PAIR_DENSE_FIVE: *l = {96, 96, 192, 1}; return p0 <= 5;
    case W_FROB1:
    case W_FROB2:
    case W_CONJ: *l = {48, 0, 96, 1}; return p0 <= 1;
    case W_ONE:
    case W_INVN:
    case W_FINAL_EXP: *l = {48, 0, 96, 1}; return p0 == 0;
    case WM_R3: *l = {15, 0, 96, 1}; return p0 == 0;
    default: return false;
  }
}

template <int OP>
void launch(const Ctx& c) {
  hipLaunchKernelGGL(pdc_lane_kernel<OP>, dim3((unsigned)((c.n + 63) / 64)), dim3(64), 0, 0, c);
}
template <int OP>
void launch_wg(const Ctx& c) {
  hipLaunchKernelGGL(pdc_wg_kernel<OP>, dim3((unsigned)c.n), dim3(PT), 0, 0, c);
}
void dispatch(int op, const Ctx& c) {
  switch (op) {
    case F2_MUL: return launch<F2_MUL>(c);
    case F2_SQR: return launch<F2_SQR>(c);
    case F2_MUL_XI: return launch<F2_MUL_XI>(c);
    case F2_INV: return launch<F2_INV>(c);
    case F2_NEG: return launch<F2_NEG>(c);
    case F2_CONJ: return launch<F2_CONJ>(c);
    case F2_MULS: return launch<F2_MULS>(c);
    case FQ_INV_RAW: return launch<FQ_INV_RAW>(c);
    case FQ_MUL_RAW: return launch<FQ_MUL_RAW>(c);
    case L9_REDUCE: return launch<L9_REDUCE>(c);
    case F6_MUL: return launch<F6_MUL>(c);
    case F6_MUL_01: return launch<F6_MUL_01>(c);
    case F6_INV: return launch<F6_INV>(c);
    case F12_MUL: return launch<F12_MUL>(c);
    case F12_SQR: return launch<F12_SQR>(c);
    case F12_MUL_LINE: return launch<F12_MUL_LINE>(c);
    case F12_CONJ: return launch<F12_CONJ>(c);
    case F12_FROB1: return launch<F12_FROB1>(c);
    case F12_FROB2: return launch<F12_FROB2>(c);
    case F12_CSQR: return launch<F12_CSQR>(c);
    case F12_FINAL_EXP: return launch<F12_FINAL_EXP>(c);
    case W_MUL_DENSE: return launch_wg<W_MUL_DENSE>(c);
    case W_MUL_LINE: return launch_wg<W_MUL_LINE>(c);
    case W_MUL_FIVE: return launch_wg<W_MUL_FIVE>(c);
    case W_DUAL: return launch_wg<W_DUAL>(c);
    case W_DUAL_NEG: return launch_wg<W_DUAL_NEG>(c);
    case W_PAIR_DENSE_FIVE: return launch_wg<W_PAIR_DENSE_FIVE>(c);
    case W_FROB1: return launch_wg<W_FROB1>(c);
    case W_FROB2: return launch_wg<W_FROB2>(c);
    case W_CONJ: return launch_wg<W_CONJ>(c);
    case W_ONE: return launch_wg<W_ONE>(c);
    case W_INVN: return launch_wg<W_INVN>(c);
    case WM_R3: return launch_wg<WM_R3>(c);
    case W_FINAL_EXP: return launch_wg<W_FINAL_EXP>(c);
  }
}

constexpr size_t MAX_COUNT = 1 << 16;

int run(int op, uint64_t p0, const void* a, const void* b, void* out, size_t count) {
  Layout l;
  if (!layout_of(op, p0, &l)) return -1;
  if (count == 0) return 0;
  if (count > MAX_COUNT || !a || !out || (l.bw && !b)) return -1;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  if (ensure_inv2k(dev) != 0) {  // the unit's own table builder, into this unit's g_inv2k
    e = hipGetLastError();
    return e == hipSuccess ? (int)hipErrorUnknown : (int)e;
  }
  const size_t na = count * l.aw * 8, nb = count * l.bw * 8, no = count * l.ow * 8;
  void *da = nullptr, *db = nullptr, *dout = nullptr;
  e = hipMalloc(&da, na);
  if (e == hipSuccess && nb) e = hipMalloc(&db, nb);
  if (e == hipSuccess) e = hipMalloc(&dout, no);
  if (e == hipSuccess) e = hipMemcpy(da, a, na, hipMemcpyHostToDevice);
  if (e == hipSuccess && nb) e = hipMemcpy(db, b, nb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0xA5, no);
  if (e == hipSuccess) {
    dispatch(op, Ctx{(const uint64_t*)da, (const uint64_t*)db, (uint64_t*)dout, count, (uint32_t)p0, make_consts()});
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
// p0: which registers of a workgroup op coincide (see Op); p1 is unused (the signature of fdc_run)
int pdc_run(int op, uint64_t p0, uint64_t p1, const void* a, const void* b, void* out, size_t count) {
  (void)p1;
  return run(op, p0, a, b, out, count);
}
// 64-bit words per element of a, b, out, and 1 for a workgroup op
int pdc_layout(int op, uint64_t p0, uint64_t p1, int* layout4) {
  (void)p1;
  Layout l;
  if (!layout4 || !layout_of(op, p0, &l)) return -1;
  layout4[0] = l.aw, layout4[1] = l.bw, layout4[2] = l.ow, layout4[3] = l.wg;
  return 0;
}
}
