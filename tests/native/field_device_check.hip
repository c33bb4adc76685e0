// Test-only device harness for the field headers of csrc/ (tests/test_field_device_gpu.py).
//
// Every kernel here runs ONE product function (or one composition of product functions that
// the kernels of csrc/ use) per thread on operands the caller chose, and stores what it
// returned: the arithmetic itself lives only in field.hpp, fp256.hpp, fr29.hpp, msm_l29.hpp,
// ntt_kernels.hpp and ntt_gl.hpp, which are included unchanged. The Python test compares the
// outputs with integer arithmetic, bit for bit. Never linked into libpbf.so.
//
//   int fdc_run(int op, uint64_t p0, uint64_t p1, const void* a, const void* b, void* out, size_t count)
//
// takes host pointers; allocates, copies in, launches (one thread per element, 256-thread
// blocks), synchronises, copies out, frees; returns the HIP error code (0 = success), -1 for
// an unknown op or a parameter outside the instantiated range. Compile-time parameters are
// picked from p0 / p1 by a fold over an integer sequence. Element layouts are in the op table
// at the end of the file (fdc_layout reports them to the caller).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <utility>

#include "../../plonk-by-fingers_amd/csrc/ntt_gl.hpp"
#include "../../plonk-by-fingers_amd/csrc/fr29.hpp"

namespace {
using namespace pbf;
using l29::L29;

// ntt_kernels.hpp defines this static kernel and the harness launches no whole pass: naming it
// keeps -Wall's unused-function check on for the harness's own functions
[[maybe_unused]] const void* const kHeaderKernelNotLaunched = (const void*)&shard_unsplit_kernel;

enum Op : int {
  GL_ADD = 0, GL_SUB, GL_MUL, GL_REDUCE128, GL_ADD_MUL_EPS, GL_MUL_POW2, GL_DIV_POW2, GL_POW2, GL_POW2_ABS,
  DFT_REG = 10, DFT_REG_TABLE, DFT_STAGE_B, DFT_POST_TWIDDLE_BR, DFT_RG3_C_SHIFT,
  M32_ADD = 20, M32_SUB, M32_MUL,
  FP_ADD = 30, FP_SUB, FP_REDUCE_ONCE, FP_MUL, FP_MUL_TP, FP_MUL2, FP_MULN3, FP_MULN4, FP_TO_MONT, FP_FROM_MONT,
  FR29_MUL = 50, FR29_ADD, FR29_SUB,
  L29_RELIMB = 60, L29_MUL, L29_SQR, L29_MULSUB, L29_MUL_SHIFT_SUB, L29_NORM, L29_SUB, L29_CANON, L29_ZERO_MOD_P,
  L29_TIMES32
};

// An op: AW / BW / OW = 64-bit words per element of a, b, out (BW = 0: b unused); BSH != 0: b is
// one table of BSH words shared by every thread. run() handles element i of n.
struct Ctx {
  const uint64_t* a;
  const uint64_t* b;
  uint64_t* out;
  size_t n;
  FieldArgs f;
};

template <class O>
__global__ void __launch_bounds__(256) fdc_kernel(Ctx c) {
#ifdef __HIP_DEVICE_COMPILE__  // the host pass must not instantiate calls of device-only templates (mulN)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < c.n) O::run(c, i);
#endif
}

// ---- Goldilocks scalars ------------------------------------------------------------------
template <int W_A, int W_B, int W_O, int W_BSH = 0>
struct Shape {
  static constexpr int AW = W_A, BW = W_B, OW = W_O, BSH = W_BSH;
};
struct GlAdd : Shape<1, 1, 1> {
  __device__ static void run(const Ctx& c, size_t i) { c.out[i] = Goldilocks::add(c.a[i], c.b[i], c.f); }
};
struct GlSub : Shape<1, 1, 1> {
  __device__ static void run(const Ctx& c, size_t i) { c.out[i] = Goldilocks::sub(c.a[i], c.b[i], c.f); }
};
struct GlMul : Shape<1, 1, 1> {
  __device__ static void run(const Ctx& c, size_t i) { c.out[i] = Goldilocks::mul(c.a[i], c.b[i], c.f); }
};
struct GlReduce128 : Shape<1, 1, 1> {
  __device__ static void run(const Ctx& c, size_t i) { c.out[i] = Goldilocks::reduce128(c.a[i], c.b[i]); }
};
struct GlAddMulEps : Shape<1, 1, 1> {
  __device__ static void run(const Ctx& c, size_t i) { c.out[i] = Goldilocks::add_mul_eps(c.a[i], (uint32_t)c.b[i]); }
};
template <int S>
struct GlMulPow2 : Shape<1, 0, 1> {
  __device__ static void run(const Ctx& c, size_t i) { c.out[i] = Goldilocks::mul_pow2<S>(c.a[i]); }
};
template <int K>
struct GlDivPow2 : Shape<1, 0, 1> {
  __device__ static void run(const Ctx& c, size_t i) { c.out[i] = gl_div_pow2<K>(c.a[i]); }
};
template <int K>
struct GlPow2 : Shape<1, 0, 1> {
  __device__ static void run(const Ctx& c, size_t i) { c.out[i] = gl_pow2<K>(c.a[i]); }
};
template <int K>
struct GlPow2Abs : Shape<1, 0, 2> {  // out = {gl_pow2_abs<K>(x), gl_pow2_neg(K)}
  __device__ static void run(const Ctx& c, size_t i) {
    c.out[2 * i] = gl_pow2_abs<K>(c.a[i]);
    c.out[2 * i + 1] = gl_pow2_neg(K) ? 1 : 0;
  }
};

// ---- register DFT blocks: 16 values per thread ----------------------------------------------
__device__ __forceinline__ void ld16(const Ctx& c, size_t i, uint64_t* v) {
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = c.a[16 * i + k];
}
__device__ __forceinline__ void st16(const Ctx& c, size_t i, const uint64_t* v) {
#pragma unroll
  for (int k = 0; k < 16; ++k) c.out[16 * i + k] = v[k];
}
// 16 / 2^LOGQ independent 2^LOGQ-point DFTs over consecutive groups (as stages A and C run them)
template <int LOGQ, int E64>
struct DftReg : Shape<16, 0, 16> {
  __device__ static void run(const Ctx& c, size_t i) {
    uint64_t v[16];
    ld16(c, i, v);
#pragma unroll
    for (int g = 0; g < 16; g += 1 << LOGQ) dft_reg<Goldilocks, LOGQ, sub_root_exp(E64, LOGQ)>(v + g, nullptr, c.f);
    st16(c, i, v);
  }
};
struct DftRegTable : Shape<16, 1, 16, 8> {  // b = wq[m] = w_16^m, m < 8
  __device__ static void run(const Ctx& c, size_t i) {
    uint64_t v[16];
    ld16(c, i, v);
    dft_reg<Goldilocks, 4, sub_root_exp(-1, 4)>(v, c.b, c.f);
    st16(c, i, v);
  }
};
template <int E64, int Q1>
struct DftStageB : Shape<16, 0, 16> {
  __device__ static void run(const Ctx& c, size_t i) {
    uint64_t v[16];
    ld16(c, i, v);
    gl_stage_b_head<E64, Q1>(v);
    dft_reg_tail<Goldilocks, 4, sub_root_exp(E64, 4), GL_B_LEVELS>(v, c.f);
    st16(c, i, v);
  }
};
template <int E64, int Q>
struct DftPostTwiddleBr : Shape<16, 0, 16> {
  __device__ static void run(const Ctx& c, size_t i) {
    uint64_t v[16];
    ld16(c, i, v);
    gl_post_twiddle_br<E64, Q>(v);
    st16(c, i, v);
  }
};
template <int E64, int WV>
struct DftRg3CShift : Shape<16, 0, 16> {
  __device__ static void run(const Ctx& c, size_t i) {
    uint64_t v[16];
    ld16(c, i, v);
    gl_rg3_c_shift<E64, WV>(v);
    st16(c, i, v);
  }
};

// ---- Mod32 (FieldArgs{m, mu} from p0, p1) --------------------------------------------------------
struct M32Add : Shape<1, 1, 1> {
  __device__ static void run(const Ctx& c, size_t i) { c.out[i] = Mod32::add(c.a[i], c.b[i], c.f); }
};
struct M32Sub : Shape<1, 1, 1> {
  __device__ static void run(const Ctx& c, size_t i) { c.out[i] = Mod32::sub(c.a[i], c.b[i], c.f); }
};
struct M32Mul : Shape<1, 1, 1> {
  __device__ static void run(const Ctx& c, size_t i) { c.out[i] = Mod32::mul(c.a[i], c.b[i], c.f); }
};

// ---- 256-bit fields: an element is 4 words (the ABI layout) -----------------------------------
__device__ __forceinline__ U256 ld256(const uint64_t* p, size_t i) { return u256_from_u64(p + 4 * i); }
__device__ __forceinline__ void st256(uint64_t* p, size_t i, const U256& v) { u256_to_u64(v, p + 4 * i); }

template <class F>
struct FpAdd : Shape<4, 4, 4> {
  __device__ static void run(const Ctx& c, size_t i) { st256(c.out, i, F::add(ld256(c.a, i), ld256(c.b, i))); }
};
template <class F>
struct FpSub : Shape<4, 4, 4> {
  __device__ static void run(const Ctx& c, size_t i) { st256(c.out, i, F::sub(ld256(c.a, i), ld256(c.b, i))); }
};
template <class F>
struct FpReduceOnce : Shape<4, 0, 4> {
  __device__ static void run(const Ctx& c, size_t i) { st256(c.out, i, F::reduce_once(ld256(c.a, i))); }
};
template <class F>
struct FpMul : Shape<4, 4, 4> {
  __device__ static void run(const Ctx& c, size_t i) { st256(c.out, i, F::mul(ld256(c.a, i), ld256(c.b, i))); }
};
template <class F>
struct FpMulTp : Shape<4, 4, 4> {
  __device__ static void run(const Ctx& c, size_t i) { st256(c.out, i, F::mul_tp(ld256(c.a, i), ld256(c.b, i))); }
};
// products of elements i, i + 1, ... (mod n): out[N i + j] = a[i + j] b[i + j]
template <class F>
struct FpMul2 : Shape<4, 4, 8> {
  __device__ static void run(const Ctx& c, size_t i) {
    const size_t k = (i + 1) % c.n;
    U256 r, s;
    F::mul2(ld256(c.a, i), ld256(c.b, i), ld256(c.a, k), ld256(c.b, k), &r, &s);
    st256(c.out, 2 * i, r);
    st256(c.out, 2 * i + 1, s);
  }
};
// ALIAS: the outputs are the x operands themselves (fp256.hpp: inputs may alias outputs)
template <class F, int N, int ALIAS>
struct FpMulN : Shape<4, 4, 4 * N> {
  __device__ static void run(const Ctx& c, size_t i) {
    U256 x[N], y[N], o[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      x[j] = ld256(c.a, (i + j) % c.n);
      y[j] = ld256(c.b, (i + j) % c.n);
    }
    const U256* xp[N];
    const U256* yp[N];
    U256* op[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      xp[j] = &x[j];
      yp[j] = &y[j];
      op[j] = ALIAS ? &x[j] : &o[j];
    }
    F::template mulN<N>(xp, yp, op);
#pragma unroll
    for (int j = 0; j < N; ++j) st256(c.out, N * i + j, ALIAS ? x[j] : o[j]);
  }
};
template <class F>
struct FpToMont : Shape<4, 0, 4> {
  __device__ static void run(const Ctx& c, size_t i) { st256(c.out, i, F::to_mont(ld256(c.a, i))); }
};
template <class F>
struct FpFromMont : Shape<4, 0, 4> {
  __device__ static void run(const Ctx& c, size_t i) { st256(c.out, i, F::from_mont(ld256(c.a, i))); }
};

// ---- fr29: an element of a / b is TWO canonical values (x0, x1); lazy operands are built from
// them with the header's own add / reduce / mul, so the ranges its comments state are entered
struct Fr29Mul : Shape<8, 8, 4> {  // canon(mul(a0, b0)) = a0 b0 2^-261
  __device__ static void run(const Ctx& c, size_t i) {
    st256(c.out, i, fr29::canon(fr29::mul(l29::from_u256(ld256(c.a, 2 * i)), l29::from_u256(ld256(c.b, 2 * i)))));
  }
};
struct Fr29Add : Shape<8, 8, 4> {  // canon(reduce((a0 + a1) + (b0 + b1))): below 4 r, limbs below 2^31
  __device__ static void run(const Ctx& c, size_t i) {
    const L29 A = fr29::add(l29::from_u256(ld256(c.a, 2 * i)), l29::from_u256(ld256(c.a, 2 * i + 1)));
    const L29 B = fr29::add(l29::from_u256(ld256(c.b, 2 * i)), l29::from_u256(ld256(c.b, 2 * i + 1)));
    st256(c.out, i, fr29::canon(fr29::reduce(fr29::add(A, B))));
  }
};
// canon(reduce(A + B - b)), A = a0 + a1 (limbs below 2^30), b as the radix-4 stage gives it:
//   B2R: b = mul(b0, b1), a product's output (normalised, below 2 r)
//   B4R: b = reduce(b0 + b1), a stage input (normalised, below 2 r + 2^234)
//   B8R: b = reduce(b0 + b1) + reduce(b0 + b0), a sum of two stage inputs (limbs below 2^30)
template <int M>
struct Fr29Sub : Shape<8, 8, 4> {
  __device__ static void run(const Ctx& c, size_t i) {
    const L29 A = fr29::add(l29::from_u256(ld256(c.a, 2 * i)), l29::from_u256(ld256(c.a, 2 * i + 1)));
    const L29 b0 = l29::from_u256(ld256(c.b, 2 * i)), b1 = l29::from_u256(ld256(c.b, 2 * i + 1));
    L29 d;
    if constexpr (M == 2) d = fr29::sub(A, fr29::mul(b0, b1), fr29::B2R);
    else if constexpr (M == 4) d = fr29::sub(A, fr29::reduce(fr29::add(b0, b1)), fr29::B4R);
    else d = fr29::sub(A, fr29::add(fr29::reduce(fr29::add(b0, b1)), fr29::reduce(fr29::add(b0, b0))), fr29::B8R);
    st256(c.out, i, fr29::canon(fr29::reduce(d)));
  }
};

// ---- l29 (Fq): operands cross as 256-bit integers; a result above 2 p leaves through a product
// by 2^266 (C266: the value times 2^5, below 2 p) and canon ------------------------------------------
__device__ __forceinline__ U256 l29_out(const L29& x) { return l29::to_u256(l29::canon(x)); }
__device__ __forceinline__ U256 l29_out32(const L29& x) { return l29_out(l29::mul(x, l29::konst(l29::C266))); }
struct L29Relimb : Shape<4, 0, 4> {  // any a < 2^256
  __device__ static void run(const Ctx& c, size_t i) { st256(c.out, i, l29::to_u256(l29::from_u256(ld256(c.a, i)))); }
};
// A lazily reduced operand from the values k, k + 1 of p. M = 0: the first, re-limbed (below
// 2^256 = 5.3 p); M = 8 / 16: l29::sub(x0, x1, M8P / M16P) = x0 + M p - x1, normalised, as the
// accumulation forms its differences: up to 13.3 p / 21.3 p, the caller keeps it below the bound
// the consumer states (17.3 p for a product's inputs, 11.3 p for X)
template <int M>
__device__ __forceinline__ L29 lazy(const uint64_t* p, size_t k) {
  const L29 x0 = l29::from_u256(ld256(p, k));
  if constexpr (M == 0) return x0;
  else return l29::sub(x0, l29::from_u256(ld256(p, k + 1)), M == 8 ? l29::M8P : l29::M16P);
}
template <int M>
struct L29Mul : Shape<8, 8, 4> {  // a b 2^-261 2^5, a = lazy<M>(a0, a1), b = lazy<M>(b0, b1)
  __device__ static void run(const Ctx& c, size_t i) {
    st256(c.out, i, l29_out32(l29::mul(lazy<M>(c.a, 2 * i), lazy<M>(c.b, 2 * i))));
  }
};
template <int M>
struct L29Sqr : Shape<8, 0, 4> {
  __device__ static void run(const Ctx& c, size_t i) { st256(c.out, i, l29_out32(l29::sqr(lazy<M>(c.a, 2 * i)))); }
};
// ((a b - c d) 2^-261 + p) 2^5; a = (a0, a1), b = (a2, a3), c = (b0, b1), d = b2. W = 0: the first
// value of each; W = 1: as madd's Y3 takes them, a, b = lazy<16> (below 17.3 p), c = lazy<8> (Y
// below 11.3 p), d = b2 (PPP below 3.3 p)
template <int W>
struct L29MulSub : Shape<16, 16, 4> {
  __device__ static void run(const Ctx& c, size_t i) {
    st256(c.out, i,
          l29_out32(l29::mulsub(lazy<W ? 16 : 0>(c.a, 4 * i), lazy<W ? 16 : 0>(c.a, 4 * i + 2),
                                lazy<W ? 8 : 0>(c.b, 4 * i), lazy<0>(c.b, 4 * i + 2))));
  }
};
// (a0 a1 2^-261 + E p - f) 2^5, E = 12 (f below 11.3 p) or 4 (f below 3.8 p); f = b0 (W = 0) or
// lazy<8>(b0, b1) (W = 1)
template <int E, int W>
struct L29MulShiftSub : Shape<8, 8, 4> {
  __device__ static void run(const Ctx& c, size_t i) {
    st256(c.out, i,
          l29_out32(l29::mul_shift_sub(lazy<0>(c.a, 2 * i), lazy<0>(c.a, 2 * i + 1), E == 12 ? l29::P12 : l29::P4,
                                       lazy<W ? 8 : 0>(c.b, 2 * i))));
  }
};
// norm of 16 p + a0 + a1 + b0 in redundant limbs (M16P's are above 2^31, each value adds up to
// 2^29 - 1: limbs up to 0xf85d977a, the value below 2^261), times 2^5
struct L29Norm : Shape<8, 4, 4> {
  __device__ static void run(const Ctx& c, size_t i) {
    const L29 s = fr29::add(fr29::add(l29::konst(l29::M16P), lazy<0>(c.a, 2 * i)),
                            fr29::add(lazy<0>(c.a, 2 * i + 1), lazy<0>(c.b, i)));
    st256(c.out, i, l29_out32(l29::norm(s)));
  }
};
template <int M>  // (a + M p - b) 2^5, M = 8 or 16, any a, b < 2^256
struct L29Sub : Shape<4, 4, 4> {
  __device__ static void run(const Ctx& c, size_t i) {
    st256(c.out, i,
          l29_out32(l29::sub(l29::from_u256(ld256(c.a, i)), l29::from_u256(ld256(c.b, i)), M == 8 ? l29::M8P : l29::M16P)));
  }
};
struct L29Canon : Shape<4, 0, 4> {  // a < 2 p
  __device__ static void run(const Ctx& c, size_t i) { st256(c.out, i, l29_out(l29::from_u256(ld256(c.a, i)))); }
};
struct L29ZeroModP : Shape<4, 0, 1> {  // a < 2 p
  __device__ static void run(const Ctx& c, size_t i) { c.out[i] = l29::zero_mod_p(l29::from_u256(ld256(c.a, i))) ? 1 : 0; }
};
struct L29Times32 : Shape<4, 0, 4> {  // a < p
  __device__ static void run(const Ctx& c, size_t i) { st256(c.out, i, l29_out(l29::times32(l29::from_u256(ld256(c.a, i))))); }
};

// ---- host side --------------------------------------------------------------------------------
struct Call {
  uint64_t p0, p1;
  const void* a;
  const void* b;
  void* out;
  size_t count;
  int* layout;  // != null: report {AW, BW, OW, BSH} instead of running
};

template <class O>
int launch(const Call& k) {
  if (k.layout) {
    k.layout[0] = O::AW, k.layout[1] = O::BW, k.layout[2] = O::OW, k.layout[3] = O::BSH;
    return 0;
  }
  if (k.count == 0) return 0;
  if (!k.a || !k.out || (O::BW && !k.b)) return -1;
  const size_t na = k.count * O::AW * 8, nb = O::BSH ? (size_t)O::BSH * 8 : k.count * O::BW * 8, no = k.count * O::OW * 8;
  void *da = nullptr, *db = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc(&da, na);
  if (e == hipSuccess && nb) e = hipMalloc(&db, nb);
  if (e == hipSuccess) e = hipMalloc(&dout, no);
  if (e == hipSuccess) e = hipMemcpy(da, k.a, na, hipMemcpyHostToDevice);
  if (e == hipSuccess && nb) e = hipMemcpy(db, k.b, nb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0xA5, no);
  if (e == hipSuccess) {
    Ctx c{(const uint64_t*)da, (const uint64_t*)db, (uint64_t*)dout, k.count, FieldArgs{k.p0, k.p1}};
    hipLaunchKernelGGL(fdc_kernel<O>, dim3((unsigned)((k.count + 255) / 256)), dim3(256), 0, 0, c);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(k.out, dout, no, hipMemcpyDeviceToHost);
  if (da) (void)hipFree(da);
  if (db) (void)hipFree(db);
  if (dout) (void)hipFree(dout);
  return (int)e;
}

// v in [LO, LO + N): run f(integral_constant<int, v>) -- one instantiation per value of the sequence
template <int LO, class Fn, int... I>
int pick_seq(uint64_t v, Fn&& fn, std::integer_sequence<int, I...>) {
  int rc = -1;
  (void)((v == (uint64_t)(LO + I) ? (rc = fn(std::integral_constant<int, LO + I>{}), true) : false) || ...);
  return rc;
}
template <int LO, int N, class Fn>
int pick(uint64_t v, Fn&& fn) {
  return pick_seq<LO>(v, fn, std::make_integer_sequence<int, N>{});
}
// E64 in {39, 153}: w_64 = 2^39 and its inverse, the two values the pass kernels are built for
template <class Fn>
int pick_e64(uint64_t e64, Fn&& fn) {
  if (e64 == 39) return fn(std::integral_constant<int, 39>{});
  if (e64 == 153) return fn(std::integral_constant<int, 153>{});
  return -1;
}
template <template <class> class O>
int fp_launch(const Call& k) {
  return k.p0 == 0 ? launch<O<Fr>>(k) : k.p0 == 1 ? launch<O<Fq>>(k) : -1;
}
template <int N>
int fp_launch_n(const Call& k) {
  if (k.p0 > 1 || k.p1 > 1) return -1;
  if (k.p0 == 0) return k.p1 ? launch<FpMulN<Fr, N, 1>>(k) : launch<FpMulN<Fr, N, 0>>(k);
  return k.p1 ? launch<FpMulN<Fq, N, 1>>(k) : launch<FpMulN<Fq, N, 0>>(k);
}

int dispatch(int op, const Call& k) {
  switch (op) {
    case GL_ADD: return launch<GlAdd>(k);
    case GL_SUB: return launch<GlSub>(k);
    case GL_MUL: return launch<GlMul>(k);
    case GL_REDUCE128: return launch<GlReduce128>(k);
    case GL_ADD_MUL_EPS: return launch<GlAddMulEps>(k);
    case GL_MUL_POW2: return pick<0, 96>(k.p0, [&](auto s) { return launch<GlMulPow2<decltype(s)::value>>(k); });
    case GL_DIV_POW2: return pick<1, 32>(k.p0, [&](auto s) { return launch<GlDivPow2<decltype(s)::value>>(k); });
    case GL_POW2: return pick<0, 192>(k.p0, [&](auto s) { return launch<GlPow2<decltype(s)::value>>(k); });
    case GL_POW2_ABS: return pick<0, 192>(k.p0, [&](auto s) { return launch<GlPow2Abs<decltype(s)::value>>(k); });
    case DFT_REG:  // p0 = LOGQ 1..4, p1 = E64
      return pick<1, 4>(k.p0, [&](auto q) {
        return pick_e64(k.p1, [&](auto e) { return launch<DftReg<decltype(q)::value, decltype(e)::value>>(k); });
      });
    case DFT_REG_TABLE: return launch<DftRegTable>(k);
    case DFT_STAGE_B:  // p0 = E64, p1 = Q1 0..3
      return pick_e64(k.p0, [&](auto e) {
        return pick<0, 4>(k.p1, [&](auto q) { return launch<DftStageB<decltype(e)::value, decltype(q)::value>>(k); });
      });
    case DFT_POST_TWIDDLE_BR:  // p0 = E64, p1 = Q 1..3
      return pick_e64(k.p0, [&](auto e) {
        return pick<1, 3>(k.p1, [&](auto q) { return launch<DftPostTwiddleBr<decltype(e)::value, decltype(q)::value>>(k); });
      });
    case DFT_RG3_C_SHIFT:  // p0 = E64, p1 = WV 0..3
      return pick_e64(k.p0, [&](auto e) {
        return pick<0, 4>(k.p1, [&](auto q) { return launch<DftRg3CShift<decltype(e)::value, decltype(q)::value>>(k); });
      });
    case M32_ADD: return launch<M32Add>(k);
    case M32_SUB: return launch<M32Sub>(k);
    case M32_MUL: return launch<M32Mul>(k);
    case FP_ADD: return fp_launch<FpAdd>(k);
    case FP_SUB: return fp_launch<FpSub>(k);
    case FP_REDUCE_ONCE: return fp_launch<FpReduceOnce>(k);
    case FP_MUL: return fp_launch<FpMul>(k);
    case FP_MUL_TP: return fp_launch<FpMulTp>(k);
    case FP_MUL2: return fp_launch<FpMul2>(k);
    case FP_MULN3: return fp_launch_n<3>(k);
    case FP_MULN4: return fp_launch_n<4>(k);
    case FP_TO_MONT: return fp_launch<FpToMont>(k);
    case FP_FROM_MONT: return fp_launch<FpFromMont>(k);
    case FR29_MUL: return launch<Fr29Mul>(k);
    case FR29_ADD: return launch<Fr29Add>(k);
    case FR29_SUB:
      return k.p0 == 2 ? launch<Fr29Sub<2>>(k) : k.p0 == 4 ? launch<Fr29Sub<4>>(k) : k.p0 == 8 ? launch<Fr29Sub<8>>(k) : -1;
    case L29_RELIMB: return launch<L29Relimb>(k);
    case L29_MUL:  // p0 = 0, 8, 16: how the operands are formed (lazy<M>)
      return k.p0 == 0 ? launch<L29Mul<0>>(k) : k.p0 == 8 ? launch<L29Mul<8>>(k) : k.p0 == 16 ? launch<L29Mul<16>>(k) : -1;
    case L29_SQR:
      return k.p0 == 0 ? launch<L29Sqr<0>>(k) : k.p0 == 8 ? launch<L29Sqr<8>>(k) : k.p0 == 16 ? launch<L29Sqr<16>>(k) : -1;
    case L29_MULSUB: return k.p0 == 0 ? launch<L29MulSub<0>>(k) : k.p0 == 1 ? launch<L29MulSub<1>>(k) : -1;
    case L29_MUL_SHIFT_SUB:  // p0 = E (12, 4), p1 = W
      if (k.p0 == 12) return k.p1 == 0 ? launch<L29MulShiftSub<12, 0>>(k) : k.p1 == 1 ? launch<L29MulShiftSub<12, 1>>(k) : -1;
      return k.p0 == 4 && k.p1 == 0 ? launch<L29MulShiftSub<4, 0>>(k) : -1;
    case L29_NORM: return launch<L29Norm>(k);
    case L29_SUB: return k.p0 == 8 ? launch<L29Sub<8>>(k) : k.p0 == 16 ? launch<L29Sub<16>>(k) : -1;
    case L29_CANON: return launch<L29Canon>(k);
    case L29_ZERO_MOD_P: return launch<L29ZeroModP>(k);
    case L29_TIMES32: return launch<L29Times32>(k);
    default: return -1;
  }
}
}  // namespace

extern "C" {
// Mod32 ops: p0 = m, p1 = mu = floor(2^64 / m). Fp256 ops: p0 = 0 (Fr) / 1 (Fq); mulN: p1 = 1
// makes the outputs alias the x operands. Everything else: see dispatch().
int fdc_run(int op, uint64_t p0, uint64_t p1, const void* a, const void* b, void* out, size_t count) {
  return dispatch(op, Call{p0, p1, a, b, out, count, nullptr});
}
// 64-bit words per element of a, b, out, and the size of a shared b table (0: per element)
int fdc_layout(int op, uint64_t p0, uint64_t p1, int* layout4) {
  if (!layout4) return -1;
  return dispatch(op, Call{p0, p1, nullptr, nullptr, nullptr, 0, layout4});
}
}
