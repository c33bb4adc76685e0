// Goldilocks pass kernel for standard roots (gfx950) — the hot path of src/fft.rs
// CooleyTurkey (fft.rs:55-106) at BASELINE configs 2 and 5.
//
// Same Stockham-over-HBM pass structure as ntt_pass_kernel (ntt_kernels.hpp): pass input
// x[j + r*(n/R)], pre-twiddle w^((n/(Ns*R))*r*(j mod Ns)), an R-point DFT along r,
// output y[(j/Ns)*Ns*R + (j mod Ns) + k*Ns]. What differs is how the R-point DFT is
// split, chosen so that every general (table) multiplication that can be a shift is one:
//
//   R = 4 * 16 * C  (C = R/64),   r = 16C*s1 + C*s2 + r2,   k = q1 + 4*q2 + 64*k2
//   stage A  4-point DFT over s1                          -> Z[q1][s2][r2]
//   stage B  Z *= w_64^(s2*q1)  (a power of two: shift)   16-point DFT over s2
//                                                          -> Y[k1 = q1 + 4 q2][r2]
//   stage C  Y *= w_R^(r2*k1)   (table, general multiply)  C-point DFT over r2 -> X[k1 + 64 k2]
//
// For a standard root w (w_64 = 2^39, inverse 2^153) every root of order <= 64 is a
// power of two, so the 4-, 16- and C-point register DFTs and the stage-B twiddle are
// shift-reductions; only stage C's pre-twiddle (and the pass twiddle) multiply by
// table entries: one general multiplication per element per pass, the minimum for
// DFT blocks of <= 64 points (2^20 = 2 passes -> 3 general multiplications per
// element including the one pass twiddle; ntt_pass_kernel's 4|16|16 split needs 5).
//
// Stage B runs one q1 per wave (4 values, 2 waves each), so its twiddle exponents are
// compile-time constants under a wave-uniform switch. LDS layouts (elements of 8 B):
//   Z: ((q1*16 + s2)*C + r2)*W + w           (A writes and B reads 64 contiguous)
//   Y: r2*(65*W) + k1*W + w                  (B writes rows r2 padded by W: 2-pass
//                                             64-bit accesses; C reads contiguous)
// Tile: TILE = R x W elements (W = TILE/R columns: W*8 B contiguous runs in HBM), TILE/16
// threads, 16 elements per thread in every stage.
#pragma once
#include "ntt_kernels.hpp"

namespace pbf {

struct GlPassArgs {
  const uint64_t* in;
  uint64_t* out;
  const uint64_t* twpass;  // per-pass [r][k] table w^((n/(Ns*R))*r*k), or null (two-level)
  const uint64_t* tw0;     // two-level table of w (low part)
  const uint64_t* tw1;     //                     (high part)
  const uint64_t* tc;      // stage-C table [r2][k1] = w_R^(r2*k1) (times n^-1 when scaled)
  const uint64_t* tws_a;   // last pass, split twiddles: A[r][w] = w_p^(r*w)   (or null)
  const uint64_t* tws_b;   //                          B[kb][r] = w_p^(r*kb*W)
  uint64_t n;
  uint32_t log_n;
  uint32_t log_ns;
  uint32_t tw_bits;
  uint32_t blocks_per_poly;
  uint32_t batch;
  uint32_t scaled;         // tc carries n^-1: multiply every element, k1 = 0 / r2 = 0 too
  uint32_t out_split_log;  // != 0: store destination-major [n/S][batch][S] (multi-GPU send layout)
  uint32_t xcd_kmajor;     // XCD-aware column-major block order (pass-twiddle table reuse in L2)
  uint64_t in_pitch, out_pitch;  // elements from one polynomial to the next
  // two-pass plans: the first pass multiplies its outputs by the second pass's twiddle w^(j k)
  // (post_tw = that pass's [r][k] table: r = this pass's column j, k its output digit) and the
  // second pass skips its own (skip_pass_tw)
  const uint64_t* post_tw;
  uint32_t skip_pass_tw;
  // SP 2 (both passes of a "10,10" plan): the intermediate is tile-major, Yb[k >> 3][j][k & 7]
  // for the first pass's output y(j, k), one second-pass tile (8 columns k x 1024 rows j) per
  // contiguous block, blk_pitch elements from one block to the next; post_tw is in that order
  uint64_t blk_pitch;
  // coset variants (template parameter CS of the kernel). CS 1, the first pass
  // of a forward transform: polynomial `poly` is the cs_len coefficients at in + poly*in_pitch
  // (in_pitch = cs_len), element i loads times shift^i, and i >= cs_len is zero padding that is
  // never read. CS 2, the last pass of an inverse: output k stores times shift^-k n^-1 (tc
  // unscaled). The factor of index i is cs_tab[i], or, two-level (cs_tab1 != null),
  // cs_tab[i mod 2^cs_bits] * cs_tab1[i >> cs_bits].
  const uint64_t* cs_tab;
  const uint64_t* cs_tab1;
  uint32_t cs_bits;
  uint64_t cs_len;
};

// x * 2^(K mod 192) (mod p), K a compile-time exponent; 2^96 = -1. Exponents in
// (160, 192) are divisions by 2^(192-K) (no sign); a remaining sign costs one subtraction.
// 2^(K mod 192) = (-1)^gl_pow2_neg(K) * (what gl_pow2_abs<K> multiplies by)
__host__ __device__ constexpr bool gl_pow2_neg(int k) {
  const int raw = ((k % 192) + 192) % 192;
  return raw > 64 && raw <= 160;  // (64, 96): -2^-(96-raw); [96, 160]: -2^(raw-96)
}
template <int K>
__device__ __forceinline__ uint64_t gl_pow2_abs(uint64_t x) {
  constexpr int RAW = ((K % 192) + 192) % 192;
  if constexpr (RAW == 0) {
    return x;
  } else if constexpr (RAW > 160) {
    return gl_div_pow2<192 - RAW>(x);
  } else {
    using T = ShiftKind<RAW>;
    static_assert(T::NEG == gl_pow2_neg(K), "sign of 2^K");
    return apply_shift<Goldilocks, T>(x);
  }
}
template <int K>
__device__ __forceinline__ uint64_t gl_pow2(uint64_t x) {
  const uint64_t y = gl_pow2_abs<K>(x);
  if constexpr (gl_pow2_neg(K)) {
    const FieldArgs f{};
    return Goldilocks::sub(0, y, f);
  } else {
    return y;
  }
}

// Stage-B twiddle: v[s2] *= w_64^(s2*Q1) = 2^(E64*s2*Q1).
template <int E64, int Q1, int S2 = 1>
__device__ __forceinline__ void gl_stage_b_twiddle(uint64_t* v) {
  if constexpr (S2 < 16) {
    v[S2] = gl_pow2<(E64 * S2 * Q1) % 192>(v[S2]);
    gl_stage_b_twiddle<E64, Q1, S2 + 1>(v);
  }
}
// The same twiddle without its signs: v[s2] *= |2^(E64*s2*Q1)|, the negative powers (about half:
// 4 VALU each as 0 - y) left to the 16-point DFT that follows, which takes their mask
// gl_stage_b_negmask and folds every one of them into its butterflies (dft_reg_signed).
template <int E64, int Q1, int S2 = 1>
__device__ __forceinline__ void gl_stage_b_twiddle_abs(uint64_t* v) {
  if constexpr (S2 < 16) {
    v[S2] = gl_pow2_abs<(E64 * S2 * Q1) % 192>(v[S2]);
    gl_stage_b_twiddle_abs<E64, Q1, S2 + 1>(v);
  }
}
__host__ __device__ constexpr unsigned gl_stage_b_negmask(int e64, int q1) {
  unsigned m = 0;
  for (int s2 = 1; s2 < 16; ++s2) m |= gl_pow2_neg((e64 * s2 * q1) % 192) ? 1u << s2 : 0u;
  return m;
}
// Levels of stage B's 16-point DFT that run per q1 (inside the wave-uniform switch) to absorb
// the twiddle's signs: after two levels 0 / 1 / 1 (E64 = 39; 153: 2 / 2 / 1) of the 8 / 7 / 7
// (9 / 8 / 8) signs of q1 = 1 / 2 / 3 are left and are negated there; the last two levels are
// common code after the switch. (All four levels per q1 leave no sign at all but repeat the
// whole DFT four times, +14 KB of code per kernel, for the same measured VALU count and a
// step time 0.5 % higher; one level leaves 2 / 4 / 4: DESIGN.md §3.1 round 7.)
constexpr int GL_B_LEVELS = 2;
// stage B of one q1: twiddle and the first GL_B_LEVELS levels of the 16-point DFT over s2
template <int E64, int Q1>
__device__ __forceinline__ void gl_stage_b_head(uint64_t* v) {
  const FieldArgs f{};
  gl_stage_b_twiddle_abs<E64, Q1>(v);
  dft_reg_signed<Goldilocks, 4, sub_root_exp(E64, 4), gl_stage_b_negmask(E64, Q1), GL_B_LEVELS>(v, f);
}

// v[bitrev4(e)] *= w_64^(e*Q) = 2^(E64*e*Q): a twiddle on the bit-reversed outputs of a
// 16-point register DFT
template <int E64, int Q, int E = 1>
__device__ __forceinline__ void gl_post_twiddle_br(uint64_t* v) {
  if constexpr (E < 16) {
    v[bitrev_c(E, 4)] = gl_pow2<(E64 * E * Q) % 192>(v[bitrev_c(E, 4)]);
    gl_post_twiddle_br<E64, Q, E + 1>(v);
  }
}
// RG 3 stage C: x[u*4 + r2] *= w_64^(r2 g), g = WV + 4 u (r2 = 1..3, u = 0..3)
template <int E64, int WV, int U = 0>
__device__ __forceinline__ void gl_rg3_c_shift(uint64_t* x) {
  if constexpr (U < 4) {
    constexpr int g = WV + 4 * U;
    x[U * 4 + 1] = gl_pow2<(E64 * g) % 192>(x[U * 4 + 1]);
    x[U * 4 + 2] = gl_pow2<(E64 * 2 * g) % 192>(x[U * 4 + 2]);
    x[U * 4 + 3] = gl_pow2<(E64 * 3 * g) % 192>(x[U * 4 + 3]);
    gl_rg3_c_shift<E64, WV, U + 1>(x);
  }
}

template <int LOGR, int TILE>
struct GlShape {
  static constexpr int R = 1 << LOGR;
  static constexpr int LOGC = LOGR - 6;
  static constexpr int C = 1 << LOGC;
  static constexpr int W = TILE / R;
  static constexpr int NT = TILE / 16;             // 16 elements per thread
  static constexpr int WPQ = NT / 256;              // waves per stage-B q1 value
  // Y rows r2: padded by W (YP = 65 W) so that the four r2 rows of one stage-B write
  // instruction fall on both halves of the banks; for W = 16 the same spread comes from
  // XOR-ing k1's low bit with r2's (YX: no padding, a 4096-element tile is exactly 32 KiB and
  // five workgroups fit a CU)
  static constexpr bool YX = W == 16 && C > 1;
  static constexpr int YP = (YX ? 64 : 65) * W;     // Y row pitch (elements)
  static constexpr int LDS = (C * YP > TILE) ? C * YP : TILE;
  static constexpr bool LDS32K = LDS * 8 <= 32768;  // five workgroups per CU by LDS
  static constexpr int NSUB_C = (64 * W) / NT;      // stage-C sub-DFTs per thread
  // Y column swizzle: the first pass's stage C reads all 64 k1 of one column w per wave
  // (so its stores are 512-B runs of out[j*R + k]); w ^ ysw(k1) spreads those reads over
  // the banks, each 8-B bank pair hit twice per 512-B wave access (the minimum). Stage B's
  // writes and later passes' reads stay permutations within a row (conflict-free).
  __host__ __device__ static constexpr int ysw(int k1) {
    return W <= 32 ? (k1 / (32 / W)) & (W - 1) : (k1 & 31);
  }
  // Y element (r2, k1, w)
  __host__ __device__ static constexpr int yidx(int r2, int k1, int w) {
    return r2 * YP + (YX ? (k1 ^ (r2 & 1)) : k1) * W + (w ^ ysw(k1));
  }
};

// Tile id -> (polynomial, column block). With xcd_kmajor the tiles of one XCD (block ids
// congruent mod 8) take a contiguous range
// of column blocks, all polynomials of a block back to back, so each slice of the
// pass-twiddle table is fetched into that XCD's L2 once per pass, not once per polynomial.
__device__ __forceinline__ void gl_tile_coords(const GlPassArgs& a, uint32_t tile, uint32_t tiles, uint32_t* poly,
                                               uint32_t* kb) {
  if (a.xcd_kmajor == 1) {
    const uint32_t v = (tile & 7) * (tiles >> 3) + (tile >> 3);
    *kb = v / a.batch;
    *poly = v % a.batch;
  } else if (a.xcd_kmajor == 2) {
    // XCD-blocked, polynomial-major: workgroups resident together on one XCD take adjacent
    // column blocks, so the 128-B lines their W*8-B runs share are fetched into one L2
    const uint32_t v = (tile & 7) * (tiles >> 3) + (tile >> 3);
    *poly = v / a.blocks_per_poly;
    *kb = v % a.blocks_per_poly;
  } else {
    *poly = tile / a.blocks_per_poly;
    *kb = tile % a.blocks_per_poly;
  }
}

// coset factor of element i (GlPassArgs cs_tab)
__device__ __forceinline__ uint64_t gl_cs_factor(const GlPassArgs& a, uint64_t i) {
  const FieldArgs f{};
  if (a.cs_tab1) return Goldilocks::mul(a.cs_tab[i & ((1ull << a.cs_bits) - 1)], a.cs_tab1[i >> a.cs_bits], f);
  return a.cs_tab[i];
}

constexpr int GL_STORES = 16;  // global stores per thread per tile (NSUB_C * C)

// SP 2 exchanges the tile through LDS in two rounds of 32-bit halves (gl_tile), so its LDS
// block is half of GlShape::LDS * 8 B and three workgroups fit a CU
__host__ __device__ constexpr bool gl_split(int sp) { return sp == 2; }
typedef uint32_t gl_u32x2 __attribute__((ext_vector_type(2)));
// The 16 incoming words of one round, o[i] = the word at p + i * STRIDE / 4, one ds_read_b32 each
// and waited for. Written out because the compiler pairs such reads into ds_read2st64_b32, whose
// two results share a register pair: each word then needs a move into its half of its element's
// own pair (two moves per element and exchange, and 76 B of scratch per lane at 80 VGPRs).
#define GL_RD(i, off) "ds_read_b32 %" #i ", %16 offset:" #off "\n\t"
template <int STRIDE>
__device__ __forceinline__ void gl_lds_read16(const uint32_t* p, uint32_t* o) {
  static_assert(STRIDE == 512 || STRIDE == 2080, "the strides written out below: Z (C*W words), Y (YP words)");
  const uint32_t a = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint32_t*)p;
#define GL_RD_OUT                                                                                                   \
  "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7]), "=&v"(o[8]), \
      "=&v"(o[9]), "=&v"(o[10]), "=&v"(o[11]), "=&v"(o[12]), "=&v"(o[13]), "=&v"(o[14]), "=&v"(o[15])
  if constexpr (STRIDE == 512) {
    asm volatile(GL_RD(0, 0) GL_RD(1, 512) GL_RD(2, 1024) GL_RD(3, 1536) GL_RD(4, 2048) GL_RD(5, 2560) GL_RD(6, 3072)
                     GL_RD(7, 3584) GL_RD(8, 4096) GL_RD(9, 4608) GL_RD(10, 5120) GL_RD(11, 5632) GL_RD(12, 6144)
                         GL_RD(13, 6656) GL_RD(14, 7168) GL_RD(15, 7680) "s_waitcnt lgkmcnt(0)"
                 : GL_RD_OUT
                 : "v"(a)
                 : "memory");
  } else {
    asm volatile(GL_RD(0, 0) GL_RD(1, 2080) GL_RD(2, 4160) GL_RD(3, 6240) GL_RD(4, 8320) GL_RD(5, 10400) GL_RD(6, 12480)
                     GL_RD(7, 14560) GL_RD(8, 16640) GL_RD(9, 18720) GL_RD(10, 20800) GL_RD(11, 22880) GL_RD(12, 24960)
                         GL_RD(13, 27040) GL_RD(14, 29120) GL_RD(15, 31200) "s_waitcnt lgkmcnt(0)"
                 : GL_RD_OUT
                 : "v"(a)
                 : "memory");
  }
#undef GL_RD_OUT
}
#undef GL_RD

// The tile-major intermediate of SP 2: elements from one 8192-element block to the next. A pad
// that takes the 128 blocks a first-pass tile writes off the 64-KiB stride measured no faster
// (DESIGN.md §3.1 round 9), so the blocks are dense; a multiple of 2 keeps the 16-B loads aligned.
constexpr uint64_t GL_BLK_PITCH = 8192;
static_assert(GL_BLK_PITCH >= 8192 && GL_BLK_PITCH % 2 == 0, "block pitch");
typedef uint64_t gl_u64x2 __attribute__((ext_vector_type(2)));

// The global accesses of SP 2: the address is a wave-uniform 64-bit base, which carries the
// kernel's pointer, the polynomial, the tile and the stride of this access, plus one 32-bit byte
// offset per lane that all accesses of a family share. The base stays in scalar registers and is
// advanced by the scalar ALU (global_load / global_store with a scalar base and a 32-bit vector
// offset): no access forms a 64-bit address on the vector ALU or keeps one live. The offset is
// zero-extended, so every lane offset must stay below 2^32 bytes: here below one polynomial.
// The empty asm pins the finished base to a scalar register pair: without it the compiler takes
// the stride back out of the base, adds the lane offset first and the stride on the vector ALU.
// (The pointer that comes out of the asm is one to global memory by its type, not by inference.)
#define GL_GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ T gl_ld_sv(const void* sbase, uint32_t voff) {
  uint64_t b = (uint64_t)sbase;
  asm("" : "+s"(b));
  return *(const GL_GLOBAL T*)((const GL_GLOBAL char*)b + voff);
}
template <class T>
__device__ __forceinline__ void gl_st_sv(void* sbase, uint32_t voff, T x) {
  uint64_t b = (uint64_t)sbase;
  asm("" : "+s"(b));
  *(GL_GLOBAL T*)((GL_GLOBAL char*)b + voff) = x;
}
#undef GL_GLOBAL

// One tile: stages A, B, C and the stores.
// RG (regrouped 2^24 plan, ntt_gl_rg2_kernel below): 1 = its first pass, 3 = its last pass.
// CS (coset transforms): 1 = a first pass that scales its loads by shift^i and reads no zero
// padding, 2 = a last pass that scales its stores by shift^-k n^-1 (GlPassArgs cs_*).
// SP (the second pass of a plain forward two-pass plan, run_gl_group): the pass compiled with
// only what such a plan executes: no pass-twiddle code (the first pass applied it: post_tw),
// no scaled table and no split store. 1 = log_ns from the arguments. 0 = the generic
// kernel of every other pass and plan. (The first pass with post_tw unconditional measured
// no faster and 5.6 VALU per element more, DESIGN.md §3.1 round 7: it stays generic.)
// 2 = both passes of one radix 2^10 ("10,10"), FIRST or not, with the intermediate between them
// tile-major (GlPassArgs blk_pitch): the first pass's stage C takes 8 digits x 8 columns per
// wave, so that each of its wave stores (and post_tw loads) is the 512 contiguous bytes of one
// block; the second pass reads its tile as 64 contiguous KiB, 16 B per lane and load, and its
// log_ns is the constant LOGR (the index arithmetic of its stores folds to constants). Both
// exchange the tile through LDS in 32-bit halves, low words first (gl_split below: half the LDS,
// three workgroups per CU).
template <int LOGR, int E64, bool FIRST, int TILE, int RG = 0, int CS = 0, int SP = 0>
__device__ __forceinline__ void gl_tile(const GlPassArgs& a, uint64_t* lds, uint32_t tile, uint32_t tiles, int t) {
  using Sh = GlShape<LOGR, TILE>;
  constexpr int C = Sh::C, LOGC = Sh::LOGC, W = Sh::W, NT = Sh::NT, YP = Sh::YP;
  (void)YP;
  static_assert(Sh::NSUB_C * C == GL_STORES, "stores per thread");
  static_assert(SP == 0 || ((!FIRST || SP == 2) && RG == 0 && CS == 0 && SP <= 2), "SP: plain two-pass plan");
  static_assert(SP != 2 || (LOGR == 10 && TILE == 8192), "SP 2: the 10,10 plan");
  static_assert(RG == 0 || (LOGR == 8 && TILE == 4096 && FIRST == (RG == 1)), "RG shape");
  static_assert(CS == 0 || (FIRST == (CS == 1) && (RG == 0 || RG == 2 * CS - 1)), "CS 1: first pass, CS 2: last pass");
  const FieldArgs f{};
  using G = Goldilocks;
  uint32_t poly, kb;
  gl_tile_coords(a, tile, tiles, &poly, &kb);
  const uint64_t j0 = (uint64_t)kb * W;
  const uint64_t* in = a.in + (uint64_t)poly * a.in_pitch;
  const uint64_t stride = a.n >> LOGR;  // input rows (r) are n/R long
  constexpr bool BLK_IN = SP == 2 && !FIRST, BLK_OUT = SP == 2 && FIRST;
  // SP 2: both exchanges pass the low words of the tile through LDS first and the high words
  // second, in the same element indices (Z, yidx) on an array of 32-bit words half the size
  constexpr bool SPLIT = gl_split(SP);
  uint32_t* lds32 = (uint32_t*)lds;
  (void)lds32;

  // ---------------- stage A: load, pass twiddle, 4-point DFTs over s1
  uint64_t v[16];
  if constexpr (BLK_IN) {
    // the tile is block kb, element (r, w) at r*W + w: thread t takes the pairs 2t + 1024 u'
    // (u' < 8), i.e. rows r = 128 u' + (t >> 2) = 256 s1 + 16 s2 + r2 with s1 = u' >> 1,
    // s2 = 8 (u' & 1) + (t >> 6), r2 = (t >> 2) & 15, and columns w = 2 (t & 3) + b: v[(2h + b)*4
    // + s1], h = u' & 1, so that each group of four shares (s2, r2, w) like the natural mapping
    const gl_u64x2* blk = (const gl_u64x2*)(in + (uint64_t)kb * a.blk_pitch);  // wave-uniform
    const uint32_t lane_off = (uint32_t)t * 16;
#pragma unroll
    for (int up = 0; up < 8; ++up) {
      const gl_u64x2 e = gl_ld_sv<gl_u64x2>(blk + 512 * up, lane_off);
      v[(2 * (up & 1)) * 4 + (up >> 1)] = e.x;
      v[(2 * (up & 1) + 1) * 4 + (up >> 1)] = e.y;
    }
  } else if constexpr (CS == 1) {
    // in groups of 8 elements like the pass twiddle below: a group's data and factor loads
    // issue together; an element past the coefficients is 0 and loads neither
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      uint64_t tw[8];
#pragma unroll
      for (int uu = 0; uu < 2; ++uu) {
        const int idx = t + NT * (2 * h + uu);
        const int w = idx % W, r2 = (idx / W) % C, s2 = idx / (C * W);
#pragma unroll
        for (int s1 = 0; s1 < 4; ++s1) {
          const uint64_t i = (j0 + w) + (uint64_t)(16 * C * s1 + C * s2 + r2) * stride;
          const bool on = i < a.cs_len;
          v[8 * h + uu * 4 + s1] = on ? in[i] : 0;
          tw[uu * 4 + s1] = on ? gl_cs_factor(a, i) : 0;
        }
      }
#pragma unroll
      for (int m = 0; m < 8; ++m) v[8 * h + m] = G::mul(v[8 * h + m], tw[m], f);
    }
  } else if constexpr (SP == 2) {
    // the natural mapping below with n = R^2 (rows R long): row r = 16 C s1 + NT / W u + t / W,
    // so the lane's part (t / W, t % W) is one offset and (s1, u) a wave-uniform stride
    static_assert(NT / W == 4 * C && 4 * (NT / W) == 16 * C, "rows of one load: 16 C s1 + 4 C u + t / W");
    const uint64_t* row0 = in + j0;
    const uint32_t lane_off = ((uint32_t)(t / W) << LOGR | (uint32_t)(t % W)) * 8;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int s1 = 0; s1 < 4; ++s1)
        v[u * 4 + s1] = gl_ld_sv<uint64_t>(row0 + ((uint64_t)(16 * C * s1 + (NT / W) * u) << LOGR), lane_off);
    }
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = t + NT * u;
      const int w = idx % W, r2 = (idx / W) % C, s2 = idx / (C * W);
#pragma unroll
      for (int s1 = 0; s1 < 4; ++s1) {
        const int r = 16 * C * s1 + C * s2 + r2;
        v[u * 4 + s1] = in[(j0 + w) + (uint64_t)r * stride];
      }
    }
  }
  // RG 3: the stage-B general twiddle w^(a0 X) (a0 = r2 + 4 s2, X = 65536 q1 + j), geometric in
  // s2: C[r2][X] D[X]^s2 with C = w^(r2 X), D = w^(4 X) (tws_a, tws_b); C and D are loaded now
  // (in flight during stage A) in the stage-B thread mapping, the powers formed in stage B
  uint64_t t3[RG == 3 ? 2 : 1];
  if constexpr (RG == 3) {
    const int wave = t >> 6, q1 = wave / Sh::WPQ, rw = (wave % Sh::WPQ) * 64 + (t & 63);
    const int r2 = rw / W, w = rw % W;
    const uint64_t X = ((uint64_t)q1 << 16) + j0 + w;
    t3[0] = a.tws_a[((uint64_t)r2 << 18) + X];
    t3[1] = a.tws_b[X];
  }
  if constexpr (!FIRST && RG != 3 && SP == 0) if (!a.skip_pass_tw) {
    const uint64_t kmask = (1ull << a.log_ns) - 1;
    // in groups of 8 elements (loads of a group issue back to back; bounded live registers)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      uint64_t tw[8];
#pragma unroll
      for (int uu = 0; uu < 2; ++uu) {
        const int u = 2 * h + uu;
        const int idx = t + NT * u;
        const int w = idx % W, r2 = (idx / W) % C, s2 = idx / (C * W);
        const uint64_t k = (j0 + w) & kmask;
#pragma unroll
        for (int s1 = 0; s1 < 4; ++s1) {
          const uint64_t r = (uint64_t)(16 * C * s1 + C * s2 + r2);
          if (a.twpass) {
            tw[uu * 4 + s1] = a.twpass[(r << a.log_ns) + k];
          } else if (a.tws_a) {  // last pass: k = kb*W + w
            tw[uu * 4 + s1] = G::mul(a.tws_b[(uint64_t)kb * Sh::R + r], a.tws_a[r * W + w], f);
          } else {
            const uint64_t e = ((r * k) << (a.log_n - a.log_ns - LOGR)) & (a.n - 1);
            tw[uu * 4 + s1] = G::mul(a.tw0[e & ((1ull << a.tw_bits) - 1)], a.tw1[e >> a.tw_bits], f);
          }
        }
      }
#pragma unroll
      for (int m = 0; m < 8; ++m) v[8 * h + m] = G::mul(v[8 * h + m], tw[m], f);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) dft_reg<G, 2, sub_root_exp(E64, 2)>(v + u * 4, nullptr, f);
  if constexpr (SPLIT) {
    // Z in two rounds, low words (hw = 0) then high words: write, barrier, read in stage B's
    // mapping (below), and a barrier before the high words overwrite the low ones. The outgoing
    // words of a round are dead before its incoming words arrive.
    const int q1r = (t >> 6) / Sh::WPQ, rwr = ((t >> 6) % Sh::WPQ) * 64 + (t & 63);
    uint32_t zl[16];
#pragma unroll
    for (int hw = 0; hw < 2; ++hw) {
      if (hw) __syncthreads();
      if constexpr (BLK_IN) {
        // rw = r2*W + w = 2 (t & 63) + b: the two columns of a pair are neighbours in Z
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int s2 = 8 * h + (t >> 6);
#pragma unroll
          for (int q1 = 0; q1 < 4; ++q1) {
            gl_u32x2 e;
            e.x = (uint32_t)(v[(2 * h) * 4 + bitrev_c(q1, 2)] >> (32 * hw));
            e.y = (uint32_t)(v[(2 * h + 1) * 4 + bitrev_c(q1, 2)] >> (32 * hw));
            *(gl_u32x2*)(lds32 + (q1 * 16 + s2) * (C * W) + 2 * (t & 63)) = e;
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int idx = t + NT * u;  // = s2*(C*W) + (r2*W + w)
          const int s2 = idx / (C * W), rw = idx % (C * W);
#pragma unroll
          for (int q1 = 0; q1 < 4; ++q1)
            lds32[(q1 * 16 + s2) * (C * W) + rw] = (uint32_t)(v[u * 4 + bitrev_c(q1, 2)] >> (32 * hw));
        }
      }
      __syncthreads();
      static_assert(C * W * 4 == 512, "Z stride of gl_lds_read16");
      if (hw == 0) {
        gl_lds_read16<512>(lds32 + q1r * 16 * (C * W) + rwr, zl);
      } else {
        uint32_t zh[16];
        gl_lds_read16<512>(lds32 + q1r * 16 * (C * W) + rwr, zh);
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) v[s2] = ((uint64_t)zh[s2] << 32) | zl[s2];
      }
    }
  } else if constexpr (BLK_IN) {
    // rw = r2*W + w = 2 (t & 63) + b: the two columns of a pair are neighbours in Z
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int s2 = 8 * h + (t >> 6);
#pragma unroll
      for (int q1 = 0; q1 < 4; ++q1) {
        gl_u64x2 e;
        e.x = v[(2 * h) * 4 + bitrev_c(q1, 2)];
        e.y = v[(2 * h + 1) * 4 + bitrev_c(q1, 2)];
        *(gl_u64x2*)(lds + (q1 * 16 + s2) * (C * W) + 2 * (t & 63)) = e;
      }
    }
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = t + NT * u;  // = s2*(C*W) + (r2*W + w)
      const int s2 = idx / (C * W), rw = idx % (C * W);
#pragma unroll
      for (int q1 = 0; q1 < 4; ++q1) lds[(q1 * 16 + s2) * (C * W) + rw] = v[u * 4 + bitrev_c(q1, 2)];
    }
  }
  if constexpr (!SPLIT) __syncthreads();

  // ---------------- stage B: one q1 per wave; shift twiddles; 16-point DFT over s2
  // SPLIT: the thread id of everything after stage B's arithmetic, opaque to the compiler there,
  // so that no address of the Y exchange or the stores is computed early and held across stage B
  int tc = t;
  // SPLIT: the 32-bit half hw of stage B's outputs q2 to Y (r2, k1 = q1 + 4 q2, w). W = 8 and
  // ysw(k1) = q2 & 7: 8 XOR variants of one base, q2 and q2 + 8 an immediate apart
  auto y_write_half = [&](int hw) {
    const int wv = tc >> 6, q1 = wv / Sh::WPQ, rw = (wv % Sh::WPQ) * 64 + (tc & 63);
    const int r2 = rw / W, w = rw % W;
    static_assert(!SPLIT || (W == 8 && Sh::yidx(3, 2 + 4 * 13, 6) == 3 * YP + 2 * W + (6 ^ (13 & 7)) + 4 * W * 13), "Y address form");
#pragma unroll
    for (int q2 = 0; q2 < 16; ++q2)
      lds32[(r2 * YP + q1 * W + (w ^ (q2 & 7))) + 4 * W * q2] = (uint32_t)(v[bitrev_c(q2, 4)] >> (32 * hw));
  };
  {
    const int wave = t >> 6;
    const int q1 = wave / Sh::WPQ;
    const int rw = (wave % Sh::WPQ) * 64 + (t & 63);  // r2*W + w
    if constexpr (!SPLIT) {
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) v[s2] = lds[(q1 * 16 + s2) * (C * W) + rw];
    }
    if constexpr (RG == 3) {
      uint64_t p = t3[0];
      const uint64_t d = t3[1];
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        v[s2] = G::mul(v[s2], p, f);
        if (s2 < 15) p = G::mul(p, d, f);
      }
      dft_reg<G, 4, sub_root_exp(E64, 4)>(v, nullptr, f);
    } else {
      // the twiddle's signs are folded into the DFT's first levels, whose butterflies then
      // differ by q1
      switch (__builtin_amdgcn_readfirstlane(q1)) {
        case 1: gl_stage_b_head<E64, 1>(v); break;
        case 2: gl_stage_b_head<E64, 2>(v); break;
        case 3: gl_stage_b_head<E64, 3>(v); break;
        default: gl_stage_b_head<E64, 0>(v); break;
      }
      dft_reg_tail<G, 4, sub_root_exp(E64, 4), GL_B_LEVELS>(v, f);
    }
    if constexpr (SPLIT) {
      asm volatile("" : "+v"(tc));
      __builtin_assume(tc >= 0 && tc < NT);
    }
    __syncthreads();  // every thread has read Z (SPLIT: its high words)
    if constexpr (SPLIT) {
      y_write_half(0);
    } else {
      const int r2 = rw / W, w = rw % W;
#pragma unroll
      for (int q2 = 0; q2 < 16; ++q2) {
        const int k1 = q1 + 4 * q2;
        lds[Sh::yidx(r2, k1, w)] = v[bitrev_c(q2, 4)];
      }
    }
  }
  __syncthreads();

  // ---------------- stage C: table twiddle w_R^(r2*k1); C-point DFT over r2
  // sub-DFT (k1, w) of thread t: FIRST pass all 64 k1 of one column per wave (512-B runs
  // of k in the output rows out[j*R + k]); later passes w fastest (W-element runs of j);
  // tile-major stores: 8 digits k1 = 8 wave + (lane & 7) of all 8 columns per wave (the 64
  // elements [j][k & 7] of this tile in block (k >> 3) = wave + 8 k2; the Y reads are a
  // permutation of the 512-B span of those 8 k1: w ^ ysw(k1) runs over all 8 columns)
  auto c_map = [&](int u, int* k1, int* w) {
    const int idx = t + NT * u;
    if constexpr (BLK_OUT) {
      *k1 = 8 * (tc >> 6) + (tc & 7);
      *w = (tc >> 3) & 7;
    } else if constexpr (FIRST) {
      *k1 = idx & 63;
      *w = idx >> 6;
    } else if constexpr (SPLIT) {
      *k1 = tc / W;  // NSUB_C = 1
      *w = tc % W;
    } else {
      *k1 = idx / W;
      *w = idx % W;
    }
  };
  uint64_t x[Sh::NSUB_C * C];
#pragma unroll
  for (int u = 0; u < Sh::NSUB_C; ++u) {
    int k1, w;
    c_map(u, &k1, &w);
    if constexpr (SPLIT) {
      // Y in two rounds like Z: the low words are read, then the high words take their place
      static_assert(Sh::NSUB_C == 1, "split exchange: one sub-DFT per thread");
      static_assert(C == 16 && YP * 4 == 2080, "Y stride of gl_lds_read16");
      uint32_t yl[C], yh[C];
      gl_lds_read16<2080>(lds32 + Sh::yidx(0, k1, w), yl);
      __syncthreads();
      y_write_half(1);
      __syncthreads();
      gl_lds_read16<2080>(lds32 + Sh::yidx(0, k1, w), yh);
#pragma unroll
      for (int r2 = 0; r2 < C; ++r2) x[r2] = ((uint64_t)yh[r2] << 32) | yl[r2];
    } else {
#pragma unroll
      for (int r2 = 0; r2 < C; ++r2) x[u * C + r2] = lds[Sh::yidx(r2, k1, w)];
    }
  }
  if constexpr (RG == 3) {
    // w_64^(r2 g), g = k1 >> 2 = wave + 4 u (4-wave tiles, W = 16): wave-uniform shifts
    switch (__builtin_amdgcn_readfirstlane(t >> 6)) {
      case 0: gl_rg3_c_shift<E64, 0>(x); break;
      case 1: gl_rg3_c_shift<E64, 1>(x); break;
      case 2: gl_rg3_c_shift<E64, 2>(x); break;
      default: gl_rg3_c_shift<E64, 3>(x); break;
    }
  } else if constexpr (RG == 1) {
    // tc[a2l][r2][k1] = w_4096^((a2l + 16 r2) k1), a2l = bits 12..15 of the column: every row
    const uint64_t* tc = a.tc + ((j0 >> 12) & 15) * 256;
#pragma unroll
    for (int u = 0; u < Sh::NSUB_C; ++u) {
      int k1, w;
      c_map(u, &k1, &w);
      uint64_t tw[C];
#pragma unroll
      for (int r2 = 0; r2 < C; ++r2) tw[r2] = tc[r2 * 64 + k1];
#pragma unroll
      for (int r2 = 0; r2 < C; ++r2) x[u * C + r2] = G::mul(x[u * C + r2], tw[r2], f);
    }
  } else {
    uint64_t tw[Sh::NSUB_C * C];
    const bool scaled = SP == 0 && a.scaled;
    const int r2lo = scaled ? 0 : 1;  // scaled table carries n^-1: every element multiplies
#pragma unroll
    for (int u = 0; u < Sh::NSUB_C; ++u) {
      int k1, w;
      c_map(u, &k1, &w);
#pragma unroll
      for (int r2 = 0; r2 < C; ++r2) tw[u * C + r2] = (r2 >= r2lo) ? a.tc[r2 * 64 + k1] : 1;
    }
    if (scaled) {
#pragma unroll
      for (int m = 0; m < Sh::NSUB_C * C; ++m) x[m] = G::mul(x[m], tw[m], f);
    } else {
      // r2 = 0 rows multiply by 1 and are skipped; k1 = 0 lanes multiply by 1 (a per-lane
      // branch would only diverge)
#pragma unroll
      for (int u = 0; u < Sh::NSUB_C; ++u)
#pragma unroll
        for (int r2 = 1; r2 < C; ++r2) x[u * C + r2] = G::mul(x[u * C + r2], tw[u * C + r2], f);
    }
  }
  if constexpr (C > 1) {
#pragma unroll
    for (int u = 0; u < Sh::NSUB_C; ++u) dft_reg<G, LOGC, sub_root_exp(E64, LOGC)>(x + u * C, nullptr, f);
  }

  // ---------------- store
  if constexpr (BLK_OUT) {
    // element and post_tw entry (block wave + 8 k2, [j0 + w][k1 & 7]): a wave-uniform base plus
    // the lane
    static_assert(Sh::NSUB_C == 1 && W == 8, "tile-major stores: one sub-DFT per thread");
    const uint64_t base = (uint64_t)__builtin_amdgcn_readfirstlane(tc >> 6) * a.blk_pitch + j0 * W;
    const uint32_t lane_off = (tc & 63) * 8;
    const uint64_t* ptw = a.post_tw + base;
    uint64_t* o = a.out + (uint64_t)poly * a.out_pitch + base;
    uint64_t tw[C];
#pragma unroll
    for (int k2 = 0; k2 < C; ++k2) tw[k2] = gl_ld_sv<uint64_t>(ptw + (uint64_t)(8 * k2) * a.blk_pitch, lane_off);
#pragma unroll
    for (int k2 = 0; k2 < C; ++k2) x[bitrev_c(k2, LOGC)] = G::mul(x[bitrev_c(k2, LOGC)], tw[k2], f);
#pragma unroll
    for (int k2 = 0; k2 < C; ++k2) gl_st_sv<uint64_t>(o + (uint64_t)(8 * k2) * a.blk_pitch, lane_off, x[bitrev_c(k2, LOGC)]);
  } else if constexpr (FIRST) {
    uint64_t* o = a.out + (uint64_t)poly * a.out_pitch;
#pragma unroll
    for (int u = 0; u < Sh::NSUB_C; ++u) {
      int k1, w;
      c_map(u, &k1, &w);
      const uint64_t base = (j0 + w) << LOGR;
      if (a.post_tw) {
        uint64_t tw[C];
#pragma unroll
        for (int k2 = 0; k2 < C; ++k2) tw[k2] = a.post_tw[base + k1 + 64 * k2];
#pragma unroll
        for (int k2 = 0; k2 < C; ++k2) x[u * C + bitrev_c(k2, LOGC)] = G::mul(x[u * C + bitrev_c(k2, LOGC)], tw[k2], f);
      }
#pragma unroll
      for (int k2 = 0; k2 < C; ++k2) o[base + k1 + 64 * k2] = x[u * C + bitrev_c(k2, LOGC)];
    }
  } else if constexpr (SP == 2) {
    // the natural-order store below with log_ns = LOGR and the tile's W columns inside one run
    // (j0 a multiple of W): out[(j0 >> LOGR << 2 LOGR) + (j0 mod R) + w + (k1 + 64 k2 << LOGR)],
    // (k1, w) the lane's offset, j0 and k2 wave-uniform
    static_assert(Sh::NSUB_C == 1 && (1 << LOGR) % W == 0, "one sub-DFT per thread, whole runs");
    uint64_t* o = a.out + (uint64_t)poly * a.out_pitch + ((j0 >> LOGR) << (2 * LOGR)) + (j0 & ((1u << LOGR) - 1));
    const uint32_t lane_off = ((uint32_t)(tc / W) << LOGR | (uint32_t)(tc % W)) * 8;
#pragma unroll
    for (int k2 = 0; k2 < C; ++k2) gl_st_sv<uint64_t>(o + ((uint64_t)(64 * k2) << LOGR), lane_off, x[bitrev_c(k2, LOGC)]);
  } else {
    const uint32_t lns = a.log_ns;
    const uint64_t ns_mask = (1ull << lns) - 1;
    uint64_t* out = a.out + (uint64_t)poly * a.out_pitch;
    const uint32_t sl = SP != 0 ? 0u : a.out_split_log;
#pragma unroll
    for (int u = 0; u < Sh::NSUB_C; ++u) {
      int k1, w;
      c_map(u, &k1, &w);
      const uint64_t j = j0 + w;
      const uint64_t base = ((j >> lns) << (lns + LOGR)) + (j & ns_mask);
      if (sl == 0) {
        if constexpr (CS == 2) {
          uint64_t tw[C];
#pragma unroll
          for (int k2 = 0; k2 < C; ++k2) tw[k2] = gl_cs_factor(a, base + ((uint64_t)(k1 + 64 * k2) << lns));
#pragma unroll
          for (int k2 = 0; k2 < C; ++k2) x[u * C + bitrev_c(k2, LOGC)] = G::mul(x[u * C + bitrev_c(k2, LOGC)], tw[k2], f);
        }
#pragma unroll
        for (int k2 = 0; k2 < C; ++k2) out[base + ((uint64_t)(k1 + 64 * k2) << lns)] = x[u * C + bitrev_c(k2, LOGC)];
      } else {
        const uint64_t smask = (1ull << sl) - 1;
#pragma unroll
        for (int k2 = 0; k2 < C; ++k2) {
          const uint64_t kk = base + ((uint64_t)(k1 + 64 * k2) << lns);
          a.out[((((kk >> sl) * a.batch) + poly) << sl) + (kk & smask)] = x[u * C + bitrev_c(k2, LOGC)];
        }
      }
    }
  }
}

template <int LOGR, int TILE>
__device__ __forceinline__ void gl_shape_checks() {
  using Sh = GlShape<LOGR, TILE>;
  static_assert(LOGR >= 6 && LOGR <= 10, "radix 2^6 .. 2^10");
  static_assert(Sh::LDS * 8 <= (TILE > 8192 ? 160 : 80) * 1024, "LDS budget");
  static_assert(Sh::W >= 8 && Sh::WPQ >= 1, "tile shape");
}

// One tile per workgroup.
template <int LOGR, int E64, bool FIRST, int TILE, int RG = 0, int CS = 0, int SP = 0>
// waves per SIMD the VGPR budget allows: 5 where the LDS allows five workgroups and the
// kernel fits 96 VGPRs without spilling (first passes and the regrouped plan's), else 4; six
// for the split exchange of SP 2 (three workgroups of 8 waves per CU, 80 VGPRs)
__global__ void __launch_bounds__(TILE / 16)
__attribute__((amdgpu_waves_per_eu(gl_split(SP) ? 6 : (FIRST || RG) && GlShape<LOGR, TILE>::LDS32K ? 5 : 4)))
ntt_gl_pass_kernel(GlPassArgs a) {
  gl_shape_checks<LOGR, TILE>();
  constexpr int LDS64 = GlShape<LOGR, TILE>::LDS / (gl_split(SP) ? 2 : 1);  // 8-B units
  static_assert(!gl_split(SP) || 3 * LDS64 * 8 <= 160 * 1024, "split exchange: three workgroups per CU");
  __shared__ __attribute__((aligned(16))) uint64_t lds[LDS64];
  const uint32_t tiles = a.blocks_per_poly * a.batch;
  gl_tile<LOGR, E64, FIRST, TILE, RG, CS, SP>(a, lds, blockIdx.x, tiles, threadIdx.x);
}

// ---- regrouped 2^24 plan (DESIGN.md §3.1 "Regrouped twiddles") --------------------------
// The three radix-2^8 passes of a 2^24 transform re-cut so that every general (table)
// twiddle sits between DFT blocks of 64 points: with the index bits in four groups of six,
// j = a0 + 64 a1 + 4096 a2 + 2^18 a3 and k = b0 + 64 b1 + 4096 b2 + 2^18 b3, decimation in
// frequency needs only the three twiddle layers w^(4096 a2 b0), w^(64 a1 (b0 + 64 b1)) and
// w^(a0 (b0 + 64 b1 + 4096 b2)); each 64-point group DFT that straddles two passes is split
// 4 x 16 or 16 x 4 with a w_64 (shift) twiddle between its halves. Per element that is 3
// general multiplications for the whole transform instead of 4.25 (0.75 + 1.75 + 1.75):
//   pass 1 (RG 1): DFT-64 over a3 | w_4096^(a2 b0) (a2l = bits 12..15 of the column) | DFT-4
//   pass 2 (this kernel): w_64^(a2l c) | DFT-16 over a2l | T2[a1][K] | DFT-16 over a1h | w_64^(a1l e)
//   pass 3 (RG 3): DFT-4 over a1l | w^(a0 X) = C[r2][X] D[X]^s2 | DFT-16 | w_64^(r2 g) | DFT-4
// Pass 2 needs one LDS exchange (two 16-point stages), not two. Data stays in the Stockham
// layout of the other passes (natural order in and out).
// Pass 2 tile: 256 rows r = 16 a2l + a1h x W = 16 columns j (Ns = 256: j mod 256 = b0 + 64 c,
// the first pass's output digit; bits 14..15 of j = a1l); stage X thread (a1h, w), stage Y
// thread (d, w); LDS [d][a1h ^ (d mod 4)][w] (the XOR spreads the stage-Y reads of four d per
// wave over both halves of the banks: every bank pair is hit exactly twice, the minimum).
template <int E64>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) ntt_gl_rg2_kernel(GlPassArgs a) {
  constexpr int W = 16;
  // 32 KiB; four waves per SIMD: at five the 96-VGPR budget spills 28 B per lane and the pass
  // runs ~2 % slower (profiles/r03/ntt_lds_ab.log)
  __shared__ __attribute__((aligned(16))) uint64_t lds[16 * 16 * W];
  const FieldArgs f{};
  using G = Goldilocks;
  const uint32_t tiles = a.blocks_per_poly * a.batch;
  uint32_t poly, kb;
  gl_tile_coords(a, blockIdx.x, tiles, &poly, &kb);
  const int t = threadIdx.x, w = t % W, a1h = t / W;
  const uint64_t j0 = (uint64_t)kb * W, j = j0 + w;
  const uint32_t c = (uint32_t)(j0 >> 6) & 3, a1l = (uint32_t)(j0 >> 14) & 3;
  const uint64_t* in = a.in + (uint64_t)poly * a.in_pitch;
  const uint64_t stride = a.n >> 8;
  uint64_t v[16], tw[16];
#pragma unroll
  for (int a2l = 0; a2l < 16; ++a2l) v[a2l] = in[j + (uint64_t)(a2l * 16 + a1h) * stride];
  // T2[a1][K] = w^(64 a1 K), a1 = a1l + 4 a1h, K = b0 + 64 b1 = (j mod 256) + 256 d (2 MiB,
  // L2-resident; the geometric form T2[a1][j mod 256] (w^(16384 a1))^d measured 1.5 % slower in
  // round 5, profiles/r05/t2geo_ab.log)
  const uint64_t* t2 = a.twpass + ((uint64_t)(a1l + 4 * a1h) << 12) + (j & 255);
#pragma unroll
  for (int d = 0; d < 16; ++d) tw[d] = t2[256 * d];
  switch (__builtin_amdgcn_readfirstlane(c)) {  // w_64^(a2l c)
    case 1: gl_stage_b_twiddle<E64, 1>(v); break;
    case 2: gl_stage_b_twiddle<E64, 2>(v); break;
    case 3: gl_stage_b_twiddle<E64, 3>(v); break;
    default: break;
  }
  dft_reg<G, 4, sub_root_exp(E64, 4)>(v, nullptr, f);  // output d at v[bitrev4(d)]
#pragma unroll
  for (int d = 0; d < 16; ++d) lds[d * 256 + (a1h ^ (d & 3)) * W + w] = G::mul(v[bitrev_c(d, 4)], tw[d], f);
  __syncthreads();
  const int d2 = t / W;
#pragma unroll
  for (int h = 0; h < 16; ++h) v[h] = lds[d2 * 256 + (h ^ (d2 & 3)) * W + w];
  dft_reg<G, 4, sub_root_exp(E64, 4)>(v, nullptr, f);  // output e at v[bitrev4(e)]
  switch (__builtin_amdgcn_readfirstlane(a1l)) {  // w_64^(a1l e)
    case 1: gl_post_twiddle_br<E64, 1>(v); break;
    case 2: gl_post_twiddle_br<E64, 2>(v); break;
    case 3: gl_post_twiddle_br<E64, 3>(v); break;
    default: break;
  }
  // output digit k = d + 16 e of the Stockham pass (Ns = 256)
  uint64_t* out = a.out + (uint64_t)poly * a.out_pitch;
  const uint64_t base = ((j >> 8) << 16) + (j & 255);
#pragma unroll
  for (int e = 0; e < 16; ++e) out[base + ((uint64_t)(d2 + 16 * e) << 8)] = v[bitrev_c(e, 4)];
}

}  // namespace pbf
