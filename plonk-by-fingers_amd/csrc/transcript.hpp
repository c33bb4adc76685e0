// The Fiat-Shamir transcript of the PLONK entry points (include/pbf.h "Fiat-Shamir", DESIGN.md
// §3.17): Keccak-256 (Ethereum's variant: rate 136 bytes, padding 0x01 .. 0x80) over messages that
// are whole 8-byte lanes. One __host__ __device__ Keccak-f[1600] and one statement of every
// message serve the host paths (single prover and verifier, circuit digest) and the kernels of
// transcript.hip alike.
//
// Lanes: a Keccak lane is the little-endian load of 8 message bytes. Every transcript item is
// big-endian, so u64(k) is the lane bswap(k), be32(x) of the limbs x[0..3] is the four lanes
// bswap(x[3]), bswap(x[2]), bswap(x[1]), bswap(x[0]), and a digest is four lanes as they leave the
// state. The state and every message are indexed by constants only (loops of constant trip count,
// unrolled), so on the device they live in registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <vector>

struct pbf_ctx;

namespace pbf {

constexpr int KECCAK_RATE_LANES = 17;  // 136 bytes
// transcript tags (the u64 after the previous digest; 7, 8: tree digests of pub and of the t6)
constexpr uint64_t FS_TAG_PUB = 7, FS_TAG_BATCH = 8, FS_TAG_RHO = 9;

__host__ __device__ __forceinline__ uint64_t fs_bswap(uint64_t v) { return __builtin_bswap64(v); }
template <int N>
__host__ __device__ __forceinline__ uint64_t keccak_rotl(uint64_t v) {
  if constexpr (N == 0) return v;
  else return (v << N) | (v >> (64 - N));
}

// one round, every index and rotation a constant
__host__ __device__ __forceinline__ void keccak_round(uint64_t (&a)[25], uint64_t rc) {
  uint64_t c[5], d[5], b[25];
#pragma unroll
  for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
  for (int x = 0; x < 5; ++x) d[x] = c[(x + 4) % 5] ^ keccak_rotl<1>(c[(x + 1) % 5]);
#pragma unroll
  for (int i = 0; i < 25; ++i) a[i] ^= d[i % 5];
  // rho and pi: b[y + 5 ((2x + 3y) mod 5)] = rotl(a[x + 5y], r[x][y])
  b[0] = a[0];
  b[10] = keccak_rotl<1>(a[1]);
  b[20] = keccak_rotl<62>(a[2]);
  b[5] = keccak_rotl<28>(a[3]);
  b[15] = keccak_rotl<27>(a[4]);
  b[16] = keccak_rotl<36>(a[5]);
  b[1] = keccak_rotl<44>(a[6]);
  b[11] = keccak_rotl<6>(a[7]);
  b[21] = keccak_rotl<55>(a[8]);
  b[6] = keccak_rotl<20>(a[9]);
  b[7] = keccak_rotl<3>(a[10]);
  b[17] = keccak_rotl<10>(a[11]);
  b[2] = keccak_rotl<43>(a[12]);
  b[12] = keccak_rotl<25>(a[13]);
  b[22] = keccak_rotl<39>(a[14]);
  b[23] = keccak_rotl<41>(a[15]);
  b[8] = keccak_rotl<45>(a[16]);
  b[18] = keccak_rotl<15>(a[17]);
  b[3] = keccak_rotl<21>(a[18]);
  b[13] = keccak_rotl<8>(a[19]);
  b[14] = keccak_rotl<18>(a[20]);
  b[24] = keccak_rotl<2>(a[21]);
  b[9] = keccak_rotl<61>(a[22]);
  b[19] = keccak_rotl<56>(a[23]);
  b[4] = keccak_rotl<14>(a[24]);
#pragma unroll
  for (int y = 0; y < 25; y += 5)
#pragma unroll
    for (int x = 0; x < 5; ++x) a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & b[y + (x + 2) % 5]);
  a[0] ^= rc;
}

// Keccak-f[1600]: 24 rounds, unrolled
__host__ __device__ inline void keccak_f1600(uint64_t (&a)[25]) {
  keccak_round(a, 0x0000000000000001ull);
  keccak_round(a, 0x0000000000008082ull);
  keccak_round(a, 0x800000000000808Aull);
  keccak_round(a, 0x8000000080008000ull);
  keccak_round(a, 0x000000000000808Bull);
  keccak_round(a, 0x0000000080000001ull);
  keccak_round(a, 0x8000000080008081ull);
  keccak_round(a, 0x8000000000008009ull);
  keccak_round(a, 0x000000000000008Aull);
  keccak_round(a, 0x0000000000000088ull);
  keccak_round(a, 0x0000000080008009ull);
  keccak_round(a, 0x000000008000000Aull);
  keccak_round(a, 0x000000008000808Bull);
  keccak_round(a, 0x800000000000008Bull);
  keccak_round(a, 0x8000000000008089ull);
  keccak_round(a, 0x8000000000008003ull);
  keccak_round(a, 0x8000000000008002ull);
  keccak_round(a, 0x8000000000000080ull);
  keccak_round(a, 0x000000000000800Aull);
  keccak_round(a, 0x800000008000000Aull);
  keccak_round(a, 0x8000000080008081ull);
  keccak_round(a, 0x8000000000008080ull);
  keccak_round(a, 0x0000000080000001ull);
  keccak_round(a, 0x8000000080008008ull);
}

// Keccak-256 of a message of K whole lanes (K a constant: every state index is one)
template <int K>
__host__ __device__ __forceinline__ void keccak256_lanes(const uint64_t (&m)[K], uint64_t out[4]) {
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) a[i] = 0;
#pragma unroll
  for (int blk = 0; blk < K / KECCAK_RATE_LANES; ++blk) {
#pragma unroll
    for (int i = 0; i < KECCAK_RATE_LANES; ++i) a[i] ^= m[KECCAK_RATE_LANES * blk + i];
    keccak_f1600(a);
  }
#pragma unroll
  for (int i = 0; i < K % KECCAK_RATE_LANES; ++i) a[i] ^= m[K - K % KECCAK_RATE_LANES + i];
  a[K % KECCAK_RATE_LANES] ^= 0x01;
  a[KECCAK_RATE_LANES - 1] ^= 0x8000000000000000ull;
  keccak_f1600(a);
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = a[i];
}

// Keccak-256 of len bytes (any len; the lanes of the last block are put together byte by byte)
__host__ __device__ inline void keccak256_bytes(const uint8_t* msg, uint64_t len, uint64_t out[4]) {
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) a[i] = 0;
  const bool aligned = ((uintptr_t)msg & 7) == 0;
  uint64_t off = 0;
  for (; off + 8 * KECCAK_RATE_LANES <= len; off += 8 * KECCAK_RATE_LANES) {
#pragma unroll
    for (int i = 0; i < KECCAK_RATE_LANES; ++i) {
      const uint8_t* p = msg + off + 8 * i;
      uint64_t v = 0;
      if (aligned) {
        __builtin_memcpy(&v, p, 8);  // one 8-byte load
      } else {
        for (int k = 0; k < 8; ++k) v |= (uint64_t)p[k] << (8 * k);
      }
      a[i] ^= v;
    }
    keccak_f1600(a);
  }
  const uint32_t rem = (uint32_t)(len - off);  // < 136: the message's tail, then the padding
#pragma unroll
  for (int i = 0; i < KECCAK_RATE_LANES; ++i) {
    uint64_t v = 0;
    for (uint32_t k = 0; k < 8; ++k)
      if (8 * i + k < rem) v |= (uint64_t)msg[off + 8 * i + k] << (8 * k);
    if ((uint32_t)i == rem / 8) v ^= (uint64_t)0x01 << (8 * (rem % 8));
    a[i] ^= v;
  }
  a[KECCAK_RATE_LANES - 1] ^= 0x8000000000000000ull;
  keccak_f1600(a);
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = a[i];
}

// ---------------------------------------------------------------- items
// be32 of 4 little-endian limbs, as 4 lanes
__host__ __device__ __forceinline__ void fs_be32(uint64_t* lanes, const uint64_t* limbs) {
#pragma unroll
  for (int k = 0; k < 4; ++k) lanes[k] = fs_bswap(limbs[3 - k]);
}
// pt(P) of an affine point (x, y as 4 + 4 limbs), as 8 lanes
__host__ __device__ __forceinline__ void fs_pt(uint64_t* lanes, const uint64_t* p) {
  fs_be32(lanes, p);
  fs_be32(lanes + 4, p + 4);
}
// int(digest) mod r as 4 little-endian limbs: the digest is below 2^256 < 6 r
__host__ __device__ inline void fs_challenge(const uint64_t dg[4], uint64_t* limbs) {
  const uint64_t R[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
  uint64_t v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = fs_bswap(dg[3 - k]);
#pragma unroll
  for (int it = 0; it < 5; ++it) {
    uint64_t d[4], borrow = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t t = v[k] - R[k];
      const uint64_t b1 = v[k] < R[k];
      d[k] = t - borrow;
      borrow = b1 | (t < borrow);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = borrow ? v[k] : d[k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) limbs[k] = v[k];
}

// one node of a tree digest: H of k = 1..4 items of 4 lanes (at most 128 bytes: one permutation).
// LIMBS: the items are field elements as limbs (the tree's first level over pub), hashed as be32.
template <bool LIMBS>
__host__ __device__ __forceinline__ void fs_tree_node(const uint64_t* items, uint32_t k, uint64_t out[4]) {
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) a[i] = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if ((uint32_t)j < k) {
#pragma unroll
      for (int l = 0; l < 4; ++l) a[4 * j + l] = LIMBS ? fs_bswap(items[4 * j + 3 - l]) : items[4 * j + l];
    }
#pragma unroll
  for (int j = 1; j <= 4; ++j)
    if (k == (uint32_t)j) a[4 * j] ^= 0x01;
  a[KECCAK_RATE_LANES - 1] ^= 0x8000000000000000ull;
  keccak_f1600(a);
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = a[i];
}
// the last hash of a tree digest: H(u64(tag) | u64(m) | root)
__host__ __device__ __forceinline__ void fs_tree_close(uint64_t tag, uint64_t m, const uint64_t root[4], uint64_t out[4]) {
  const uint64_t msg[6] = {fs_bswap(tag), fs_bswap(m), root[0], root[1], root[2], root[3]};
  keccak256_lanes(msg, out);
}

// ---------------------------------------------------------------- the rounds of one proof
// prev | u64(tag) | NP points | NF fields -> the round's digest. pts: NP x 8 limbs, f: NF x 4 limbs
template <int NP, int NF>
__host__ __device__ __forceinline__ void fs_round(const uint64_t prev[4], uint64_t tag, const uint64_t* pts,
                                                 const uint64_t* f, uint64_t out[4]) {
  uint64_t m[5 + 8 * NP + 4 * NF];
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = prev[i];
  m[4] = fs_bswap(tag);
#pragma unroll
  for (int p = 0; p < NP; ++p) fs_pt(m + 5 + 8 * p, pts + 8 * p);
#pragma unroll
  for (int k = 0; k < NF; ++k) fs_be32(m + 5 + 8 * NP + 4 * k, f + 4 * k);
  keccak256_lanes(m, out);
}
// t1 = H(h0 | u64(1) | P | pt(a_s) | pt(b_s) | pt(c_s))
__host__ __device__ __forceinline__ void fs_round1(const uint64_t h0[4], const uint64_t P[4], const uint64_t* abc_s,
                                                  uint64_t out[4]) {
  uint64_t m[9 + 24];
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = h0[i], m[5 + i] = P[i];
  m[4] = fs_bswap(1);
#pragma unroll
  for (int p = 0; p < 3; ++p) fs_pt(m + 9 + 8 * p, abc_s + 8 * p);
  keccak256_lanes(m, out);
}

// The whole chain of one proof (pts 9 x 8, f 7 x 4 limbs, as given): chal = alpha beta gamma z v
// (5 x 4 limbs, the order of the entry points), u (4 limbs), t6 (4 lanes)
__host__ __device__ inline void fs_proof_chain(const uint64_t h0[4], const uint64_t P[4], const uint64_t* pts,
                                               const uint64_t* f, uint64_t* chal, uint64_t* u, uint64_t t6[4]) {
  uint64_t t[4], n[4];
  fs_round1(h0, P, pts, t);
  fs_challenge(t, chal + 4);  // beta
  fs_round<0, 0>(t, 2, nullptr, nullptr, n);
  fs_challenge(n, chal + 8);  // gamma
  fs_round<1, 0>(n, 3, pts + 8 * 3, nullptr, t);
  fs_challenge(t, chal);  // alpha
  fs_round<3, 0>(t, 4, pts + 8 * 4, nullptr, n);
  fs_challenge(n, chal + 12);  // z
  fs_round<0, 7>(n, 5, nullptr, f, t);
  fs_challenge(t, chal + 16);  // v
  fs_round<2, 0>(t, 6, pts + 8 * 7, nullptr, t6);
  fs_challenge(t6, u);
}
// rho_i = H(T | u64(9) | u64(i)) mod r, 0 replaced by 1
__host__ __device__ __forceinline__ void fs_rho(const uint64_t T[4], uint64_t i, uint64_t* rho) {
  const uint64_t m[6] = {T[0], T[1], T[2], T[3], fs_bswap(FS_TAG_RHO), fs_bswap(i)};
  uint64_t d[4];
  keccak256_lanes(m, d);
  fs_challenge(d, rho);
  if (!(rho[0] | rho[1] | rho[2] | rho[3])) rho[0] = 1;
}

// ---------------------------------------------------------------- host
// The single-proof paths run these: the root of the tree over m >= 1 items of 4 u64 each (limbs:
// field elements as limbs, the first level hashes them as be32), items overwritten level by level;
// the tree digest of m field elements under tag (m = 0 included); and h0, the circuit digest from
// the verification key (pre: verifier_vk's 8 commitments; g2: [G2, [s]G2], 2 x 16 u64).
inline void fs_tree_root_host(uint64_t* items, uint64_t m, bool limbs, uint64_t root[4]) {
  do {
    const uint64_t mo = (m + 3) / 4;
    for (uint64_t j = 0; j < mo; ++j) {
      const uint32_t k = (uint32_t)(m - 4 * j < 4 ? m - 4 * j : 4);
      uint64_t in[16] = {}, d[4];
      memcpy(in, items + 16 * j, (size_t)k * 32);
      if (limbs) fs_tree_node<true>(in, k, d);
      else fs_tree_node<false>(in, k, d);
      memcpy(items + 4 * j, d, 32);  // node j < 4 j: behind every item still to be read
    }
    m = mo;
    limbs = false;
  } while (m > 1);
  memcpy(root, items, 32);
}

inline void fs_tree_digest_host(uint64_t tag, const uint64_t* limbs, uint64_t m, uint64_t out[4]) {
  uint64_t root[4] = {0, 0, 0, 0};
  if (m) {
    std::vector<uint64_t> w(limbs, limbs + 4 * m);
    fs_tree_root_host(w.data(), m, true, root);
  }
  fs_tree_close(tag, m, root, out);
}

inline void fs_circuit_digest(int mode, uint64_t n, uint64_t npub, const uint64_t* k1k2, const uint64_t (*pre)[8],
                            const uint64_t* g2, uint64_t h0[4]) {
  static const char D[33] = "pbf-plonk-bn254-fiat-shamir-v1\0";  // 30 bytes and two zero bytes
  uint64_t m[4 + 3 + 8 + 64 + 16];
  memcpy(m, D, 32);
  m[4] = fs_bswap((uint64_t)(int64_t)mode), m[5] = fs_bswap(n), m[6] = fs_bswap(npub);
  fs_be32(m + 7, k1k2);
  fs_be32(m + 11, k1k2 + 4);
  for (int k = 0; k < 8; ++k) fs_pt(m + 15 + 8 * k, pre[k]);
  for (int k = 0; k < 4; ++k) fs_be32(m + 79 + 4 * k, g2 + 16 + 4 * k);
  keccak256_lanes(m, h0);
}

// ---------------------------------------------------------------- device (transcript.hip)
// PBF_EINVAL unless every level of the trees over count x npub public inputs and over count digests
// fits one launch: for the entry points' checks, before anything is enqueued
int fs_batch_validate(uint64_t count, uint64_t npub);
// Device runs, enqueued on s, all pointers on the device:
// roots[t] = the tree root over items t m .. t m + m - 1 (4 u64 each; limbs as above), trees x m >= 1.
// Scratch: the context's fs.tree0 / fs.tree1.
int fs_tree_run(pbf_ctx* ctx, const uint64_t* d_items, uint64_t trees, uint64_t m, bool limbs, uint64_t* d_roots,
                hipStream_t s);
// chal (count x 5 x 4), u (count x 4), rho (count x 4, or null) of count proofs under h0 (host, 4
// lanes); d_pub count x npub x 4 (null with npub = 0)
int fs_batch_run(pbf_ctx* ctx, const uint64_t h0[4], uint64_t count, const uint64_t* d_pts, const uint64_t* d_f,
                 const uint64_t* d_pub, uint64_t npub, uint64_t* d_chal, uint64_t* d_u, uint64_t* d_rho, hipStream_t s);

}  // namespace pbf
