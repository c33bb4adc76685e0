// Host harness over csrc/transcript.hpp (tests/test_transcript_host.py): the __host__ side of the
// Keccak-f[1600] and of every transcript message that the kernels of csrc/transcript.hip compile
// for the device. Reads commands from the file named on the command line, one per line, every
// value hexadecimal, and prints one line of hexadecimal per command:
//   keccak LEN BYTES A        Keccak-256 of LEN bytes (BYTES: 2 LEN digits, "-" when LEN = 0) read
//                             at an address that is A mod 8
//   tree TAG M X_0 .. X_M-1   the tree digest of M field elements (64 digits each) under TAG
//   chain H0 NPUB PUB.. 18 coordinates 7 fields
//                             alpha beta gamma z v u t6 (64 digits each, t6 as bytes)
//   rho COUNT T6_0 ..         rho_0 .. rho_COUNT-1 from the digests t6 (as bytes)
//   circuit MODE N NPUB K1 K2 16 coordinates G2S x 4
//                             the circuit digest (as bytes)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../plonk-by-fingers_amd/csrc/transcript.hpp"

using namespace pbf;

static FILE* in;

static std::string word() {
  char buf[1 << 12];
  if (fscanf(in, "%4095s", buf) != 1) exit(2);
  return buf;
}
static uint64_t num() { return strtoull(word().c_str(), nullptr, 16); }
// 64 digits, big-endian -> 4 little-endian limbs
static void limbs(uint64_t* l) {
  const std::string w = word();
  if (w.size() != 64) exit(2);
  for (int k = 0; k < 4; ++k) l[k] = strtoull(w.substr(16 * (3 - k), 16).c_str(), nullptr, 16);
}
// 64 digits as 32 bytes -> 4 lanes
static void digest(uint64_t* d) {
  uint64_t l[4];
  limbs(l);
  fs_be32(d, l);
}
static void put_limbs(const uint64_t* l) {
  printf("%016llx%016llx%016llx%016llx", (unsigned long long)l[3], (unsigned long long)l[2], (unsigned long long)l[1],
         (unsigned long long)l[0]);
}
static void put_digest(const uint64_t* d) {
  uint64_t l[4];
  fs_be32(l, d);  // the byte swap is its own inverse
  put_limbs(l);
}

int main(int argc, char** argv) {
  in = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!in) return 2;
  char cmd[32];
  while (fscanf(in, "%31s", cmd) == 1) {
    const std::string c = cmd;
    if (c == "keccak") {
      const uint64_t len = num();
      const std::string hex = word();
      std::vector<uint8_t> msg(len + 8);
      uint8_t* p = msg.data() + (num() & 7);  // the alignment to read at
      for (uint64_t i = 0; i < len; ++i) p[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
      uint64_t d[4];
      keccak256_bytes(p, len, d);
      put_digest(d);
    } else if (c == "tree") {
      const uint64_t tag = num(), m = num();
      std::vector<uint64_t> x(4 * m + 4);
      for (uint64_t i = 0; i < m; ++i) limbs(x.data() + 4 * i);
      uint64_t d[4];
      fs_tree_digest_host(tag, x.data(), m, d);
      put_digest(d);
    } else if (c == "chain") {
      uint64_t h0[4], P[4], pts[72], f[28], chal[20], u[4], t6[4];
      digest(h0);
      const uint64_t npub = num();
      std::vector<uint64_t> pub(4 * npub + 4);
      for (uint64_t i = 0; i < npub; ++i) limbs(pub.data() + 4 * i);
      for (int i = 0; i < 18; ++i) limbs(pts + 4 * i);
      for (int i = 0; i < 7; ++i) limbs(f + 4 * i);
      fs_tree_digest_host(FS_TAG_PUB, pub.data(), npub, P);
      fs_proof_chain(h0, P, pts, f, chal, u, t6);
      for (int i = 0; i < 5; ++i) put_limbs(chal + 4 * i), printf(" ");
      put_limbs(u);
      printf(" ");
      put_digest(t6);
    } else if (c == "rho") {
      const uint64_t count = num();
      std::vector<uint64_t> t(4 * count);
      for (uint64_t i = 0; i < count; ++i) digest(t.data() + 4 * i);
      uint64_t root[4], T[4];
      fs_tree_root_host(t.data(), count, false, root);
      fs_tree_close(FS_TAG_BATCH, count, root, T);
      for (uint64_t i = 0; i < count; ++i) {
        uint64_t r[4];
        fs_rho(T, i, r);
        put_limbs(r);
        printf(" ");
      }
    } else if (c == "circuit") {
      const int mode = (int)num();
      const uint64_t n = num(), npub = num();
      uint64_t k1k2[8], pre[8][8], g2[32] = {}, h0[4];
      limbs(k1k2), limbs(k1k2 + 4);
      for (int i = 0; i < 16; ++i) limbs(&pre[i / 2][4 * (i % 2)]);
      for (int i = 0; i < 4; ++i) limbs(g2 + 16 + 4 * i);
      fs_circuit_digest(mode, n, npub, k1k2, pre, g2, h0);
      put_digest(h0);
    } else {
      return 2;
    }
    printf("\n");
  }
  return 0;
}
