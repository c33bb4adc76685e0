// The Fiat-Shamir transcript of a batch on ONE host thread, over the same __host__ Keccak-f[1600]
// and messages the kernels of csrc/transcript.hip run (csrc/transcript.hpp): per proof the tree
// digest of its public inputs and the six rounds, then the batch's tree and weights. This is the
// figure the case for hashing batches on the GPU rests on.
//   fs_host COUNT NPUB [REPS]   -> one line: count npub permutations ms(median of REPS) us/permutation
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>
#include "../../plonk-by-fingers_amd/csrc/transcript.hpp"

using namespace pbf;

static uint64_t sm64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const uint64_t count = strtoull(argv[1], nullptr, 10), npub = strtoull(argv[2], nullptr, 10);
  const int reps = argc > 3 ? atoi(argv[3]) : 5;
  uint64_t seed = 0x5EED0F5;
  std::vector<uint64_t> pts(72 * count), f(28 * count), pub(4 * count * npub), chal(20 * count), u(4 * count),
      t6(4 * count), rho(4 * count), work;
  for (auto* v : {&pts, &f, &pub})
    for (size_t i = 0; i < v->size(); ++i) (*v)[i] = sm64(seed) >> (i % 4 == 3 ? 4 : 0);  // below 2^252
  uint64_t h0[4] = {sm64(seed), sm64(seed), sm64(seed), sm64(seed)};
  std::vector<double> ms;
  for (int r = 0; r < reps; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t i = 0; i < count; ++i) {
      uint64_t P[4];
      fs_tree_digest_host(FS_TAG_PUB, pub.data() + 4 * i * npub, npub, P);
      fs_proof_chain(h0, P, pts.data() + 72 * i, f.data() + 28 * i, chal.data() + 20 * i, u.data() + 4 * i,
                     t6.data() + 4 * i);
    }
    work = t6;
    uint64_t root[4], T[4];
    fs_tree_root_host(work.data(), count, false, root);
    fs_tree_close(FS_TAG_BATCH, count, root, T);
    for (uint64_t i = 0; i < count; ++i) fs_rho(T, i, rho.data() + 4 * i);
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  std::sort(ms.begin(), ms.end());
  // permutations: a tree over m items takes ceil(m/4) + ceil(m/16) + .. nodes and one closing hash
  const auto tree = [](uint64_t m) {
    uint64_t k = 1;
    do {
      m = (m + 3) / 4;
      k += m;
    } while (m > 1);
    return k;
  };
  const uint64_t perms = count * ((npub ? tree(npub) : 1) + 10 + 1) + tree(count);
  uint64_t sink = 0;
  for (uint64_t x : rho) sink ^= x;
  for (uint64_t x : chal) sink ^= x;
  printf("host, one thread: count %llu npub %llu | %llu permutations | %.3f ms (min %.3f, %d reps) | %.3f us per "
         "permutation | check %016llx\n",
         (unsigned long long)count, (unsigned long long)npub, (unsigned long long)perms, ms[ms.size() / 2], ms[0], reps,
         1e3 * ms[ms.size() / 2] / perms, (unsigned long long)sink);
  return 0;
}
