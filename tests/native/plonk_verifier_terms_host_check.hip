// Host harness over plonk_verifier_scalars and plonk_domain of csrc/plonk_terms.hpp
// (tests/test_plonk_verifier_terms_host.py): reads
//   n mode has_pi | alpha beta gamma z v k1 k2 | a_z b_z c_z s1_z s2_z r_z zw_z | u rho | N D
// from the file named on the command line (n, mode and has_pi decimal, the field elements as 64 hex
// digits, canonical; N and D only with has_pi = 1) and prints the 20 scalars in the order of out(j, .),
// one canonical 64-digit hex integer per line -- or the one line "Z_H(z) = 0" when the function
// reports that and hands out nothing.
#include <cstdio>
#include <cstdlib>
#include "../../plonk-by-fingers_amd/csrc/plonk_terms.hpp"

using namespace pbf;

static bool read_fr(FILE* f, U256* out) {
  char buf[80];
  if (fscanf(f, "%79s", buf) != 1) return false;
  uint64_t l[4];
  for (int k = 0; k < 4; ++k) {
    char part[17] = {0};
    for (int i = 0; i < 16; ++i) part[i] = buf[16 * (3 - k) + i];
    l[k] = strtoull(part, nullptr, 16);
  }
  if (!fr_canonical(l)) return false;
  *out = hm(l);
  return true;
}

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!f) return 2;
  unsigned long long n;
  int mode, has_pi;
  if (fscanf(f, "%llu %d %d", &n, &mode, &has_pi) != 3) return 2;
  PlonkChallenges ch;
  PlonkEvals e{};
  PlonkVerifierArgs g;
  U256* in[16] = {&ch.alpha, &ch.beta, &ch.gamma, &ch.z, &ch.v, &ch.k1, &ch.k2, &e.a_z,
                  &e.b_z,    &e.c_z,   &e.s1_z,   &e.s2_z, &e.r_z, &e.zw_z, &g.u,   &g.rho};
  for (U256* p : in)
    if (!read_fr(f, p)) return 2;
  uint64_t nd[8];  // Montgomery form, as plonk_pi_fraction_run stores the fraction
  for (int k = 0; k < 2 * has_pi; ++k) {
    U256 m;
    if (!read_fr(f, &m)) return 2;
    u256_to_u64(m, nd + 4 * k);
  }
  fclose(f);
  g.dom = plonk_domain(n);
  g.mode = mode;
  uint64_t out[20][4];
  bool seen[20] = {};
  const bool ok = plonk_verifier_scalars(ch, e, g, has_pi ? nd : nullptr, [&](int j, const U256& m) {
    hout(out[j], m);
    seen[j] = true;
  });
  if (!ok) {
    for (bool s : seen)
      if (s) return 3;
    printf("Z_H(z) = 0\n");
    return 0;
  }
  for (int j = 0; j < 20; ++j) {
    if (!seen[j]) return 3;
    printf("%016llx%016llx%016llx%016llx\n", (unsigned long long)out[j][3], (unsigned long long)out[j][2],
           (unsigned long long)out[j][1], (unsigned long long)out[j][0]);
  }
  return 0;
}
