// Host harness over csrc/plonk_terms.hpp (tests/test_plonk_terms_host.py): reads
//   n mode | alpha beta gamma z v k1 k2 | a_z b_z c_z s1_z s2_z zw_z l1_z t_z r_z
// from the file named on the command line (n and mode decimal, the 16 field elements as 64 hex
// digits, canonical) and prints the seven coefficients of r(x), the nine of the W_z numerator and
// its constant term, one canonical 64-digit hex integer per line.
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
static void print_fr(const U256& m) {
  uint64_t l[4];
  hout(l, m);
  printf("%016llx%016llx%016llx%016llx\n", (unsigned long long)l[3], (unsigned long long)l[2],
         (unsigned long long)l[1], (unsigned long long)l[0]);
}

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!f) return 2;
  unsigned long long n;
  int mode;
  if (fscanf(f, "%llu %d", &n, &mode) != 2) return 2;
  PlonkChallenges ch;
  PlonkEvals e;
  U256* in[16] = {&ch.alpha, &ch.beta, &ch.gamma, &ch.z, &ch.v, &ch.k1, &ch.k2, &e.a_z, &e.b_z,
                  &e.c_z, &e.s1_z, &e.s2_z, &e.zw_z, &e.l1_z, &e.t_z, &e.r_z};
  for (U256* p : in)
    if (!read_fr(f, p)) return 2;
  fclose(f);
  U256 rc[7], wc[9];
  plonk_r_coeffs(ch, e, mode, rc);
  const U256 c0 = plonk_wz_coeffs(ch, e, n, wc);
  for (const U256& c : rc) print_fr(c);
  for (const U256& c : wc) print_fr(c);
  print_fr(c0);
  return 0;
}
