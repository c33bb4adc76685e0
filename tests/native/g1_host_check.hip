// Host-side check of the BN254 G1 group law (csrc/ec_bn254.hpp): the G1:: functions are
// __host__ __device__, and their host build is what msm_finish_host and the prover's commitment
// collection run. Reads the case table tests/group_device_inputs.py writes (host_case_lines():
// the operand tables of tests/test_group_device_gpu.py, every exit of every addition, with the
// results of the integer restatement of the formulas), one case per line:
//
//   <op> <k> <v0> <v1> ...      values: canonical plain field elements, 64 hex digits each
//
// inputs then expected outputs (XYZZ point: 4 values, affine: 2). Every result must equal the
// expected one coordinate for coordinate (in Montgomery form below q). Prints bad=<mismatches>.
#include "../../plonk-by-fingers_amd/csrc/ec_bn254.hpp"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace pbf;
#if !defined(__HIP_DEVICE_COMPILE__)  // host-only check
static long bad = 0, seen = 0;

static bool parse256(const char* s, U256* out) {
  if (strlen(s) != 64) return false;
  for (int i = 0; i < 8; ++i) {
    uint32_t w = 0;
    for (int j = 0; j < 8; ++j) {
      const char c = s[(7 - i) * 8 + j];
      const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
      if (d < 0) return false;
      w = (w << 4) | (uint32_t)d;
    }
    out->w[i] = w;
  }
  return true;
}
static Xyzz xyzz_m(const U256* v) {
  Xyzz r;
  r.X = Fq::to_mont(v[0]), r.Y = Fq::to_mont(v[1]), r.ZZ = Fq::to_mont(v[2]), r.ZZZ = Fq::to_mont(v[3]);
  return r;
}
static Affine aff_m(const U256* v) {
  Affine r;
  r.x = Fq::to_mont(v[0]), r.y = Fq::to_mont(v[1]);
  return r;
}
static bool same_m(const U256& got_m, const U256& want_plain) {
  return !Fq::geq_p(got_m) && Fq::eq(Fq::from_mont(got_m), want_plain);
}
static bool same_xyzz(const Xyzz& g, const U256* w) {
  return same_m(g.X, w[0]) && same_m(g.Y, w[1]) && same_m(g.ZZ, w[2]) && same_m(g.ZZZ, w[3]);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<char> line(1 << 12);
  while (fgets(line.data(), (int)line.size(), f)) {
    std::vector<std::string> tok;
    for (char* t = strtok(line.data(), " \n"); t; t = strtok(nullptr, " \n")) tok.push_back(t);
    if (tok.empty()) continue;
    const std::string& op = tok[0];
    const uint32_t k = tok.size() > 1 ? (uint32_t)strtoul(tok[1].c_str(), nullptr, 10) : 0;
    std::vector<U256> v(tok.size() > 2 ? tok.size() - 2 : 0);
    bool ok = tok.size() > 2;
    for (size_t i = 0; ok && i < v.size(); ++i) ok = parse256(tok[i + 2].c_str(), &v[i]);
    const size_t n = v.size();
    if (!ok) {  // an unreadable line: counted below
    } else if (op == "mdbl" && n == 6) {
      ok = same_xyzz(G1::mdbl(aff_m(&v[0])), &v[2]);
    } else if (op == "dbl" && n == 8) {
      ok = same_xyzz(G1::dbl(xyzz_m(&v[0])), &v[4]);
    } else if (op == "dbl2" && n == 8) {
      ok = same_xyzz(G1::dbl2(xyzz_m(&v[0])), &v[4]);
    } else if (op == "madd" && n == 10) {
      ok = same_xyzz(G1::madd(xyzz_m(&v[0]), aff_m(&v[4])), &v[6]);
    } else if (op == "madd_tp" && n == 10) {
      ok = same_xyzz(G1::madd_tp(xyzz_m(&v[0]), aff_m(&v[4])), &v[6]);
    } else if (op == "add" && n == 12) {
      ok = same_xyzz(G1::add(xyzz_m(&v[0]), xyzz_m(&v[4])), &v[8]);
    } else if (op == "add2" && n == 12) {
      ok = same_xyzz(G1::add2(xyzz_m(&v[0]), xyzz_m(&v[4])), &v[8]);
    } else if (op == "mul_small" && n == 8) {
      ok = same_xyzz(G1::mul_small(xyzz_m(&v[0]), k), &v[4]);
    } else if (op == "to_affine" && n == 6) {
      U256 x, y;
      G1::to_affine_plain(xyzz_m(&v[0]), &x, &y);
      ok = Fq::eq(x, v[4]) && Fq::eq(y, v[5]);
    } else {
      ok = false;  // an unknown op or a wrong value count
    }
    ++seen;
    if (!ok && bad++ < 8) printf("mismatch: case %ld, %s k=%u\n", seen, op.c_str(), k);
  }
  fclose(f);
  printf("g1_host_check cases=%ld bad=%ld\n", seen, bad);
  return bad ? 1 : 0;
}
#endif
