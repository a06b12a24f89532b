// CPU check of the task-head and signed-addition forms of bn254_curve29.cuh (driven by tests/test_curve29_task_head_cpu.py).
// input, one command per line (points as 16 hex words of the memory format, accumulators as 36 hex limbs X Y ZZ ZZZ):
//   "mmadd <a> <nega> <b> <negb>"   xyzz29_mmadd(+-a, +-b)
//   "from <q> <neg>"                xyzz29_from_affine(+-q)
//   "madd <acc> <q> <neg>"          xyzz29_madd(acc, q, neg), then on a second line "negate, then xyzz29_madd(acc, q)"
// output per result: 32 canonical words (xyzz29_to_words), then the 36 raw limbs
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../../circuits_halo2_amd/csrc/bn254_curve29.cuh"
using namespace sg;

static affine29 read_affine(std::istringstream& ss) {
  uint32_t w[16];
  for (int i = 0; i < 16; i++) ss >> std::hex >> w[i];
  return affine29_from_words(w);
}
static void print(const xyzz29& p) {
  uint32_t w[32];
  xyzz29_to_words(p, w);
  for (int i = 0; i < 32; i++) printf("%08x ", w[i]);
  const f29* c[4] = {&p.x, &p.y, &p.zz, &p.zzz};
  for (int k = 0; k < 4; k++)
    for (int i = 0; i < 9; i++) printf("%08x%c", c[k]->l[i], k == 3 && i == 8 ? '\n' : ' ');
}
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream ss(line);
    std::string op;
    ss >> op;
    if (op == "mmadd") {
      int na, nb;
      affine29 a = read_affine(ss);
      ss >> na;
      affine29 b = read_affine(ss);
      ss >> nb;
      if (na) affine29_negate(a);
      if (nb) affine29_negate(b);
      print(xyzz29_mmadd(a, b));
    } else if (op == "from") {
      int n;
      affine29 q = read_affine(ss);
      ss >> n;
      if (n) affine29_negate(q);
      print(xyzz29_from_affine(q));
    } else if (op == "madd") {
      xyzz29 acc;
      f29* c[4] = {&acc.x, &acc.y, &acc.zz, &acc.zzz};
      for (int k = 0; k < 4; k++)
        for (int i = 0; i < 9; i++) ss >> std::hex >> c[k]->l[i];
      int n;
      affine29 q = read_affine(ss);
      ss >> n;
      xyzz29 signed_form = acc, old_form = acc;
      xyzz29_madd(signed_form, q, n != 0);
      if (n) affine29_negate(q);
      xyzz29_madd(old_form, q);
      print(signed_form);
      print(old_form);
    } else if (!op.empty()) {
      fprintf(stderr, "unknown command %s\n", op.c_str());
      return 2;
    }
  }
  return 0;
}
