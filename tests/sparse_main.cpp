// sparse_main.cpp -- gx_sparse.h in a program of its own (tests/test_sparse.py builds it under the sanitizers).
// Input, case after case:  "K nA nB", then nA + nB lines "key v1 .. vK": two lists, each ascending, keys may repeat.
// Output per case: each list as gx_sparse::append folds it ("fold A" / "fold B"), then A with B added ("add"); one
// "key v1 .. vK" line per entry, "--" after each list.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../genrich_amd/csrc/gx_sparse.h"

using gx_sparse::Col;

template <size_t K>
struct List {
  Col key, val[K];
  void read(FILE* f, size_t n) {
    Col* out[K];
    for (size_t c = 0; c < K; c++) out[c] = &val[c];
    for (size_t i = 0; i < n; i++) {
      uint64_t k = 0, v[K];
      if (fscanf(f, "%" SCNu64, &k) != 1) exit(2);
      for (size_t c = 0; c < K; c++)
        if (fscanf(f, "%" SCNu64, &v[c]) != 1) exit(2);
      gx_sparse::append(key, out, k, v);
    }
  }
  void print(const char* what) const {
    printf("%s\n", what);
    for (size_t i = 0; i < key.size(); i++) {
      printf("%" PRIu64, key[i]);
      for (size_t c = 0; c < K; c++) printf(" %" PRIu64, val[c][i]);
      printf("\n");
    }
    printf("--\n");
  }
};

template <size_t K>
void run(FILE* f, size_t nA, size_t nB) {
  List<K> a, b;
  a.read(f, nA);
  b.read(f, nB);
  a.print("fold A");
  b.print("fold B");
  Col* av[K];
  const Col* bv[K];
  for (size_t c = 0; c < K; c++) {
    av[c] = &a.val[c];
    bv[c] = &b.val[c];
  }
  gx_sparse::add(a.key, av, b.key, bv);
  a.print("add");
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  unsigned K = 0;
  size_t nA = 0, nB = 0;
  while (fscanf(f, "%u %zu %zu", &K, &nA, &nB) == 3) {
    if (K == 1) run<1>(f, nA, nB);
    else if (K == 2) run<2>(f, nA, nB);
    else if (K == 3) run<3>(f, nA, nB);
    else return 2;
  }
  fclose(f);
  return 0;
}
