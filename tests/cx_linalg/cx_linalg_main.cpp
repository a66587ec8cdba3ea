// Host driver of csrc/cx_linalg.h for tests/test_cx_linalg_host.py:  cx_linalg_main f32|f64 <in> <out>
// in:  int32 cases, then per case int32 n, cols, items and A [items][n][n], X [items][n][cols] as interleaved (re, im)
// out: per case L [items][n][n] (lower triangle, the rest zero), L^-1 X and L^-H L^-1 X [items][n][cols] from the
//      run-time-size functions (NT = 0); for n = 2 and n = 4 the same three arrays again from the NT = n instantiations
#include <cstdio>
#include <cstring>
#include <vector>

#include "cx_linalg.h"

using namespace samd;

template <typename R, int NT> void run(int n, int cols, int items, const R* a, const R* x, FILE* out) {
  std::vector<cx<R>> L((size_t)items * n * n, C<R>(R(0), R(0))), Y((size_t)items * n * cols), Z;
  std::vector<cx<R>> w((size_t)n * n);
  memcpy(Y.data(), x, Y.size() * sizeof(cx<R>));
  for (int it = 0; it < items; ++it) {
    memcpy(w.data(), a + (size_t)2 * it * n * n, w.size() * sizeof(cx<R>));
    chol<R, NT>(w.data(), n);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j <= i; ++j) L[((size_t)it * n + i) * n + j] = w[i * n + j];
    fwd<R, NT>(w.data(), n, Y.data() + (size_t)it * n * cols, cols, cols);
  }
  Z = Y;
  for (int it = 0; it < items; ++it) {
    for (int i = 0; i < n * n; ++i) w[i] = L[(size_t)it * n * n + i];
    bwd<R, NT>(w.data(), n, Z.data() + (size_t)it * n * cols, cols, cols);
  }
  fwrite(L.data(), sizeof(cx<R>), L.size(), out);
  fwrite(Y.data(), sizeof(cx<R>), Y.size(), out);
  fwrite(Z.data(), sizeof(cx<R>), Z.size(), out);
}

template <typename R> int run_all(FILE* in, FILE* out) {
  int cases = 0;
  if (fread(&cases, sizeof(int), 1, in) != 1) return 1;
  for (int c = 0; c < cases; ++c) {
    int hdr[3];
    if (fread(hdr, sizeof(int), 3, in) != 3) return 1;
    const int n = hdr[0], cols = hdr[1], items = hdr[2];
    std::vector<R> a((size_t)2 * items * n * n), x((size_t)2 * items * n * cols);
    if (fread(a.data(), sizeof(R), a.size(), in) != a.size() || fread(x.data(), sizeof(R), x.size(), in) != x.size()) return 1;
    run<R, 0>(n, cols, items, a.data(), x.data(), out);
    if (n == 2) run<R, 2>(n, cols, items, a.data(), x.data(), out);
    if (n == 4) run<R, 4>(n, cols, items, a.data(), x.data(), out);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) return 2;
  const int rc = strcmp(argv[1], "f64") == 0 ? run_all<double>(in, out) : run_all<float>(in, out);
  fclose(in);
  return fclose(out) != 0 || rc;
}
