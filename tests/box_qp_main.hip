// Host program around cacto_amd/csrc/box_qp.h for tests/test_to_box_cpu.py (built there with
// hipcc -x hip --offload-host-only): reads box QPs, writes to_box_qp<M>'s answers.
//   in : per problem  M  H[M*M]  q[M]  lo[M]  hi[M]   (whitespace separated; inf / -inf allowed)
//   out: per problem  ok  free_mask  x[M] (hex floats)  Lf[M*M] (hex floats)
// M = 0 asks for the offsets of a node's box:  0  u  lo  hi  ->  1 0 box_offset_lo(u, lo) box_offset_hi(u, hi)
#include <cstdio>
#include <cstdlib>

#include "box_qp.h"

template <int M>
static bool one(FILE* in, FILE* out) {
  double H[M * M], q[M], lo[M], hi[M], x[M], Lf[M * M];
  for (int k = 0; k < M * M; ++k)
    if (fscanf(in, "%lf", &H[k]) != 1) return false;
  for (double* v : {q, lo, hi})
    for (int k = 0; k < M; ++k)
      if (fscanf(in, "%lf", &v[k]) != 1) return false;
  for (int k = 0; k < M; ++k) x[k] = 0.0;
  for (int k = 0; k < M * M; ++k) Lf[k] = 0.0;
  unsigned mask = 0u;
  const bool ok = cacto::to_box_qp<M>(H, q, lo, hi, x, &mask, Lf);
  fprintf(out, "%d %u", ok ? 1 : 0, mask);
  for (int k = 0; k < M; ++k) fprintf(out, " %a", x[k]);
  for (int k = 0; k < M * M; ++k) fprintf(out, " %a", Lf[k]);
  fprintf(out, "\n");
  return true;
}

static bool offsets(FILE* in, FILE* out) {
  double u, lo, hi;
  if (fscanf(in, "%lf %lf %lf", &u, &lo, &hi) != 3) return false;
  fprintf(out, "1 0 %a %a\n", cacto::box_offset_lo(u, lo), cacto::box_offset_hi(u, hi));
  return true;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) return 2;
  int M;
  while (fscanf(in, "%d", &M) == 1) {
    bool ok = false;
    switch (M) {
      case 0: ok = offsets(in, out); break;
      case 1: ok = one<1>(in, out); break;
      case 2: ok = one<2>(in, out); break;
      case 3: ok = one<3>(in, out); break;
      case 6: ok = one<6>(in, out); break;
      default: break;
    }
    if (!ok) return 3;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
