/* The host side of the tiered direct solver (lsb_direct.c) under ASan + UBSan: a stand-alone program that orders,
 * counts and builds the tiered inverse factor of the operators given as arguments (matrix files, symmetrised from
 * their upper triangle as the solver does; synth:SPEC for a grid) and of one row on its own, in 1 .. 4 tiers, the most
 * there are, and the automatic choice.  Built and run by tests/test_direct_tiers_asan.py; no GPU, no Python. */
#include "lsbench.h"
#include "lsbench_hip.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int run(const char *name, const struct csr *S) {
  const unsigned n = S->nrows;
  unsigned *perm = (unsigned *)malloc((size_t)(n ? n : 1) * sizeof(unsigned));
  if (!perm || lsb_csr_nd(S, perm))
    return 1;
  int fail = 0, refused = 0;
  static const unsigned ask[] = {1, 2, 3, 4, LSB_DIRECT_MAX_TIERS, 0};
  for (unsigned a = 0; a < sizeof ask / sizeof ask[0] && !fail; a++) {
    unsigned long long w = 0, c = 0;
    unsigned h = 0;
    int why = 0;
    if (ask[a] && lsb_csr_tiered_count(S, perm, ask[a], &w, &c, &h))
      fail = 1;
    struct lsb_tierinv *T = lsb_csr_tiered_inverse(S, perm, ask[a], &why);
    if (!T) {
      refused += why == 1; /* not positive definite: every tier count says so */
      fail |= why != 1;
      continue;
    }
    const unsigned lo1 = T->lo[T->ntier > 1 ? 1 : T->ntier];
    /* read every array to its end: the sums keep the loads alive */
    double s = 0.0;
    unsigned long long u = 0;
    for (unsigned k = 0; k < n; k++)
      u += T->perm[k] + T->first[k] + T->parent[k] + T->run_end[k] + T->woff[k + 1];
    for (unsigned long long e = 0; e < T->woff[n]; e++)
      s += T->vals[e];
    const unsigned nc = T->coffs[n - lo1];
    for (unsigned e = 0; e < nc; e++)
      s += T->cvals[e] - T->tvals[e], u += T->ccols[e] + T->tcols[e];
    size_t nt = 0;
    for (unsigned t = 1; t < T->ntier; t++)
      nt += (size_t)T->lo[t] + 1;
    for (size_t k = 0; k < nt; k++)
      u += T->toffs[k];
    if (ask[a] && (T->woff[n] != w || nc != c || T->ntier > ask[a] || T->lo[T->ntier] != n))
      fail = 1;
    if (s != s)
      fail = 1;
    printf("   %s: asked %u tiers, got %u, %llu + %u entries, height %u (%llu)\n", name, ask[a], T->ntier, T->woff[n],
           nc, h, u & 1);
    lsb_tierinv_free(T);
  }
  /* what is no permutation is refused, not read out of bounds */
  if (n > 1) {
    perm[0] = perm[1];
    int why = 0;
    if (lsb_csr_tiered_inverse(S, perm, 2, &why) || why != 3 || !lsb_csr_tiered_count(S, perm, 2, NULL, NULL, NULL))
      fail = 1;
  }
  free(perm);
  if (refused && refused != 6)
    fail = 1;
  printf("%s %s%s\n", fail ? "FAILED" : "ok", name, refused ? " (not positive definite: refused)" : "");
  return fail;
}

int main(int argc, char **argv) {
  int fail = 0;
  for (int a = 1; a < argc; a++) {
    struct csr *A = lsbench_matrix_read(argv[a]);
    struct csr *S = strncmp(argv[a], "synth:", 6) ? lsb_csr_symmetrize_upper(A) : lsb_csr_copy_base0(A);
    fail |= run(argv[a], S);
    lsb_csr_free(S);
    lsbench_matrix_free(A);
  }
  unsigned offs[2] = {0, 1}, cols[1] = {0};
  double vals[1] = {3.0};
  struct csr one = {1, 0, offs, cols, vals};
  fail |= run("one row", &one);
  return fail;
}
