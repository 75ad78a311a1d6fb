/*
 * Geometric multigrid on constant-coefficient grids (LSB_PRECOND_GMG), pure host logic; hip_gmg_drv.c applies it
 * through the kernels of hip_gmg.hip.  No level has a matrix: every level is the 5- or 7-point stencil with the one
 * off-diagonal value -c, and what differs between the levels is a handful of numbers.
 *
 *   detection    the operator is  a  on the diagonal and  -c  at every grid neighbour that exists, nothing else,
 *                c > 0 and a == 2 dim c exactly, on an nx x ny [x nz] grid, row (k ny + j) nx + i (lsb_gmg_detect)
 *   levels       per level and dimension n_d points and delta_d, the distance from the last point to the far boundary
 *                in the level's spacing (the near boundary is at distance 1).  Level 0: delta = 1.  Coarse points sit
 *                at the fine indices 2 j + 1: n' = n / 2, delta' = delta / 2 (n even) or (1 + delta) / 2 (n odd).  All
 *                dimensions coarsen together, until <= `coarse` rows, some n_d < 4, or the level cap (lsb_gmg_plan)
 *   operator     off-diagonals -c, diagonal D = c (2 dim + sum_d [i_d == n_d - 1] (1 / delta_d - 1)): the same
 *                stencil with a correction on the far faces, 2^dim distinct diagonals (lsb_gmg_diagonals)
 *   P            the tensor product of: fine 2 j + 1 takes c_j; fine 2 j takes (c_{j-1} + c_j) / 2 with c_{-1} =
 *                c_{n'} = 0; n odd: the last fine point n - 1 takes c_{n'-1} delta / (1 + delta)
 *   R            sigma P^T, sigma = 4 / 2^dim
 *   smoother     damped Jacobi, w_i = omega / D_i, omega = 4/5 (2-D), 6/7 (3-D)
 *   coarsest     dense inverse by Cholesky on the host (lsb_amg_coarse_inverse)
 */
#include <math.h>
#include <string.h>

#include "lsb_impl.h"

/* 0: the operator qualifies and *g says how; else which rule it breaks (the text: lsb_gmg_why) */
int lsb_gmg_detect(const struct csr *S, struct lsb_gmg_grid *g) {
  if (!S || !g || S->nrows < 4)
    return 1;
  memset(g, 0, sizeof *g);
  const unsigned n = S->nrows, base = S->base;
  /* row 0 holds the diagonal and one forward neighbour per dimension: at +1, +nx, +nx ny */
  const unsigned len0 = S->offs[1] - S->offs[0];
  if (len0 != 3 && len0 != 4)
    return 2;
  const unsigned dim = len0 - 1;
  unsigned off[3] = {0, 0, 0}, have = 0;
  double a = 0.0, c = 0.0;
  for (unsigned e = S->offs[0]; e < S->offs[1]; e++) {
    const unsigned col = S->cols[e] - base;
    if (col >= n)
      return 2;
    if (col == 0)
      a = S->vals[e];
    else {
      unsigned at = have++;
      if (at >= dim)
        return 2; /* no diagonal in row 0 */
      for (; at > 0 && off[at - 1] > col; at--)
        off[at] = off[at - 1];
      off[at] = col;
      if (col == 1)
        c = -S->vals[e];
    }
  }
  if (have != dim || off[0] != 1 || off[1] < 2 || n % off[1] ||
      (dim == 3 && (off[2] <= off[1] || off[2] % off[1] || n % off[2])))
    return 2;
  const unsigned nx = off[1], ny = dim == 3 ? off[2] / nx : n / nx, nz = dim == 3 ? n / off[2] : 1;
  if (nx < 2 || ny < 2 || (dim == 3 && nz < 2) || (unsigned long long)nx * ny * nz != n)
    return 2;
  if (!(c > 0.0) || !isfinite(c))
    return 3;
  if (a != 2.0 * dim * c)
    return 4;
  const unsigned nd[3] = {nx, ny, nz}, stride[3] = {1, nx, nx * ny};
  for (unsigned r = 0; r < n; r++) {
    const unsigned id[3] = {r % nx, r / nx % ny, r / nx / ny};
    unsigned want = 1, seen = 0; /* bit 0 the diagonal, bits 1 + 2 d and 2 + 2 d the neighbours of dimension d */
    for (unsigned d = 0; d < dim; d++)
      want |= (id[d] > 0 ? 1u << (1 + 2 * d) : 0u) | (id[d] + 1 < nd[d] ? 1u << (2 + 2 * d) : 0u);
    for (unsigned e = S->offs[r]; e < S->offs[r + 1]; e++) {
      const unsigned col = S->cols[e] - base;
      unsigned bit = 0;
      if (col == r)
        bit = 1;
      for (unsigned d = 0; d < dim && !bit; d++)
        bit = (col + stride[d] == r ? 1u << (1 + 2 * d) : 0u) | (col == r + stride[d] ? 1u << (2 + 2 * d) : 0u);
      if (!bit || (seen & bit) || !(want & bit))
        return 2; /* an entry that is no grid neighbour, twice, or across the end of a line */
      seen |= bit;
      if (bit == 1 ? S->vals[e] != a : S->vals[e] != -c)
        return bit == 1 ? 4 : 3;
    }
    if (seen != want)
      return 2;
  }
  g->dim = dim, g->n[0] = nx, g->n[1] = ny, g->n[2] = nz, g->c = c;
  return 0;
}

const char *lsb_gmg_why(int rc) {
  switch (rc) {
  case 0: return "it qualifies";
  case 1: return "fewer than 4 rows";
  case 2: return "its rows are not the 5- or 7-point stencil of an nx x ny [x nz] grid";
  case 3: return "its off-diagonal entries are not one value -c with c > 0";
  case 4: return "its diagonal is not 2 dim c in every row";
  default: return "unknown";
  }
}

int lsb_gmg_plan(const struct lsb_gmg_grid *g, unsigned coarse, unsigned max_levels, struct lsb_gmg_level *lv,
                 unsigned cap) {
  if (!g || !lv || cap < 1 || (g->dim != 2 && g->dim != 3))
    return -2;
  if (max_levels < 1)
    max_levels = 1;
  if (max_levels > cap)
    max_levels = cap;
  if (coarse < 1)
    coarse = 1;
  unsigned nlev = 1;
  for (unsigned d = 0; d < 3; d++)
    lv[0].n[d] = d < g->dim ? g->n[d] : 1, lv[0].delta[d] = 1.0;
  for (;; nlev++) {
    const struct lsb_gmg_level *f = &lv[nlev - 1];
    unsigned long long rows = 1;
    int thin = 0;
    for (unsigned d = 0; d < g->dim; d++)
      rows *= f->n[d], thin |= f->n[d] < 4;
    if (rows <= coarse || thin || nlev >= max_levels) {
      if (rows > LSB_GMG_COARSE_MAX)
        return -1;
      return (int)nlev;
    }
    struct lsb_gmg_level *k = &lv[nlev];
    for (unsigned d = 0; d < 3; d++) {
      k->n[d] = d < g->dim ? f->n[d] / 2 : 1;
      k->delta[d] = d < g->dim ? (f->n[d] % 2 ? 0.5 * (1.0 + f->delta[d]) : 0.5 * f->delta[d]) : 1.0;
    }
  }
}

void lsb_gmg_diagonals(unsigned dim, double c, const double delta[3], double D[8], double w[8]) {
  const double omega = dim == 2 ? 4.0 / 5.0 : 6.0 / 7.0;
  for (unsigned m = 0; m < 8; m++) {
    double corr = 0.0;
    for (unsigned d = 0; d < dim; d++)
      if (m >> d & 1u)
        corr += 1.0 / delta[d] - 1.0;
    D[m] = c * (2.0 * dim + corr);
    w[m] = omega / D[m];
  }
}

/* the level's operator as a CSR with sorted columns: the coarsest level's, for the dense inverse */
struct csr *lsb_gmg_level_csr(unsigned dim, double c, const struct lsb_gmg_level *lv) {
  const unsigned nx = lv->n[0], ny = lv->n[1], nz = dim == 3 ? lv->n[2] : 1, n = nx * ny * nz;
  double D[8], w[8];
  lsb_gmg_diagonals(dim, c, lv->delta, D, w);
  struct csr *A = lsb_calloc(struct csr, 1);
  A->nrows = n, A->base = 0;
  A->offs = lsb_calloc(unsigned, (size_t)n + 1);
  A->cols = lsb_calloc(unsigned, (size_t)n * 7);
  A->vals = lsb_calloc(double, (size_t)n * 7);
  unsigned at = 0;
  for (unsigned r = 0; r < n; r++) {
    const unsigned i = r % nx, j = r / nx % ny, k = r / nx / ny;
    const unsigned m = (i == nx - 1) | (unsigned)(j == ny - 1) << 1 | (unsigned)(dim == 3 && k == nz - 1) << 2;
    A->offs[r] = at;
#define GMG_ENT(cond, col, v) \
  if (cond)                   \
    A->cols[at] = (col), A->vals[at] = (v), at++;
    GMG_ENT(dim == 3 && k > 0, r - nx * ny, -c)
    GMG_ENT(j > 0, r - nx, -c)
    GMG_ENT(i > 0, r - 1, -c)
    GMG_ENT(1, r, D[m])
    GMG_ENT(i + 1 < nx, r + 1, -c)
    GMG_ENT(j + 1 < ny, r + nx, -c)
    GMG_ENT(dim == 3 && k + 1 < nz, r + nx * ny, -c)
#undef GMG_ENT
  }
  A->offs[n] = at;
  return A;
}
