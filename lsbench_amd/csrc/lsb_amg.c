/*
 * Smoothed-aggregation AMG hierarchy (LSB_PRECOND_AMG; hip_amg_drv.c applies it through
 * hip_amg.hip).  Host set-up, untimed, like FSAI's and CHOLMOD's factorisation
 * (src/cholmod-impl.h:25-26).  The rules are fixed so that a test restates them exactly:
 *
 *   strength     j != i is strong for i when |a_ij| >= theta sqrt(|a_ii a_jj|)
 *   aggregates   three passes, each in ascending row order
 *                  1. an unaggregated row whose strong neighbours are all unaggregated starts
 *                     an aggregate with them;
 *                  2. a row still unaggregated with a strong neighbour aggregated by pass 1
 *                     joins that neighbour's aggregate, the neighbour of largest |a_ij|, the
 *                     lowest column on a tie (rows joined in this pass recruit nobody: no
 *                     chains, aggregates stay local);
 *                  3. a row still unaggregated with strong neighbours starts an aggregate with
 *                     its still-unaggregated strong neighbours.
 *                Rows without a strong neighbour stay -1: an empty row of the tentative
 *                prolongator.
 *   P_tent       piecewise constant, column j scaled to unit 2-norm (1 / sqrt(|aggregate j|))
 *   P            (I - omega D^-1 A) P_tent, omega = 4 / (3 rho), rho = max_i sum_j |a_ij| / a_ii
 *                (Gershgorin: no eigen-iteration); R = P^T by a counting sort
 *   A_c          R (A P): every row summed over the left factor's entries in ascending column
 *                order, output columns sorted -- the same bits for any OMP_NUM_THREADS
 *   stop         n <= coarse, no aggregate, n_next > 0.8 n, or max_levels levels
 *   coarsest     dense inverse by Cholesky on the host
 */
#define _GNU_SOURCE
#include <math.h>
#include <omp.h>
#include <string.h>

#include "lsb_impl.h"

#define AMG_MAX_COARSE_DENSE 4096 /* rows of the coarsest level: its dense inverse is 8 nc^2 bytes */

static struct csr *amg_csr_alloc(unsigned n, unsigned long long nnz) {
  if (nnz > 0xFFFFFFF0ull)
    errx(EXIT_FAILURE, "hip_cdna4: an AMG level has %llu entries, more than 32-bit offsets hold", nnz);
  struct csr *A = lsb_calloc(struct csr, 1);
  A->nrows = n, A->base = 0;
  A->offs = lsb_calloc(unsigned, (size_t)n + 1);
  A->cols = lsb_calloc(unsigned, (size_t)nnz);
  A->vals = lsb_calloc(double, (size_t)nnz);
  if (!A->offs || !A->cols || !A->vals)
    errx(EXIT_FAILURE, "hip_cdna4: out of host memory for an AMG level (%u rows, %llu entries)", n, nnz);
  return A;
}

/* (column, value) pairs of one row by column; insertion sort for the short rows */
static void amg_sort_row(unsigned *c, double *v, unsigned m) {
  for (unsigned a = 1; a < m; a++) {
    const unsigned cc = c[a];
    const double vv = v[a];
    unsigned b = a;
    while (b > 0 && c[b - 1] > cc)
      c[b] = c[b - 1], v[b] = v[b - 1], b--;
    c[b] = cc, v[b] = vv;
  }
}

/* 0-based copy with sorted columns and merged duplicates (summed in storage order) */
static struct csr *amg_canonical(const struct csr *S) {
  const unsigned n = S->nrows, base = S->base;
  struct csr *A = amg_csr_alloc(n, S->offs[n]);
  unsigned at = 0;
  for (unsigned i = 0; i < n; i++) {
    const unsigned r0 = at;
    for (unsigned e = S->offs[i]; e < S->offs[i + 1]; e++)
      A->cols[at] = S->cols[e] - base, A->vals[at] = S->vals[e], at++;
    /* stable: duplicates keep their storage order, and are summed in it */
    amg_sort_row(A->cols + r0, A->vals + r0, at - r0);
    unsigned w = r0;
    for (unsigned e = r0; e < at; e++) {
      if (w > r0 && A->cols[w - 1] == A->cols[e])
        A->vals[w - 1] += A->vals[e];
      else
        A->cols[w] = A->cols[e], A->vals[w] = A->vals[e], w++;
    }
    at = w;
    A->offs[i + 1] = at;
  }
  return A;
}

static double *amg_diag(const struct csr *A) {
  const unsigned n = A->nrows;
  double *d = lsb_calloc(double, n);
  for (unsigned i = 0; i < n; i++) {
    for (unsigned e = A->offs[i]; e < A->offs[i + 1]; e++)
      if (A->cols[e] == i)
        d[i] += A->vals[e];
    if (!(d[i] > 0.0))
      errx(EXIT_FAILURE, "hip_cdna4: --precond amg needs a symmetric positive definite operator (row %u of "
                         "a %u-row level has diagonal %g)", i, n, d[i]);
  }
  return d;
}

static int amg_strong(const struct csr *A, const double *d, double theta, unsigned i, unsigned e) {
  const unsigned j = A->cols[e];
  return j != i && fabs(A->vals[e]) >= theta * sqrt(fabs(d[i] * d[j]));
}

static int *amg_aggregate_diag(const struct csr *A, const double *d, double theta, unsigned *naggr) {
  const unsigned n = A->nrows;
  int *agg = (int *)malloc((size_t)(n ? n : 1) * sizeof(int));
  if (!agg)
    errx(EXIT_FAILURE, "hip_cdna4: out of host memory for the AMG aggregates");
  for (unsigned i = 0; i < n; i++)
    agg[i] = -1;
  int na = 0;
  for (unsigned i = 0; i < n; i++) { /* pass 1 */
    if (agg[i] != -1)
      continue;
    int any = 0, free_all = 1;
    for (unsigned e = A->offs[i]; e < A->offs[i + 1] && free_all; e++)
      if (amg_strong(A, d, theta, i, e))
        any = 1, free_all = agg[A->cols[e]] == -1;
    if (!any || !free_all)
      continue;
    agg[i] = na;
    for (unsigned e = A->offs[i]; e < A->offs[i + 1]; e++)
      if (amg_strong(A, d, theta, i, e))
        agg[A->cols[e]] = na;
    na++;
  }
  int *first = (int *)malloc((size_t)(n ? n : 1) * sizeof(int)); /* the aggregates of pass 1 */
  if (!first)
    errx(EXIT_FAILURE, "hip_cdna4: out of host memory for the AMG aggregates");
  memcpy(first, agg, (size_t)n * sizeof(int));
  for (unsigned i = 0; i < n; i++) { /* pass 2: joins pass-1 aggregates only (no chains of joins) */
    if (agg[i] != -1)
      continue;
    long long best = -1;
    double bw = 0.0;
    for (unsigned e = A->offs[i]; e < A->offs[i + 1]; e++) {
      const unsigned j = A->cols[e];
      if (!amg_strong(A, d, theta, i, e) || first[j] == -1)
        continue;
      const double w = fabs(A->vals[e]);
      if (best < 0 || w > bw || (w == bw && (long long)j < best))
        best = j, bw = w;
    }
    if (best >= 0)
      agg[i] = first[best];
  }
  free(first);
  for (unsigned i = 0; i < n; i++) { /* pass 3 */
    if (agg[i] != -1)
      continue;
    int any = 0;
    for (unsigned e = A->offs[i]; e < A->offs[i + 1] && !any; e++)
      any = amg_strong(A, d, theta, i, e);
    if (!any)
      continue;
    agg[i] = na;
    for (unsigned e = A->offs[i]; e < A->offs[i + 1]; e++)
      if (amg_strong(A, d, theta, i, e) && agg[A->cols[e]] == -1)
        agg[A->cols[e]] = na;
    na++;
  }
  *naggr = (unsigned)na;
  return agg;
}

int *lsb_amg_aggregate(const struct csr *A, double theta, unsigned *naggr) {
  if (!A || !naggr)
    return NULL;
  struct csr *C = amg_canonical(A);
  double *d = amg_diag(C);
  int *agg = amg_aggregate_diag(C, d, theta, naggr);
  free(d);
  lsb_csr_free(C);
  return agg;
}

/* C = L * Rt-style sparse product, row i of C = sum over the entries (k, a_ik) of row i of L, in
 * ascending k, of a_ik * row k of Rm; output columns sorted.  Two passes of the same row routine
 * (count, fill); per thread: a dense accumulator over Rm's columns and a list of touched columns. */
static struct csr *amg_spgemm(const struct csr *L, const struct csr *Rm, unsigned ncols) {
  const unsigned n = L->nrows;
  unsigned *len = lsb_calloc(unsigned, (size_t)n + 1);
  struct csr *C = NULL;
  for (int pass = 0; pass < 2; pass++) {
    if (pass == 1) {
      unsigned long long acc = 0;
      for (unsigned i = 0; i < n; i++)
        acc += len[i];
      C = amg_csr_alloc(n, acc);
      acc = 0;
      for (unsigned i = 0; i < n; i++)
        C->offs[i] = (unsigned)acc, acc += len[i];
      C->offs[n] = (unsigned)acc;
    }
#pragma omp parallel
    {
      double *acc = (double *)calloc((size_t)(ncols ? ncols : 1), sizeof(double));
      unsigned *mark = (unsigned *)calloc((size_t)(ncols ? ncols : 1), sizeof(unsigned)); /* i + 1: touched by row i */
      unsigned *list = (unsigned *)malloc((size_t)(ncols ? ncols : 1) * sizeof(unsigned));
      if (!acc || !mark || !list)
        errx(EXIT_FAILURE, "hip_cdna4: out of host memory for the AMG Galerkin product (%u columns)", ncols);
#pragma omp for schedule(dynamic, 512)
      for (long long ii = 0; ii < (long long)n; ii++) {
        const unsigned i = (unsigned)ii;
        unsigned cnt = 0;
        for (unsigned e = L->offs[i]; e < L->offs[i + 1]; e++) {
          const unsigned k = L->cols[e];
          const double a = L->vals[e];
          for (unsigned f = Rm->offs[k]; f < Rm->offs[k + 1]; f++) {
            const unsigned j = Rm->cols[f];
            if (mark[j] != i + 1)
              mark[j] = i + 1, acc[j] = 0.0, list[cnt++] = j;
            acc[j] += a * Rm->vals[f];
          }
        }
        if (pass == 0) {
          len[i] = cnt;
          continue;
        }
        unsigned *c = C->cols + C->offs[i];
        double *v = C->vals + C->offs[i];
        for (unsigned t = 0; t < cnt; t++)
          c[t] = list[t], v[t] = acc[list[t]];
        amg_sort_row(c, v, cnt);
      }
      free(acc), free(mark), free(list);
    }
  }
  free(len);
  return C;
}

/* transpose by a counting sort: rows of the result come out with ascending columns */
static struct csr *amg_transpose(const struct csr *P, unsigned ncols) {
  const unsigned n = P->nrows;
  struct csr *R = amg_csr_alloc(ncols, P->offs[n]);
  for (unsigned long long e = 0; e < P->offs[n]; e++)
    R->offs[P->cols[e] + 1]++;
  for (unsigned j = 0; j < ncols; j++)
    R->offs[j + 1] += R->offs[j];
  unsigned *at = lsb_calloc(unsigned, (size_t)ncols + 1);
  memcpy(at, R->offs, ((size_t)ncols + 1) * sizeof(unsigned));
  for (unsigned i = 0; i < n; i++)
    for (unsigned e = P->offs[i]; e < P->offs[i + 1]; e++) {
      const unsigned k = at[P->cols[e]]++;
      R->cols[k] = i, R->vals[k] = P->vals[e];
    }
  free(at);
  return R;
}

/* rho = max_i sum_j |a_ij| / a_ii >= lambda_max(D^-1 A) (Gershgorin): each row's |a_ij| summed in storage
 * order, the diagonal as amg_diag sums it.  No eigen-iteration, so the same bits for any thread count: the
 * prolongator's omega and the upper end of the Chebyshev smoother's interval (an estimate from a power
 * iteration fell below lambda_max on coarse Galerkin levels, and PCG then did not converge; DESIGN.md
 * section 4). */
double lsb_amg_gershgorin(const struct csr *A) {
  double rho = 0.0;
  for (unsigned i = 0; i < A->nrows; i++) {
    double s = 0.0, d = 0.0;
    for (unsigned e = A->offs[i]; e < A->offs[i + 1]; e++) {
      s += fabs(A->vals[e]);
      if (A->cols[e] - A->base == i)
        d += A->vals[e];
    }
    if (!(d > 0.0))
      errx(EXIT_FAILURE, "hip_cdna4: --precond amg needs a symmetric positive definite operator (row %u of "
                         "a %u-row level has diagonal %g)", i, A->nrows, d);
    if (s / d > rho)
      rho = s / d;
  }
  return rho;
}

/* The Chebyshev smoother's coefficients on [hi / ratio, hi] (ratio >= 1.5), degree deg: step k is
 *   d <- c1[k] d + c2[k] D^-1 (b - A x),  x <- x + d     (c1[0] = 0: step 0 does not read d)
 * with theta = (hi + lo) / 2, delta = (hi - lo) / 2, sigma = theta / delta, rho_0 = 1 / sigma,
 * rho_k = 1 / (2 sigma - rho_{k-1}), c1[k] = rho_k rho_{k-1}, c2[k] = 2 rho_k / delta, c2[0] = 1 / theta. */
void lsb_amg_cheb_coeffs(double hi, double ratio, unsigned deg, double *c1, double *c2) {
  if (!(ratio >= 1.5))
    ratio = 1.5;
  const double lo = hi / ratio, theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo), sigma = theta / delta;
  double rho = 1.0 / sigma;
  for (unsigned k = 0; k < deg; k++) {
    if (k == 0) {
      c1[0] = 0.0, c2[0] = 1.0 / theta;
      continue;
    }
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    c1[k] = rho_new * rho, c2[k] = 2.0 * rho_new / delta;
    rho = rho_new;
  }
}

/* P = (I - omega D^-1 A) P_tent; row i: for every entry (k, a_ik) of row i in ascending k with
 * agg[k] >= 0, column agg[k] gathers a_ik (summed in that order); then
 *   P_ij = [agg[i] == j] s_j - (omega / a_ii) * sum * s_j */
static struct csr *amg_prolongator(const struct csr *A, const double *d, const int *agg, unsigned na) {
  const unsigned n = A->nrows;
  double *scale = lsb_calloc(double, na);
  for (unsigned i = 0; i < n; i++)
    if (agg[i] >= 0)
      scale[agg[i]] += 1.0;
  for (unsigned j = 0; j < na; j++)
    scale[j] = 1.0 / sqrt(scale[j]);
  const double rho = lsb_amg_gershgorin(A);
  const double omega = 4.0 / (3.0 * rho);
  /* the pattern of row i: the aggregates of its columns (and of i itself) */
  unsigned *len = lsb_calloc(unsigned, (size_t)n + 1);
  struct csr *P = NULL;
  for (int pass = 0; pass < 2; pass++) {
    if (pass == 1) {
      unsigned long long acc = 0;
      for (unsigned i = 0; i < n; i++)
        acc += len[i];
      P = amg_csr_alloc(n, acc);
      acc = 0;
      for (unsigned i = 0; i < n; i++)
        P->offs[i] = (unsigned)acc, acc += len[i];
      P->offs[n] = (unsigned)acc;
    }
#pragma omp parallel for schedule(dynamic, 1024)
    for (long long ii = 0; ii < (long long)n; ii++) {
      const unsigned i = (unsigned)ii;
      unsigned cbuf[64], *c = cbuf;
      double vbuf[64], *v = vbuf;
      const unsigned m = A->offs[i + 1] - A->offs[i] + 1;
      if (m > 64) {
        c = (unsigned *)malloc((size_t)m * sizeof(unsigned)), v = (double *)malloc((size_t)m * sizeof(double));
        if (!c || !v)
          errx(EXIT_FAILURE, "hip_cdna4: out of host memory for the AMG prolongator");
      }
      unsigned cnt = 0;
      for (unsigned e = A->offs[i]; e < A->offs[i + 1]; e++) {
        const int g = agg[A->cols[e]];
        if (g < 0)
          continue;
        unsigned t = 0;
        while (t < cnt && c[t] != (unsigned)g)
          t++;
        if (t == cnt)
          c[cnt] = (unsigned)g, v[cnt] = 0.0, cnt++;
        v[t] += A->vals[e];
      }
      if (agg[i] >= 0) { /* (a row with a diagonal is in its own list already) */
        unsigned t = 0;
        while (t < cnt && c[t] != (unsigned)agg[i])
          t++;
        if (t == cnt)
          c[cnt] = (unsigned)agg[i], v[cnt] = 0.0, cnt++;
      }
      if (pass == 0)
        len[i] = cnt;
      else {
        const double w = omega / d[i];
        for (unsigned t = 0; t < cnt; t++) {
          const double s = scale[c[t]];
          v[t] = ((int)c[t] == agg[i] ? s : 0.0) - w * v[t] * s;
        }
        amg_sort_row(c, v, cnt);
        memcpy(P->cols + P->offs[i], c, cnt * sizeof(unsigned));
        memcpy(P->vals + P->offs[i], v, cnt * sizeof(double));
      }
      if (c != cbuf)
        free(c), free(v);
    }
  }
  free(len), free(scale);
  return P;
}

/* dense inverse of the SPD coarsest operator: Cholesky A = L L^T, then A^-1 column by column (the geometric
 * cycle's coarsest level comes here too: who = the option the messages name, what = the inverse as the out-of-memory
 * message calls it) */
double *lsb_amg_coarse_inverse(const struct csr *A, const char *who, const char *what) {
  const unsigned n = A->nrows;
  double *L = lsb_calloc(double, (size_t)n * n), *X = lsb_calloc(double, (size_t)n * n);
  if (!L || !X)
    errx(EXIT_FAILURE, "hip_cdna4: out of host memory for %s (%u rows)", what, n);
  for (unsigned i = 0; i < n; i++)
    for (unsigned e = A->offs[i]; e < A->offs[i + 1]; e++)
      L[(size_t)i * n + A->cols[e]] = A->vals[e];
  for (unsigned k = 0; k < n; k++) {
    double p = L[(size_t)k * n + k];
    for (unsigned t = 0; t < k; t++)
      p -= L[(size_t)k * n + t] * L[(size_t)k * n + t];
    if (!(p > 0.0))
      errx(EXIT_FAILURE, "hip_cdna4: %s needs a symmetric positive definite operator (the "
                         "coarsest level's Cholesky met a pivot <= 0 in row %u of %u)", who, k, n);
    const double lkk = sqrt(p);
    L[(size_t)k * n + k] = lkk;
#pragma omp parallel for schedule(static)
    for (long long ii = k + 1; ii < (long long)n; ii++) {
      const unsigned i = (unsigned)ii;
      double s = L[(size_t)i * n + k];
      for (unsigned t = 0; t < k; t++)
        s -= L[(size_t)i * n + t] * L[(size_t)k * n + t];
      L[(size_t)i * n + k] = s / lkk;
    }
  }
  /* column c of A^-1: L y = e_c, L^T x = y; written as row c (A^-1 is symmetric) */
#pragma omp parallel for schedule(dynamic, 4)
  for (long long cc = 0; cc < (long long)n; cc++) {
    const unsigned c = (unsigned)cc;
    double *x = X + (size_t)c * n;
    for (unsigned i = 0; i < n; i++) {
      double s = i == c ? 1.0 : 0.0;
      for (unsigned t = c; t < i; t++)
        s -= L[(size_t)i * n + t] * x[t];
      x[i] = i < c ? 0.0 : s / L[(size_t)i * n + i];
    }
    for (unsigned i = n; i-- > 0;) {
      double s = x[i];
      for (unsigned t = i + 1; t < n; t++)
        s -= L[(size_t)t * n + i] * x[t];
      x[i] = s / L[(size_t)i * n + i];
    }
  }
  /* exactly symmetric, so that the V-cycle stays a symmetric operator for CG */
  for (unsigned i = 0; i < n; i++)
    for (unsigned j = i + 1; j < n; j++) {
      const double v = 0.5 * (X[(size_t)i * n + j] + X[(size_t)j * n + i]);
      X[(size_t)i * n + j] = X[(size_t)j * n + i] = v;
    }
  free(L);
  return X;
}

struct lsb_amg_hier *lsb_amg_setup(const struct csr *S, double theta, unsigned coarse, unsigned max_levels) {
  if (!S || S->nrows == 0)
    return NULL;
  if (max_levels < 1)
    max_levels = 1;
  struct lsb_amg_hier *h = lsb_calloc(struct lsb_amg_hier, 1);
  h->lv = lsb_calloc(struct lsb_amg_level, max_levels);
  struct csr *A = amg_canonical(S);
  for (;;) {
    struct lsb_amg_level *L = &h->lv[h->nlev++];
    L->n = A->nrows, L->A = A;
    double *d = amg_diag(A);
    if (A->nrows <= coarse || h->nlev >= max_levels) {
      free(d);
      break;
    }
    unsigned na = 0;
    int *agg = amg_aggregate_diag(A, d, theta, &na);
    if (na == 0 || (double)na > 0.8 * A->nrows) {
      free(agg), free(d);
      break;
    }
    L->P = amg_prolongator(A, d, agg, na);
    L->R = amg_transpose(L->P, na);
    struct csr *AP = amg_spgemm(A, L->P, na);
    A = amg_spgemm(L->R, AP, na);
    lsb_csr_free(AP);
    free(agg), free(d);
  }
  h->nc = h->lv[h->nlev - 1].n;
  if (h->nc > AMG_MAX_COARSE_DENSE)
    errx(EXIT_FAILURE, "hip_cdna4: AMG coarsening stopped at %u rows (level %u), more than the %d a dense "
                       "coarse solve takes; raise --amg-max-levels or --amg-theta", h->nc, h->nlev,
         AMG_MAX_COARSE_DENSE);
  h->coarse_inv = lsb_amg_coarse_inverse(h->lv[h->nlev - 1].A, "--precond amg", "the AMG coarse inverse");
  return h;
}

void lsb_amg_free(struct lsb_amg_hier *h) {
  if (!h)
    return;
  for (unsigned l = 0; l < h->nlev; l++) {
    lsb_csr_free(h->lv[l].A);
    lsb_csr_free(h->lv[l].P);
    lsb_csr_free(h->lv[l].R);
  }
  free(h->lv), free(h->coarse_inv), free(h);
}

/* The entries of a CSR as hip_amg_f32.hip streams them: word j = {0-based column, bits of (float)vals[j]}.  The
 * conversion rounds to nearest even (the default mode; nothing here changes it).  NULL: some value is not finite
 * or rounds to +-inf -- the fp32 cycle refuses such a hierarchy. */
unsigned long long *lsb_csr_pack_f32(const struct csr *A) {
  if (!A)
    return NULL;
  const unsigned long long nnz = A->offs[A->nrows];
  unsigned long long *w = (unsigned long long *)malloc((size_t)(nnz ? nnz : 1) * sizeof *w);
  if (!w)
    return NULL;
  w[0] = 0;
  int ok = 1;
#pragma omp parallel for reduction(& : ok) schedule(static)
  for (long long j = 0; j < (long long)nnz; j++) {
    const float f = (float)A->vals[j];
    unsigned bits;
    memcpy(&bits, &f, sizeof bits);
    ok &= isfinite(A->vals[j]) && !isinf(f);
    w[j] = (unsigned long long)(A->cols[j] - A->base) | ((unsigned long long)bits << 32);
  }
  if (!ok) {
    free(w);
    return NULL;
  }
  return w;
}

/* ---- multicolour Gauss-Seidel (LSB_AMG_SMOOTH_MCGS): colouring, the colour-sorted copy, the check ------------ */

/* Greedy colouring of the stored pattern: rows in ascending order, each takes the smallest colour that none of its
 * stored off-diagonal neighbours holds yet.  Structural (a stored zero is a neighbour) and serial: the same result
 * for any thread count.  mark[c] == i + 1: colour c is held by a neighbour of row i. */
int *lsb_amg_colour(const struct csr *A, unsigned *ncolours) {
  if (!A || !ncolours)
    return NULL;
  const unsigned n = A->nrows, base = A->base;
  int *colour = (int *)malloc((size_t)(n ? n : 1) * sizeof(int));
  unsigned *mark = (unsigned *)calloc((size_t)n + 1, sizeof(unsigned));
  if (!colour || !mark)
    errx(EXIT_FAILURE, "hip_cdna4: out of host memory for the colouring of an AMG level (%u rows)", n);
  unsigned nc = 0;
  for (unsigned i = 0; i < n; i++)
    colour[i] = -1;
  for (unsigned i = 0; i < n; i++) {
    for (unsigned e = A->offs[i]; e < A->offs[i + 1]; e++) {
      const unsigned j = A->cols[e] - base;
      if (j != i && j < n && colour[j] >= 0)
        mark[colour[j]] = i + 1;
    }
    unsigned c = 0;
    while (mark[c] == i + 1) /* (a row has fewer than n neighbours: mark[n] is never reached) */
      c++;
    colour[i] = (int)c;
    if (c + 1 > nc)
      nc = c + 1;
  }
  free(mark);
  *ncolours = nc;
  return colour;
}

/* The rows of A regrouped colour by colour, ascending row order inside a colour (a counting sort: stable); column
 * ids stay A's, 0-based. */
struct lsb_mcgs *lsb_csr_mcgs(const struct csr *A, const int *colour, unsigned ncolours) {
  if (!A || !colour)
    return NULL;
  const unsigned n = A->nrows, base = A->base;
  for (unsigned i = 0; i < n; i++)
    if (colour[i] < 0 || (unsigned)colour[i] >= ncolours)
      return NULL;
  struct lsb_mcgs *M = lsb_calloc(struct lsb_mcgs, 1);
  const unsigned long long nnz = A->offs[n];
  M->n = n, M->ncolours = ncolours;
  M->cbeg = lsb_calloc(unsigned, (size_t)ncolours + 1);
  M->rowid = lsb_calloc(unsigned, (size_t)(n ? n : 1));
  M->offs = lsb_calloc(unsigned, (size_t)n + 1);
  M->cols = lsb_calloc(unsigned, (size_t)(nnz ? nnz : 1));
  M->vals = lsb_calloc(double, (size_t)(nnz ? nnz : 1));
  if (!M->cbeg || !M->rowid || !M->offs || !M->cols || !M->vals)
    errx(EXIT_FAILURE, "hip_cdna4: out of host memory for the colour-sorted copy of an AMG level (%u rows)", n);
  for (unsigned i = 0; i < n; i++)
    M->cbeg[colour[i] + 1]++;
  for (unsigned c = 0; c < ncolours; c++)
    M->cbeg[c + 1] += M->cbeg[c];
  unsigned *at = lsb_calloc(unsigned, (size_t)ncolours + 1);
  memcpy(at, M->cbeg, ((size_t)ncolours + 1) * sizeof(unsigned));
  for (unsigned i = 0; i < n; i++)
    M->rowid[at[colour[i]]++] = i;
  free(at);
  for (unsigned p = 0; p < n; p++) {
    const unsigned i = M->rowid[p], len = A->offs[i + 1] - A->offs[i];
    unsigned w = M->offs[p];
    for (unsigned e = A->offs[i]; e < A->offs[i + 1]; e++, w++)
      M->cols[w] = A->cols[e] - base, M->vals[w] = A->vals[e];
    M->offs[p + 1] = M->offs[p] + len;
  }
  return M;
}

void lsb_mcgs_free(struct lsb_mcgs *M) {
  if (!M)
    return;
  free(M->cbeg), free(M->rowid), free(M->offs), free(M->cols), free(M->vals), free(M);
}

/* What k_amg_mcgs relies on to update x in place without a race, asserted on the host at every upload: 0, or the
 * number of the violated rule and its text in why[whylen]. */
int lsb_mcgs_check(const struct csr *A, const int *colour, const struct lsb_mcgs *M, char *why, size_t whylen) {
#define MCGS_FAIL(code, ...)                 \
  do {                                       \
    if (why && whylen)                       \
      snprintf(why, whylen, __VA_ARGS__);    \
    free(seen);                              \
    return code;                             \
  } while (0)
  unsigned char *seen = NULL;
  if (!A || !colour || !M || !M->cbeg || !M->rowid || !M->offs || !M->cols || !M->vals)
    MCGS_FAIL(1, "rule 1: a matrix, a colouring and a copy with all its arrays");
  const unsigned n = A->nrows, base = A->base;
  if (M->n != n || M->cbeg[0] != 0 || M->cbeg[M->ncolours] != n)
    MCGS_FAIL(2, "rule 2: the colour ranges cover positions 0 .. n: cbeg[0] = 0, cbeg[ncolours] = n = %u", n);
  for (unsigned c = 0; c < M->ncolours; c++)
    if (M->cbeg[c] > M->cbeg[c + 1])
      MCGS_FAIL(2, "rule 2: the colour ranges ascend (cbeg[%u] = %u > cbeg[%u] = %u)", c, M->cbeg[c], c + 1,
                M->cbeg[c + 1]);
  seen = (unsigned char *)calloc((size_t)n + 1, 1);
  if (!seen)
    MCGS_FAIL(1, "rule 1: out of host memory");
  /* rowid is a permutation, and every row sits in the range of its own colour: in exactly one range */
  for (unsigned c = 0; c < M->ncolours; c++)
    for (unsigned p = M->cbeg[c]; p < M->cbeg[c + 1]; p++) {
      const unsigned i = M->rowid[p];
      if (i >= n || seen[i])
        MCGS_FAIL(3, "rule 3: rowid is a permutation of the rows (position %u holds row %u %s)", p, i,
                  i >= n ? "of no such row" : "a second time");
      seen[i] = 1;
      if (colour[i] != (int)c)
        MCGS_FAIL(4, "rule 4: a row is in the range of its colour (row %u of colour %d at position %u, in the range "
                     "of colour %u)", i, colour[i], p, c);
    }
  for (unsigned i = 0; i < n; i++) {
    double d = 0.0;
    for (unsigned e = A->offs[i]; e < A->offs[i + 1]; e++) {
      const unsigned j = A->cols[e] - base;
      if (j >= n)
        MCGS_FAIL(5, "rule 5: every column is a row of the level (row %u has column %u of %u)", i, j, n);
      if (j == i)
        d += A->vals[e];
      else if (colour[j] == colour[i])
        MCGS_FAIL(6, "rule 6: rows coupled by a stored entry have different colours (a[%u][%u] is stored, both rows "
                     "have colour %d)", i, j, colour[i]);
    }
    if (!(d > 0.0))
      MCGS_FAIL(7, "rule 7: every diagonal is > 0 (row %u has %g)", i, d);
  }
  /* the copy's rows are the original rows, entry for entry */
  if (M->offs[0] != 0)
    MCGS_FAIL(8, "rule 8: the copy's offsets start at 0");
  for (unsigned p = 0; p < n; p++) {
    const unsigned i = M->rowid[p], len = A->offs[i + 1] - A->offs[i];
    if (M->offs[p + 1] < M->offs[p] || M->offs[p + 1] - M->offs[p] != len || M->offs[p + 1] > A->offs[n])
      MCGS_FAIL(8, "rule 8: position %u of the copy has the length of row %u (%u entries)", p, i, len);
    for (unsigned k = 0; k < len; k++) {
      const unsigned e = A->offs[i] + k, w = M->offs[p] + k;
      if (M->cols[w] != A->cols[e] - base || memcmp(&M->vals[w], &A->vals[e], sizeof(double)) != 0)
        MCGS_FAIL(8, "rule 8: the copy's rows are the original rows entry for entry (entry %u of row %u differs)", k,
                  i);
    }
  }
  free(seen);
  return 0;
#undef MCGS_FAIL
}
