/*
 * ORACLE -- TEST INFRASTRUCTURE ONLY.  Not part of the product.
 *
 * A plain-C CPU restatement of the lsbench hot path that the HIP backend
 * (lsbench_amd/csrc) is checked against.  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load this file's library; the product
 * never does and has no CPU fallback.
 *
 * What is restated, and from where (all paths under /root/reference):
 *   - text matrix -> CSR ............ src/lsbench-csr.c:29-92
 *   - matrix print .................. src/lsbench-csr.c:94-99
 *   - right-hand side / x0 .......... src/lsbench.c:157-160   (b_i = i, x0 = 0)
 *   - operator CHOLMOD factorises ... src/cholmod-impl.h:5-21 (upper triangle
 *                                     kept, stype=-1 mirrors it: S =
 *                                     triu(A)+triu(A,1)^T)
 * What has NO reference source (it lives inside third-party libraries that are
 * fetched at configure time, libs/suitesparse.cmake:8-10, libs/ginkgo.cmake:4-5,
 * none of them present offline) and is therefore restated from the textbook:
 *   - CSR SpMV, dot, Jacobi-preconditioned CG.
 *
 * PARITY PINNING.  Loader: pinned against the reference's own loader compiled
 * from its sources (oracle/Makefile -> oracle/_ref/, tests/test_oracle_ref.py)
 * and against the committed print-outs in tests/golden/.  Solve: the reference
 * holds no expected solutions and its solver (SuiteSparse CHOLMOD v7.0.1) is
 * not in /root/reference nor installable, so there is no reference output to
 * pin against: "parity unpinned" by reference fixtures.  It is pinned instead
 * by the mathematical definition x = S^-1 b on the reference's tests/ matrices
 * through (i) exact known answers for tests/{I1_05x05,A0_02x02,A1_02x02}.txt,
 * (ii) golden vectors from two independent direct solvers (LAPACK dense
 * Cholesky and SuperLU, oracle/make_golden.py) that agree to <= 2e-14, and
 * (iii) the residual ||b - S x||.
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

typedef struct {
  uint32_t nrows, base;
  uint32_t *offs, *cols;
  double *vals;
} orc_csr;

/* ---------------------------------------------------------------------- */
/* Loader: follows src/lsbench-csr.c:29-92 step by step.                    */
/* ---------------------------------------------------------------------- */

typedef struct {
  uint32_t r, c;
  double v;
} orc_trip;

static int orc_trip_cmp(const void *pa, const void *pb) {
  const orc_trip *a = (const orc_trip *)pa, *b = (const orc_trip *)pb;
  if (a->r != b->r)
    return a->r < b->r ? -1 : 1; /* rows first: src/lsbench-csr.c:16-19 */
  if (a->c != b->c)
    return a->c < b->c ? -1 : 1; /* then columns: :21-24 */
  return 0;
}

/* Returns NULL and fills err[] instead of exiting, so tests can assert on the
 * failure modes of src/lsbench-csr.c:31-32,38-43,51-52. */
orc_csr *orc_matrix_read(const char *fname, char *err, int errlen) {
  FILE *fp = fopen(fname, "r");
  if (!fp) {
    snprintf(err, errlen, "open");
    return NULL;
  }
  unsigned nnz, base;
  char ch;
  int ret = fscanf(fp, "%u %u%c", &nnz, &base, &ch); /* :37 */
  if (ret != 3 || (ch != '\n' && ch != EOF)) {
    snprintf(err, errlen, "meta");
    fclose(fp);
    return NULL;
  }
  if (base > 1) { /* :40-41 */
    snprintf(err, errlen, "base");
    fclose(fp);
    return NULL;
  }
  if (nnz == 0) { /* :42-43 */
    snprintf(err, errlen, "nnz0");
    fclose(fp);
    return NULL;
  }
  orc_trip *t = (orc_trip *)calloc(nnz, sizeof *t);
  for (unsigned i = 0; i < nnz; i++) {
    ret = fscanf(fp, "%u %u %lf%c", &t[i].r, &t[i].c, &t[i].v, &ch); /* :50 */
    if (ret != 4 || (ch != '\n' && ch != EOF)) {
      snprintf(err, errlen, "entries");
      free(t);
      fclose(fp);
      return NULL;
    }
  }
  fclose(fp);
  qsort(t, nnz, sizeof *t, orc_trip_cmp); /* :54 */

  /* Sum repeated (r,c) and compress in place: :57-63. */
  unsigned m = 0, s = 0;
  while (s < nnz) {
    unsigned e = s + 1;
    t[m] = t[s];
    while (e < nnz && t[e].r == t[s].r && t[e].c == t[s].c)
      t[m].v += t[e].v, e++;
    s = e, m++;
  }

  /* nrows = number of distinct row ids present: :66-70 (rows are renumbered
   * densely, column ids are kept verbatim). */
  unsigned nrows = 1;
  for (unsigned i = 1; i < m; i++)
    nrows += (t[i].r != t[i - 1].r);

  orc_csr *A = (orc_csr *)calloc(1, sizeof *A);
  A->nrows = nrows, A->base = base;
  A->offs = (uint32_t *)calloc((size_t)nrows + 1, sizeof(uint32_t));
  A->cols = (uint32_t *)calloc(m, sizeof(uint32_t));
  A->vals = (double *)calloc(m, sizeof(double));
  unsigned row = 0;
  for (unsigned i = 0; i < m; i++) { /* :79-86 */
    if (i > 0 && t[i].r != t[i - 1].r)
      A->offs[++row] = i;
    A->cols[i] = t[i].c, A->vals[i] = t[i].v;
  }
  A->offs[nrows] = m;
  free(t);
  return A;
}

void orc_csr_free(orc_csr *A) {
  if (!A)
    return;
  free(A->offs), free(A->cols), free(A->vals), free(A);
}

void orc_csr_dims(const orc_csr *A, uint32_t *nrows, uint32_t *base,
                  uint32_t *nnz) {
  *nrows = A->nrows, *base = A->base, *nnz = A->offs[A->nrows];
}

void orc_csr_export(const orc_csr *A, uint32_t *offs, uint32_t *cols,
                    double *vals) {
  uint32_t nnz = A->offs[A->nrows];
  memcpy(offs, A->offs, ((size_t)A->nrows + 1) * sizeof(uint32_t));
  memcpy(cols, A->cols, (size_t)nnz * sizeof(uint32_t));
  memcpy(vals, A->vals, (size_t)nnz * sizeof(double));
}

/* src/lsbench-csr.c:94-99: "row+base col(as stored) %lf". */
int orc_matrix_print_file(const orc_csr *A, const char *path) {
  FILE *fp = fopen(path, "w");
  if (!fp)
    return 1;
  for (uint32_t i = 0; i < A->nrows; i++)
    for (uint32_t j = A->offs[i]; j < A->offs[i + 1]; j++)
      fprintf(fp, "%u %u %lf\n", i + A->base, A->cols[j], A->vals[j]);
  fclose(fp);
  return 0;
}

/* ---------------------------------------------------------------------- */
/* Operator: src/cholmod-impl.h:5-21.  Per row i keep the entries with       */
/* col-base >= i as triplets (i, col-base, v) of a stype=-1 symmetric matrix, */
/* i.e. each kept off-diagonal entry also appears transposed.                 */
/* Output: full CSR of S, 0-based, sorted.  Arrays are caller-allocated with  */
/* capacity 2*nnz(A); returns nnz(S).                                         */
/* ---------------------------------------------------------------------- */
uint32_t orc_operator_upper(uint32_t n, uint32_t base, const uint32_t *offs,
                            const uint32_t *cols, const double *vals,
                            uint32_t *s_offs, uint32_t *s_cols,
                            double *s_vals) {
  uint32_t nnz = offs[n];
  orc_trip *t = (orc_trip *)malloc((size_t)2 * nnz * sizeof *t + 16);
  size_t z = 0;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t j = offs[i], je = offs[i + 1];
    /* :13-14 skips the strictly-lower part (bounded here by the row end; the
     * reference scans unbounded and relies on a stored diagonal). */
    while (j < je && cols[j] - base < i)
      j++;
    for (; j < je; j++) { /* :15-16 */
      uint32_t c = cols[j] - base;
      t[z].r = i, t[z].c = c, t[z].v = vals[j], z++;
      if (c != i) /* stype = -1 (:6): mirror into the other triangle */
        t[z].r = c, t[z].c = i, t[z].v = vals[j], z++;
    }
  }
  qsort(t, z, sizeof *t, orc_trip_cmp);
  memset(s_offs, 0, ((size_t)n + 1) * sizeof(uint32_t));
  for (size_t k = 0; k < z; k++) {
    s_offs[t[k].r + 1]++;
    s_cols[k] = t[k].c, s_vals[k] = t[k].v;
  }
  for (uint32_t i = 0; i < n; i++)
    s_offs[i + 1] += s_offs[i];
  free(t);
  return (uint32_t)z;
}

/* ---------------------------------------------------------------------- */
/* Textbook kernels (no reference source; see header).                      */
/* 64-bit offsets so the 447 M-nnz configuration fits.                       */
/* ---------------------------------------------------------------------- */

static int g_threads = 1;
void orc_set_threads(int t) {
  g_threads = t < 1 ? 1 : t;
#ifdef _OPENMP
  omp_set_num_threads(g_threads);
#endif
}
int orc_get_max_threads(void) {
#ifdef _OPENMP
  return omp_get_num_procs();
#else
  return 1;
#endif
}

/* y = A x, rows summed left to right in stored (column) order. */
void orc_spmv(uint64_t n, const uint64_t *offs, const uint32_t *cols,
              const double *vals, const double *x, double *y) {
#pragma omp parallel for schedule(static) if (g_threads > 1)
  for (int64_t i = 0; i < (int64_t)n; i++) {
    double s = 0.0;
    for (uint64_t j = offs[i]; j < offs[i + 1]; j++)
      s += vals[j] * x[cols[j]];
    y[i] = s;
  }
}

/* 32-bit-offset flavour for CSR straight out of the loader. */
void orc_spmv32(uint32_t n, const uint32_t *offs, const uint32_t *cols,
                const double *vals, const double *x, double *y) {
  for (uint32_t i = 0; i < n; i++) {
    double s = 0.0;
    for (uint32_t j = offs[i]; j < offs[i + 1]; j++)
      s += vals[j] * x[cols[j]];
    y[i] = s;
  }
}

static double orc_dot(uint64_t n, const double *a, const double *b) {
  double s = 0.0;
#pragma omp parallel for reduction(+ : s) schedule(static) if (g_threads > 1)
  for (int64_t i = 0; i < (int64_t)n; i++)
    s += a[i] * b[i];
  return s;
}

/*
 * Jacobi-preconditioned conjugate gradients, x0 = 0.
 *   r = b; z = D^-1 r; p = z; rz = r.z; bb = b.b
 *   repeat: q = A p; alpha = rz / p.q; x += alpha p; r -= alpha q;
 *           z = D^-1 r; rz' = r.z; rr = r.r;
 *           stop if rr <= tol^2 bb; beta = rz'/rz; p = z + beta p
 * Stop test on the recurrence residual, counted in whole iterations -- the
 * HIP driver (lsbench_amd/csrc/hip_cdna4.c) uses exactly these rules.
 * status: 1 converged, 2 breakdown (p.q == 0 or not finite), 3 maxit.
 * max_iter_only > 0 forces exactly that many iterations unless converged
 * first with tol; use tol = 0 for a fixed-work run.
 */
int orc_pcg_jacobi(uint64_t n, const uint64_t *offs, const uint32_t *cols,
                   const double *vals, const double *b, double *x, double tol,
                   uint32_t maxit, int use_jacobi, uint32_t *iters_out,
                   double *relres_out) {
  double *r = (double *)malloc(n * sizeof(double));
  double *p = (double *)malloc(n * sizeof(double));
  double *q = (double *)malloc(n * sizeof(double));
  double *dinv = (double *)malloc(n * sizeof(double));
  int status = 3;
  uint32_t it = 0;

#pragma omp parallel for schedule(static) if (g_threads > 1)
  for (int64_t i = 0; i < (int64_t)n; i++) {
    double d = 0.0;
    for (uint64_t j = offs[i]; j < offs[i + 1]; j++)
      if (use_jacobi == 2) /* l1-Jacobi: the row's absolute sum, in column order */
        d += fabs(vals[j]);
      else if (cols[j] == (uint64_t)i)
        d = vals[j];
    dinv[i] = (use_jacobi && d != 0.0) ? 1.0 / d : (use_jacobi ? 0.0 : 1.0);
  }
  double rz = 0.0, bb = 0.0;
#pragma omp parallel for reduction(+ : rz, bb) schedule(static) if (g_threads > 1)
  for (int64_t i = 0; i < (int64_t)n; i++) {
    x[i] = 0.0;
    r[i] = b[i];
    p[i] = dinv[i] * b[i];
    rz += b[i] * p[i];
    bb += b[i] * b[i];
  }
  double rr = bb;
  const double thresh2 = tol * tol * bb;
  if (bb == 0.0) {
    status = 1;
    goto done;
  }
  while (it < maxit) {
    orc_spmv(n, offs, cols, vals, p, q);
    double pq = orc_dot(n, p, q);
    if (!(pq != 0.0) || !isfinite(pq)) {
      status = 2;
      break;
    }
    double alpha = rz / pq, rz_new = 0.0;
    rr = 0.0;
#pragma omp parallel for reduction(+ : rz_new, rr) schedule(static) if (g_threads > 1)
    for (int64_t i = 0; i < (int64_t)n; i++) {
      x[i] += alpha * p[i];
      double ri = r[i] - alpha * q[i];
      r[i] = ri;
      rz_new += ri * (dinv[i] * ri);
      rr += ri * ri;
    }
    it++;
    if (rr <= thresh2) {
      status = 1;
      break;
    }
    double beta = rz_new / rz;
    rz = rz_new;
#pragma omp parallel for schedule(static) if (g_threads > 1)
    for (int64_t i = 0; i < (int64_t)n; i++)
      p[i] = dinv[i] * r[i] + beta * p[i];
  }
done:
  *iters_out = it;
  *relres_out = bb > 0.0 ? sqrt(rr / bb) : 0.0;
  free(r), free(p), free(q), free(dinv);
  return status;
}

/*
 * PCG with a preconditioner applied as a vector operation z = M^-1 r -- textbook
 * restatement of what lsbench_amd/csrc/hip_precond.c enqueues (no reference
 * source: the nearest statements are the smoother set-ups of src/hypre.c:126-158,
 * src/amgx.c:78-85 and the Jacobi preconditioner of src/ginkgo.cpp:57-58).
 *   kind 3  Chebyshev polynomial of degree m = `param` in D^-1 A on [lmax / max(30, 16 m^2), lmax],
 *           lmax = 1.1 x the estimate of 20 power iterations from the start vector
 *           v_i = 1 + ((7919 i) mod 1024) / 1024:
 *              theta = (lmax+lmin)/2, delta = (lmax-lmin)/2, sigma = theta/delta, rho = 1/sigma
 *              d = D^-1 r / theta ; z = d
 *              k = 1..param: rho' = 1/(2 sigma - rho)
 *                            d = rho' rho d + (2 rho'/delta) D^-1 (r - A z) ; z += d ; rho = rho'
 *   kind 4  block-Jacobi: z_B = A_BB^-1 r_B for blocks B of `param` consecutive rows
 *           (the last one shorter), each solved by a dense Cholesky factorisation
 *           -- a different algorithm from the product's in-place Gauss-Jordan inverse.
 * Recurrences and stop rule as orc_pcg_jacobi.  *spmv_out counts A-multiplications.
 */
static void orc_chol_blocks(uint64_t n, uint32_t bs, const uint64_t *offs, const uint32_t *cols,
                            const double *vals, double *L) {
  for (uint64_t b0 = 0, k = 0; b0 < n; b0 += bs, k++) {
    const uint32_t m = (uint32_t)(n - b0 < bs ? n - b0 : bs);
    double *B = L + k * (uint64_t)bs * bs;
    for (uint32_t i = 0; i < m; i++)
      for (uint64_t j = offs[b0 + i]; j < offs[b0 + i + 1]; j++)
        if (cols[j] >= b0 && cols[j] < b0 + m)
          B[(uint64_t)i * m + (cols[j] - b0)] = vals[j];
    for (uint32_t j = 0; j < m; j++) { /* B = L L^T, lower triangle in place */
      double d = B[(uint64_t)j * m + j];
      for (uint32_t t = 0; t < j; t++)
        d -= B[(uint64_t)j * m + t] * B[(uint64_t)j * m + t];
      d = sqrt(d);
      B[(uint64_t)j * m + j] = d;
      for (uint32_t i = j + 1; i < m; i++) {
        double v = B[(uint64_t)i * m + j];
        for (uint32_t t = 0; t < j; t++)
          v -= B[(uint64_t)i * m + t] * B[(uint64_t)j * m + t];
        B[(uint64_t)i * m + j] = v / d;
      }
    }
  }
}

static void orc_chol_solve(uint64_t n, uint32_t bs, const double *L, const double *r, double *z) {
  for (uint64_t b0 = 0, k = 0; b0 < n; b0 += bs, k++) {
    const uint32_t m = (uint32_t)(n - b0 < bs ? n - b0 : bs);
    const double *B = L + k * (uint64_t)bs * bs;
    double *y = z + b0;
    for (uint32_t i = 0; i < m; i++) { /* L y = r */
      double v = r[b0 + i];
      for (uint32_t t = 0; t < i; t++)
        v -= B[(uint64_t)i * m + t] * y[t];
      y[i] = v / B[(uint64_t)i * m + i];
    }
    for (uint32_t ii = m; ii-- > 0;) { /* L^T z = y */
      double v = y[ii];
      for (uint32_t t = ii + 1; t < m; t++)
        v -= B[(uint64_t)t * m + ii] * y[t];
      y[ii] = v / B[(uint64_t)ii * m + ii];
    }
  }
}

/* FSAI (kind 5 of orc_pcg_prec; the product: lsb_csr_fsai_pattern + hip_fsai.hip), restated
 * from the definition: row i of G lives on J = {j <= i reached from i in `power` hops of S's
 * graph (stored pattern, both triangles)}, the 128 largest where there are more, and is
 * y / sqrt(y_last) with S[J, J] y = e_last.  The local systems are solved by Gaussian
 * elimination with partial pivoting on a dense copy (the product uses a Cholesky
 * factorisation in LDS); the pattern is found by a breadth-first sweep with a visited array
 * per row (the product: stamps + a shell sort).  goffs[n+1], gcols/gvals: caller frees. */
static int orc_cmp_u32(const void *a, const void *b) {
  const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
  return x < y ? -1 : x > y;
}
static void orc_fsai_build(uint64_t n, const uint64_t *offs, const uint32_t *cols, const double *vals,
                           uint32_t power, uint64_t **goffs_out, uint32_t **gcols_out, double **gvals_out) {
  const uint32_t cap = 128;
  uint64_t *goffs = (uint64_t *)calloc(n + 1, sizeof(uint64_t));
  uint64_t capn = 16 * n + 16, used = 0;
  uint32_t *gcols = (uint32_t *)malloc(capn * sizeof(uint32_t));
  double *gvals = (double *)malloc(capn * sizeof(double));
  unsigned char *seen = (unsigned char *)calloc(n, 1);
  uint32_t *front = (uint32_t *)malloc(n * sizeof(uint32_t)), *J = (uint32_t *)malloc(n * sizeof(uint32_t));
  double *A = (double *)malloc((size_t)cap * cap * sizeof(double)), *y = (double *)malloc(cap * sizeof(double));
  for (uint64_t i = 0; i < n; i++) {
    /* breadth first, `power` levels */
    uint64_t nf = 0, lo = 0;
    front[nf++] = (uint32_t)i, seen[i] = 1;
    for (uint32_t lev = 0; lev < power; lev++) {
      const uint64_t hi = nf;
      for (uint64_t a = lo; a < hi; a++)
        for (uint64_t e = offs[front[a]]; e < offs[front[a] + 1]; e++)
          if (cols[e] < n && !seen[cols[e]])
            seen[cols[e]] = 1, front[nf++] = cols[e];
      lo = hi;
    }
    uint64_t m = 0;
    for (uint64_t a = 0; a < nf; a++) {
      seen[front[a]] = 0;
      if (front[a] <= i)
        J[m++] = front[a];
    }
    qsort(J, m, sizeof(uint32_t), orc_cmp_u32);
    const uint32_t *Jk = J + (m > cap ? m - cap : 0);
    const uint32_t mk = (uint32_t)(m > cap ? cap : m);
    /* dense S[J, J] (both triangles), right-hand side e_last */
    for (uint32_t a = 0; a < mk; a++) {
      for (uint32_t b = 0; b < mk; b++)
        A[(size_t)a * mk + b] = 0.0;
      for (uint64_t e = offs[Jk[a]]; e < offs[Jk[a] + 1]; e++) {
        const uint32_t *hit = (const uint32_t *)bsearch(&cols[e], Jk, mk, sizeof(uint32_t), orc_cmp_u32);
        if (hit)
          A[(size_t)a * mk + (size_t)(hit - Jk)] = vals[e];
      }
      y[a] = a + 1 == mk ? 1.0 : 0.0;
    }
    for (uint32_t k = 0; k < mk; k++) { /* elimination with partial pivoting */
      uint32_t piv = k;
      for (uint32_t a = k + 1; a < mk; a++)
        if (fabs(A[(size_t)a * mk + k]) > fabs(A[(size_t)piv * mk + k]))
          piv = a;
      if (piv != k) {
        for (uint32_t b = 0; b < mk; b++) {
          const double t = A[(size_t)k * mk + b];
          A[(size_t)k * mk + b] = A[(size_t)piv * mk + b], A[(size_t)piv * mk + b] = t;
        }
        const double t = y[k];
        y[k] = y[piv], y[piv] = t;
      }
      for (uint32_t a = k + 1; a < mk; a++) {
        const double f = A[(size_t)a * mk + k] / A[(size_t)k * mk + k];
        if (f != 0.0) {
          for (uint32_t b = k; b < mk; b++)
            A[(size_t)a * mk + b] -= f * A[(size_t)k * mk + b];
          y[a] -= f * y[k];
        }
      }
    }
    for (uint32_t k = mk; k-- > 0;) {
      double t = y[k];
      for (uint32_t b = k + 1; b < mk; b++)
        t -= A[(size_t)k * mk + b] * y[b];
      y[k] = t / A[(size_t)k * mk + k];
    }
    const double sc = 1.0 / sqrt(y[mk - 1]);
    if (used + mk > capn) {
      capn = 2 * capn + mk;
      gcols = (uint32_t *)realloc(gcols, capn * sizeof(uint32_t));
      gvals = (double *)realloc(gvals, capn * sizeof(double));
    }
    goffs[i] = used;
    for (uint32_t a = 0; a < mk; a++)
      gcols[used] = Jk[a], gvals[used++] = y[a] * sc;
  }
  goffs[n] = used;
  free(seen), free(front), free(J), free(A), free(y);
  *goffs_out = goffs, *gcols_out = gcols, *gvals_out = gvals;
}

int orc_pcg_prec(uint64_t n, const uint64_t *offs, const uint32_t *cols, const double *vals,
                 const double *b, double *x, double tol, uint32_t maxit, int kind, uint32_t param,
                 uint32_t *iters_out, double *relres_out, uint32_t *spmv_out, double *lmax_out) {
  double *r = (double *)malloc(n * sizeof(double)), *p = (double *)malloc(n * sizeof(double));
  double *q = (double *)malloc(n * sizeof(double)), *z = (double *)malloc(n * sizeof(double));
  double *d = (double *)calloc(n, sizeof(double)), *dinv = (double *)malloc(n * sizeof(double));
  double *L = NULL, *gvals = NULL;
  uint64_t *goffs = NULL;
  uint32_t *gcols = NULL;
  uint32_t it = 0, nspmv = 0;
  int status = 3;
  double lmax = 0.0, theta = 0.0, delta = 0.0, sigma = 0.0;
  for (uint64_t i = 0; i < n; i++) {
    double dd = 0.0;
    for (uint64_t j = offs[i]; j < offs[i + 1]; j++)
      if (cols[j] == i)
        dd = vals[j];
    dinv[i] = dd != 0.0 ? 1.0 / dd : 0.0;
  }
  if (kind == 3) {
    double vv = 0.0, lam = 1.0;
    for (uint64_t i = 0; i < n; i++) {
      z[i] = 1.0 + (double)(((uint32_t)i * 7919u) % 1024u) / 1024.0;
      vv += z[i] * z[i];
    }
    for (int k = 0; k < 20; k++) {
      orc_spmv(n, offs, cols, vals, z, q);
      double ww = 0.0;
      for (uint64_t i = 0; i < n; i++) {
        q[i] *= dinv[i];
        ww += q[i] * q[i];
      }
      if (!(ww > 0.0) || !(vv > 0.0))
        break;
      lam = sqrt(ww / vv);
      const double c = 1.0 / sqrt(ww);
      for (uint64_t i = 0; i < n; i++)
        z[i] = c * q[i];
      vv = 1.0;
    }
    lmax = 1.1 * lam;
    /* the interval grows with the degree: lmax / max(30, 16 m^2) (see hip_precond.c) */
    const double ratio = 16.0 * param * param > 30.0 ? 16.0 * param * param : 30.0;
    const double lmin = lmax / ratio;
    theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
  } else if (kind == 4) {
    const uint64_t nb = (n + param - 1) / param;
    L = (double *)calloc(nb * (uint64_t)param * param, sizeof(double));
    orc_chol_blocks(n, param, offs, cols, vals, L);
  } else if (kind == 5) {
    orc_fsai_build(n, offs, cols, vals, param, &goffs, &gcols, &gvals);
  }
#define ORC_PREC()                                                                       \
  do {                                                                                   \
    if (kind == 5) { /* z = G^T (G r): t by rows, z by scattering rows of G */          \
      for (uint64_t i = 0; i < n; i++) {                                                 \
        double t = 0.0;                                                                  \
        for (uint64_t e = goffs[i]; e < goffs[i + 1]; e++)                               \
          t += gvals[e] * r[gcols[e]];                                                   \
        d[i] = t, z[i] = 0.0;                                                            \
      }                                                                                  \
      for (uint64_t i = 0; i < n; i++)                                                   \
        for (uint64_t e = goffs[i]; e < goffs[i + 1]; e++)                               \
          z[gcols[e]] += gvals[e] * d[i];                                                \
    } else if (kind == 4) {                                                              \
      orc_chol_solve(n, param, L, r, z);                                                 \
    } else {                                                                             \
      double rho = 1.0 / sigma;                                                          \
      for (uint64_t i = 0; i < n; i++)                                                   \
        d[i] = (1.0 / theta) * (dinv[i] * r[i]), z[i] = d[i];                            \
      for (uint32_t k = 0; k < param; k++) {                                             \
        const double rho_new = 1.0 / (2.0 * sigma - rho);                                \
        const double ca = rho_new * rho, cb = 2.0 * rho_new / delta;                     \
        orc_spmv(n, offs, cols, vals, z, q);                                             \
        nspmv++;                                                                         \
        for (uint64_t i = 0; i < n; i++) {                                               \
          d[i] = ca * d[i] + cb * (dinv[i] * (r[i] - q[i]));                             \
          z[i] += d[i];                                                                  \
        }                                                                                \
        rho = rho_new;                                                                   \
      }                                                                                  \
    }                                                                                    \
  } while (0)
  double bb = 0.0;
  for (uint64_t i = 0; i < n; i++)
    x[i] = 0.0, r[i] = b[i], bb += b[i] * b[i];
  double rr = bb, rz = 0.0;
  const double thresh2 = tol * tol * bb;
  if (bb == 0.0) {
    status = 1;
    goto done;
  }
  ORC_PREC();
  for (uint64_t i = 0; i < n; i++)
    p[i] = z[i], rz += r[i] * z[i];
  while (it < maxit) {
    orc_spmv(n, offs, cols, vals, p, q);
    nspmv++;
    const double pq = orc_dot(n, p, q);
    if (!(pq != 0.0) || !isfinite(pq)) {
      status = 2;
      break;
    }
    const double alpha = rz / pq;
    rr = 0.0;
    for (uint64_t i = 0; i < n; i++) {
      x[i] += alpha * p[i];
      r[i] -= alpha * q[i];
      rr += r[i] * r[i];
    }
    it++;
    if (rr <= thresh2) {
      status = 1;
      break;
    }
    ORC_PREC();
    double rz_new = 0.0;
    for (uint64_t i = 0; i < n; i++)
      rz_new += r[i] * z[i];
    const double beta = rz_new / rz;
    rz = rz_new;
    for (uint64_t i = 0; i < n; i++)
      p[i] = z[i] + beta * p[i];
  }
#undef ORC_PREC
done:
  *iters_out = it, *relres_out = bb > 0.0 ? sqrt(rr / bb) : 0.0, *spmv_out = nspmv;
  if (lmax_out)
    *lmax_out = lmax;
  free(r), free(p), free(q), free(z), free(d), free(dinv), free(L);
  free(goffs), free(gcols), free(gvals);
  return status;
}

/*
 * Single-reduction CG (Chronopoulos & Gear 1989), Jacobi-preconditioned,
 * x0 = 0 -- the recurrences of k_cg1_update in lsbench_amd/csrc/hip_sweeps.hip,
 * stated sequentially:
 *   r = b; u = D^-1 r; w = A u; g = r.u; d = w.u
 *   repeat: stop if r.r <= tol^2 b.b
 *           beta = g/g_old (0 first); alpha = g / (d - beta g/alpha_old) (g/d first)
 *           p = u + beta p; s = w + beta s; x += alpha p; r -= alpha s
 *           u = D^-1 r; w = A u; g_old = g; g = r.u; d = w.u
 * Same iterates as orc_pcg_jacobi in exact arithmetic.
 */
int orc_pcg1_jacobi(uint64_t n, const uint64_t *offs, const uint32_t *cols,
                    const double *vals, const double *b, double *x, double tol,
                    uint32_t maxit, uint32_t *iters_out, double *relres_out) {
  double *r = (double *)malloc(n * sizeof(double)), *u = (double *)malloc(n * sizeof(double));
  double *w = (double *)malloc(n * sizeof(double)), *p = (double *)calloc(n, sizeof(double));
  double *s = (double *)calloc(n, sizeof(double)), *dinv = (double *)malloc(n * sizeof(double));
  for (uint64_t i = 0; i < n; i++) {
    double d = 0.0;
    for (uint64_t j = offs[i]; j < offs[i + 1]; j++)
      if (cols[j] == i)
        d = vals[j];
    dinv[i] = d != 0.0 ? 1.0 / d : 0.0;
    x[i] = 0.0, r[i] = b[i], u[i] = dinv[i] * b[i];
  }
  orc_spmv(n, offs, cols, vals, u, w);
  double g = orc_dot(n, r, u), d = orc_dot(n, w, u), rr = orc_dot(n, r, r);
  const double bb = rr, thresh2 = tol * tol * bb;
  double g_old = 0.0, a_old = 0.0;
  int status = bb == 0.0 ? 1 : (maxit == 0 ? 3 : 0);
  uint32_t it = 0;
  while (status == 0) {
    if (rr <= thresh2) {
      status = 1;
      break;
    }
    double beta = 0.0, alpha;
    if (a_old == 0.0)
      alpha = g / d;
    else
      beta = g / g_old, alpha = g / (d - beta * g / a_old);
    if (!isfinite(alpha) || alpha == 0.0) {
      status = 2;
      break;
    }
    for (uint64_t i = 0; i < n; i++) {
      p[i] = u[i] + beta * p[i];
      s[i] = w[i] + beta * s[i];
      x[i] += alpha * p[i];
      r[i] -= alpha * s[i];
      u[i] = dinv[i] * r[i];
    }
    it++;
    g_old = g, a_old = alpha;
    orc_spmv(n, offs, cols, vals, u, w);
    g = orc_dot(n, r, u), d = orc_dot(n, w, u), rr = orc_dot(n, r, r);
    if (it >= maxit && rr > thresh2)
      status = 3;
  }
  *iters_out = it;
  *relres_out = bb > 0.0 ? sqrt(rr / bb) : 0.0;
  free(r), free(u), free(w), free(p), free(s), free(dinv);
  return status;
}

/*
 * Restarted GMRES(m), right Jacobi preconditioning, x0 = 0, Arnoldi by
 * classical Gram-Schmidt applied twice, Givens rotations; stop when the
 * residual estimate |g_{j+1}| <= tol*||b||, counted in inner steps -- the rules
 * of lsbench_amd/csrc/hip_gmres.hip, stated sequentially.  Textbook (Saad,
 * Iterative Methods, Alg. 6.9 + 9.5); no reference source exists.
 * status: 1 converged, 2 breakdown, 3 maxit.
 */
int orc_gmres_jacobi(uint64_t n, const uint64_t *offs, const uint32_t *cols,
                     const double *vals, const double *b, double *x, double tol,
                     uint32_t maxit, uint32_t restart, uint32_t *iters_out,
                     double *relres_out) {
  const uint32_t m = restart < 1 ? 1 : restart;
  double *V = (double *)malloc((size_t)(m + 1) * n * sizeof(double));
  double *z = (double *)malloc(n * sizeof(double));
  double *ax = (double *)calloc(n, sizeof(double));
  double *dinv = (double *)malloc(n * sizeof(double));
  double *R = (double *)calloc((size_t)m * m, sizeof(double));
  double *g = (double *)calloc(m + 1, sizeof(double));
  double *cs = (double *)calloc(m, sizeof(double)), *sn = (double *)calloc(m, sizeof(double));
  double *h = (double *)calloc(m + 2, sizeof(double)), *y = (double *)calloc(m, sizeof(double));
  for (uint64_t i = 0; i < n; i++) {
    double d = 0.0;
    for (uint64_t j = offs[i]; j < offs[i + 1]; j++)
      if (cols[j] == i)
        d = vals[j];
    dinv[i] = d != 0.0 ? 1.0 / d : 0.0;
    x[i] = 0.0;
  }
  int status = 0;
  uint32_t it = 0;
  double bnorm = 0.0, resid = 0.0, thresh = 0.0;
  for (int cycle = 0; status == 0; cycle++) {
    if (cycle > 0)
      orc_spmv(n, offs, cols, vals, x, ax);
    double rr = 0.0;
    for (uint64_t i = 0; i < n; i++) {
      V[i] = b[i] - ax[i];
      rr += V[i] * V[i];
    }
    const double beta = sqrt(rr);
    if (cycle == 0)
      bnorm = beta, thresh = tol * beta;
    resid = beta;
    if (beta <= thresh || beta == 0.0) {
      status = 1;
      break;
    }
    if (it >= maxit) {
      status = 3;
      break;
    }
    memset(g, 0, (m + 1) * sizeof(double));
    g[0] = beta;
    double hnorm = beta;
    uint32_t jlast = 0;
    for (uint32_t j = 0; j < m && status == 0; j++) {
      double *vj = V + (size_t)j * n, *w = V + (size_t)(j + 1) * n;
      for (uint64_t i = 0; i < n; i++) {
        vj[i] /= hnorm;
        z[i] = dinv[i] * vj[i];
      }
      orc_spmv(n, offs, cols, vals, z, w);
      for (uint32_t k = 0; k <= j; k++)
        h[k] = 0.0;
      for (int pass = 0; pass < 2; pass++) { /* CGS2 */
        double hp[64];
        for (uint32_t k = 0; k <= j; k++)
          hp[k] = orc_dot(n, V + (size_t)k * n, w);
        for (uint32_t k = 0; k <= j; k++) {
          const double *vk = V + (size_t)k * n;
          for (uint64_t i = 0; i < n; i++)
            w[i] -= hp[k] * vk[i];
          h[k] += hp[k];
        }
      }
      hnorm = sqrt(orc_dot(n, w, w));
      h[j + 1] = hnorm;
      for (uint32_t i = 0; i < j; i++) {
        const double t = cs[i] * h[i] + sn[i] * h[i + 1];
        h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1];
        h[i] = t;
      }
      const double a = h[j], bb = h[j + 1], d = sqrt(a * a + bb * bb);
      double c = 1.0, s = 0.0;
      if (d != 0.0)
        c = a / d, s = bb / d;
      cs[j] = c, sn[j] = s;
      h[j] = d;
      for (uint32_t i = 0; i <= j; i++)
        R[(size_t)i * m + j] = h[i];
      g[j + 1] = -s * g[j];
      g[j] = c * g[j];
      resid = fabs(g[j + 1]);
      jlast = j + 1;
      it++;
      if (d == 0.0)
        status = 2;
      else if (resid <= thresh || hnorm == 0.0)
        status = 1;
      else if (it >= maxit)
        status = 3;
    }
    for (int i = (int)jlast - 1; i >= 0; i--) {
      double s = g[i];
      for (uint32_t k = i + 1; k < jlast; k++)
        s -= R[(size_t)i * m + k] * y[k];
      y[i] = R[(size_t)i * m + i] != 0.0 ? s / R[(size_t)i * m + i] : 0.0;
    }
    for (uint64_t i = 0; i < n; i++) {
      double s = 0.0;
      for (uint32_t k = 0; k < jlast; k++)
        s += y[k] * V[(size_t)k * n + i];
      x[i] += dinv[i] * s;
    }
  }
  *iters_out = it;
  *relres_out = bnorm > 0.0 ? resid / bnorm : 0.0;
  free(V), free(z), free(ax), free(dinv), free(R), free(g), free(cs), free(sn), free(h), free(y);
  return status;
}

/* ---------------------------------------------------------------------- */
/* Synthetic operators of BASELINE.json configs 3-5, stated independently    */
/* of the product generator (lsbench_amd/csrc/lsb_synth.c).  Definitions in  */
/* DESIGN.md "Synthetic operators".  Rows [r0,r1), global 0-based columns.    */
/* Two-pass use: call with cols==NULL to get the nnz count.                   */
/* ---------------------------------------------------------------------- */

uint64_t orc_lap2d(uint64_t nx, uint64_t ny, uint64_t r0, uint64_t r1,
                   uint64_t *offs, uint32_t *cols, double *vals) {
  uint64_t z = 0;
  for (uint64_t row = r0; row < r1; row++) {
    uint64_t i = row % nx, j = row / nx; /* lexicographic: row = j*nx + i */
    if (offs)
      offs[row - r0] = z;
#define ORC_PUT(c, v)                                                          \
  do {                                                                         \
    if (cols)                                                                  \
      cols[z] = (uint32_t)(c), vals[z] = (v);                                  \
    z++;                                                                       \
  } while (0)
    if (j > 0)
      ORC_PUT(row - nx, -1.0);
    if (i > 0)
      ORC_PUT(row - 1, -1.0);
    ORC_PUT(row, 4.0);
    if (i + 1 < nx)
      ORC_PUT(row + 1, -1.0);
    if (j + 1 < ny)
      ORC_PUT(row + nx, -1.0);
  }
  if (offs)
    offs[r1 - r0] = z;
  return z;
}

uint64_t orc_lap3d(uint64_t nx, uint64_t ny, uint64_t nz, uint64_t r0,
                   uint64_t r1, uint64_t *offs, uint32_t *cols, double *vals) {
  uint64_t z = 0, nxy = nx * ny;
  for (uint64_t row = r0; row < r1; row++) {
    uint64_t i = row % nx, j = (row / nx) % ny, k = row / nxy;
    if (offs)
      offs[row - r0] = z;
    if (k > 0)
      ORC_PUT(row - nxy, -1.0);
    if (j > 0)
      ORC_PUT(row - nx, -1.0);
    if (i > 0)
      ORC_PUT(row - 1, -1.0);
    ORC_PUT(row, 6.0);
    if (i + 1 < nx)
      ORC_PUT(row + 1, -1.0);
    if (j + 1 < ny)
      ORC_PUT(row + nx, -1.0);
    if (k + 1 < nz)
      ORC_PUT(row + nxy, -1.0);
  }
  if (offs)
    offs[r1 - r0] = z;
  return z;
}

/* splitmix64 finaliser keyed by (seed, a, b): the counter-based PRNG of the
 * power-law operator. */
static uint64_t orc_mix(uint64_t seed, uint64_t a, uint64_t b) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (a + 1) +
               0xC2B2AE3D27D4EB4Full * (b + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

/* Variable-coefficient 5-/7-point operator on the lap2d / lap3d pattern
 * ("...,coef=K" of the product's generator; DESIGN.md "Synthetic operators"):
 * the stencil of -div(w grad u) with one weight per grid edge.  Directions
 * d = 0..5 are k-, j-, i-, i+, j+, k+ (2-D: d = 1..4 only).  An edge joining
 * rows a < b weighs 1/2 + (mix(K, a, b) >> 11) / 2^53; an edge leaving the
 * grid from `row` in direction d weighs 1/2 + (mix(K ^ 0x5851F42D4C957F2D,
 * row, d) >> 11) / 2^53 (Dirichlet: it only feeds the diagonal).  Entry
 * (row, neighbour) = -w, diagonal = sum of the row's weights in direction
 * order, starting from 0.  Stated from the definition with a direction table,
 * not from the product's unrolled code. */
uint64_t orc_lap_coef(uint64_t nx, uint64_t ny, uint64_t nz, int three, uint64_t K,
                      uint64_t r0, uint64_t r1, uint64_t *offs, uint32_t *cols,
                      double *vals) {
  const int64_t stride[6] = {-(int64_t)(nx * ny), -(int64_t)nx, -1, 1, (int64_t)nx,
                             (int64_t)(nx * ny)};
  uint64_t z = 0;
  for (uint64_t row = r0; row < r1; row++) {
    const uint64_t c[3] = {row % nx, (row / nx) % ny, row / (nx * ny)}; /* i, j, k */
    const uint64_t ext[3] = {nx, ny, three ? nz : 1};
    double w[6], diag = 0.0;
    int inside[6];
    for (int d = 0; d < 6; d++) {
      const int axis = d < 3 ? 2 - d : d - 3; /* k j i | i j k */
      inside[d] = d < 3 ? c[axis] > 0 : c[axis] + 1 < ext[axis];
      if (!three && axis == 2) {
        w[d] = 0.0, inside[d] = -1; /* no such direction in 2-D */
        continue;
      }
      if (inside[d]) {
        const uint64_t nb = (uint64_t)((int64_t)row + stride[d]);
        const uint64_t a = nb < row ? nb : row, b = nb < row ? row : nb;
        w[d] = 0.5 + (double)(orc_mix(K, a, b) >> 11) / 9007199254740992.0;
      } else {
        w[d] = 0.5 + (double)(orc_mix(K ^ 0x5851F42D4C957F2Dull, row, (uint64_t)d) >> 11) /
                         9007199254740992.0;
      }
      diag += w[d];
    }
    if (offs)
      offs[row - r0] = z;
    for (int d = 0; d < 3; d++)
      if (inside[d] == 1)
        ORC_PUT((uint64_t)((int64_t)row + stride[d]), -w[d]);
    ORC_PUT(row, diag);
    for (int d = 3; d < 6; d++)
      if (inside[d] == 1)
        ORC_PUT((uint64_t)((int64_t)row + stride[d]), -w[d]);
  }
  if (offs)
    offs[r1 - r0] = z;
  return z;
}

/* Row degree: inverse-CDF of a discrete power law P(d) ~ d^-gamma on
 * [1, dmax], through an integer threshold table thr[d-1] = floor(2^53 *
 * CDF(d)) that the caller passes in (it is part of the operator's
 * definition and is produced once, see orc_powerlaw_table). */
static uint32_t orc_pl_degree(const uint64_t *thr, uint32_t dmax, uint64_t u53) {
  uint32_t lo = 0, hi = dmax - 1; /* first d with u53 < thr[d-1] */
  while (lo < hi) {
    uint32_t mid = (lo + hi) / 2;
    if (u53 < thr[mid])
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo + 1;
}

/* thr[] for exponent gamma; returns the mean degree it yields. */
double orc_powerlaw_table(double gamma, uint32_t dmax, uint64_t *thr) {
  double tot = 0.0, mean = 0.0, acc = 0.0;
  for (uint32_t d = 1; d <= dmax; d++)
    tot += pow((double)d, -gamma);
  for (uint32_t d = 1; d <= dmax; d++) {
    double pd = pow((double)d, -gamma) / tot;
    acc += pd, mean += d * pd;
    double c = acc >= 1.0 ? 1.0 : acc;
    thr[d - 1] = (uint64_t)floor(c * 9007199254740992.0);
  }
  thr[dmax - 1] = 9007199254740992ull;
  return mean;
}

/* Rows [r0,r1) of the n x n power-law operator.  Row i has d_i entries; the
 * k-th (k = 0..d_i-1) sits in column floor((k*n + u_k) / d_i) with
 * u_k = mix(seed, i, 2k+1) mod (n - d_i + 1): one column per stratum, hence
 * sorted and distinct; value = 2*(mix(seed,i,2k+2) >> 11)*2^-53 - 1.
 * spd != 0: the entry nearest the diagonal stratum is replaced by (i, i) with
 * value 1 + sum|others| ... is NOT done here; see DESIGN.md (SpMV-only). */
uint64_t orc_powerlaw(uint64_t n, uint32_t dmax, const uint64_t *thr,
                      uint64_t seed, uint64_t r0, uint64_t r1, uint64_t *offs,
                      uint32_t *cols, double *vals) {
  uint64_t z = 0;
  for (uint64_t row = r0; row < r1; row++) {
    uint64_t u = orc_mix(seed, row, 0) >> 11;
    uint64_t d = orc_pl_degree(thr, dmax, u);
    if (d > n)
      d = n;
    if (offs)
      offs[row - r0] = z;
    for (uint64_t k = 0; k < d; k++) {
      if (cols) {
        uint64_t uk = orc_mix(seed, row, 2 * k + 1) % (n - d + 1);
        unsigned __int128 num = (unsigned __int128)k * n + uk;
        cols[z] = (uint32_t)(num / d);
        vals[z] =
            (double)(orc_mix(seed, row, 2 * k + 2) >> 11) * (2.0 / 9007199254740992.0) -
            1.0;
      }
      z++;
    }
  }
  if (offs)
    offs[r1 - r0] = z;
  return z;
}
