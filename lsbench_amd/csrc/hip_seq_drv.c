/*
 * Successive right-hand sides ("Successive right-hand sides"; kernels: hip_seq.hip): a solver
 * that was asked to (lsb_hip_solver_seq_begin) keeps an S-orthonormal basis of earlier solutions, starts each solve of
 * a sequence from the projection of b on it and adds the remainder it then solved for.  Everything here works in the
 * solver's internal numbering, behind the gather of a padded or re-ordered solver; the solves themselves are
 * solve_core and solve_x0_core (hip_solve.c), unchanged.
 */
#define _GNU_SOURCE
#include "hip_solver.h"

/* the scalars: [0, MAX) the projection's alpha, then the coefficients of the Gram-Schmidt passes -- beta of the dots,
 * the outputs of the first and of the second lsb_k_seq_orth (MAX + 2 each) -- and the record of lsb_k_seq_store */
enum {
  SEQ_ALPHA = 0,
  SEQ_BETA = LSB_SEQ_MAX_DEPTH,
  SEQ_OUT1 = 2 * LSB_SEQ_MAX_DEPTH,
  SEQ_OUT2 = 3 * LSB_SEQ_MAX_DEPTH + 2,
  SEQ_REC = 4 * LSB_SEQ_MAX_DEPTH + 4,
  SEQ_NSCAL = 4 * LSB_SEQ_MAX_DEPTH + 8
};

/* what the projection cannot serve: shards (the sums here are one device's), and the two unsymmetric drivers */
static int seq_serves(const lsb_hip_solver *sv) {
  return sv->nshard == 1 && !sv->dist && sv->o.krylov != LSB_KRYLOV_GMRES && sv->o.krylov != LSB_KRYLOV_BICGSTAB;
}

void seq_free(lsb_hip_solver *sv) {
  struct seq_basis *q = sv->seq;
  if (!q)
    return;
  LSB_CHK_HIP(hipStreamSynchronize(g_stream));
  for (int i = 0; q->timing && i < 4; i++)
    LSB_CHK_HIP(hipEventDestroy(q->ev[i]));
  lsb_hip_free(q->X);
  free(q);
  sv->seq = NULL;
}

int lsb_hip_solver_seq_begin(lsb_hip_solver *sv, unsigned depth) {
  if (!lsb_initialized)
    return 1;
  if (!sv || depth > LSB_SEQ_MAX_DEPTH || !seq_serves(sv))
    return 2;
  if (sv->seq && sv->seq->depth != depth)
    seq_free(sv);
  if (depth == 0)
    return 0;
  struct seq_basis *q = sv->seq;
  if (!q) {
    q = lsb_calloc(struct seq_basis, 1);
    q->depth = depth;
    q->ld = ((size_t)sv->n_here + 1) & ~(size_t)1;
    const size_t nparts = (size_t)lsb_k_seq_grid(sv->n_here) * (LSB_SEQ_MAX_DEPTH + 2);
    const size_t total = 2 * (size_t)depth * q->ld + nparts + SEQ_NSCAL;
    q->bytes = (unsigned long long)total * sizeof(double);
    q->X = (double *)lsb_hip_malloc(q->bytes);
    q->SX = q->X + (size_t)depth * q->ld;
    q->parts = q->SX + (size_t)depth * q->ld;
    q->scal = q->parts + nparts;
    LSB_CHK_HIP(hipMemsetAsync(q->X, 0, q->bytes, g_stream));
    sv->seq = q;
  }
  drain_stream(sv, "emptying the basis");
  q->held = q->restarts = 0;
  q->timed_project = q->timed_update = 0;
  return 0;
}

/* The update behind a solve that ended CONVERGED after at least one iteration.  warm: the solve ran from a projection,
 * and sv->d_x0e holds its correction e = x - x0; else d = x.  A full basis restarts on d = x. */
static void seq_update(lsb_hip_solver *sv, const double *d_x, const struct lsb_hip_result *r, int warm) {
  struct seq_basis *q = sv->seq;
  struct shard *s = &sv->sh[0];
  const unsigned n = sv->n_here;
  double rec[3] = {0.0, 0.0, 0.0}, *sc = q->scal;
  q->timed_update = 0;
  if (!(r->status == LSB_STATUS_CONVERGED && r->iters > 0 && sv->o.tol > 0.0))
    return;
  if (q->timing)
    LSB_CHK_HIP(hipEventRecord(q->ev[2], g_stream));
  x0_vecs(sv);
  double *d = sv->d_x0e, *w = s->d_q;
  const int full = q->held == q->depth;
  if (warm && !full && r->corrections > 0) {
    /* correction runs (opts.verify, mixed precision) moved x on behind e: d = x - x0, with x0 formed again from
     * the coefficients of the projection -- the same launch on the same operands, so the same bits */
    static const double minus_one = -1.0;
    LSB_CHK_HIP(hipMemcpyAsync(sc + SEQ_REC + 3, &minus_one, sizeof(double), hipMemcpyHostToDevice, g_stream));
    lsb_k_seq_combine(n, q->held, q->X, q->ld, sc + SEQ_ALPHA, sv->d_x0r, g_stream);
    LSB_CHK_HIP(hipMemcpyAsync(d, d_x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, g_stream));
    lsb_k_axpy(n, sc + SEQ_REC + 3, sv->d_x0r, d, g_stream);
  }
  if (full)
    q->held = 0, q->restarts++, warm = 0;
  const unsigned m = q->held;
  if (!warm)
    LSB_CHK_HIP(hipMemcpyAsync(d, d_x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, g_stream));
  op_exact(sv, d); /* w = S d */
  const double *nu, *nu0;
  if (m == 0) {
    unsigned np = 0;
    lsb_k_dot(n, d, w, q->parts, &np, g_stream);
    lsb_k_reduce_final(q->parts, np, 1, sc + SEQ_OUT2, 0, NULL, g_stream);
    nu = nu0 = sc + SEQ_OUT2;
  } else {
    lsb_k_seq_dots(n, m, q->X, q->ld, w, q->parts, sc + SEQ_BETA, g_stream);
    lsb_k_seq_orth(n, m, q->X, q->SX, q->ld, sc + SEQ_BETA, d, w, q->parts, sc + SEQ_OUT1, g_stream);
    lsb_k_seq_orth(n, m, q->X, q->SX, q->ld, sc + SEQ_OUT1, d, w, q->parts, sc + SEQ_OUT2, g_stream);
    nu = sc + SEQ_OUT2 + m, nu0 = sc + SEQ_OUT1 + m + 1;
  }
  lsb_k_seq_store(n, d, w, q->X + (size_t)m * q->ld, q->SX + (size_t)m * q->ld, nu, nu0, sc + SEQ_REC, g_stream);
  if (q->timing)
    LSB_CHK_HIP(hipEventRecord(q->ev[3], g_stream));
  LSB_CHK_HIP(hipMemcpyAsync(rec, sc + SEQ_REC, sizeof rec, hipMemcpyDeviceToHost, g_stream));
  drain_stream(sv, "the basis update");
  q->timed_update = q->timing;
  if (rec[2] != 0.0)
    q->held++;
}

/* one solve of a sequence on b and x in the solver's numbering */
static int seq_core(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res) {
  struct seq_basis *q = sv->seq;
  struct lsb_hip_result r;
  const int warm = q->held > 0;
  int rc;
  q->timed_project = 0;
  if (!warm)
    rc = solve_core(sv, d_b, d_x, &r);
  else {
    if (q->timing)
      LSB_CHK_HIP(hipEventRecord(q->ev[0], g_stream));
    lsb_k_seq_dots(sv->n_here, q->held, q->X, q->ld, d_b, q->parts, q->scal + SEQ_ALPHA, g_stream);
    lsb_k_seq_combine(sv->n_here, q->held, q->X, q->ld, q->scal + SEQ_ALPHA, d_x, g_stream);
    if (q->timing)
      LSB_CHK_HIP(hipEventRecord(q->ev[1], g_stream));
    q->timed_project = q->timing;
    rc = solve_x0_core(sv, d_b, d_x, &r);
  }
  if (rc == 0)
    seq_update(sv, d_x, &r, warm);
  if (res)
    *res = r;
  return rc;
}

/* ... in the caller's (solve_user_dev's rule, hip_solve.c; the x0 is not the caller's, so x is always written) */
static int seq_user_dev(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res) {
  if (!sv->d_perm)
    return seq_core(sv, d_b, d_x, res);
  lsb_k_perm_gather(sv->n_here, sv->d_perm, d_b, sv->d_bp, g_stream);
  const int rc = seq_core(sv, sv->d_bp, sv->d_xp, res);
  lsb_k_perm_scatter(sv->n_here, sv->d_perm, sv->d_xp, d_x, g_stream);
  drain_stream(sv, "un-permuting x");
  return rc;
}

int lsb_hip_solver_solve_seq_dev(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (!sv || !d_b || !d_x || !sv->seq)
    return 2;
  return seq_user_dev(sv, d_b, d_x, res);
}

int lsb_hip_solver_solve_seq(lsb_hip_solver *sv, const double *b, double *x, struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (!sv || !b || !x || !sv->seq)
    return 2;
  const size_t bytes = (size_t)sv->n_user * sizeof(double);
  double *d_b = (double *)lsb_hip_malloc(bytes), *d_x = (double *)lsb_hip_malloc(bytes);
  LSB_CHK_HIP(hipMemcpy(d_b, b, bytes, hipMemcpyHostToDevice));
  const int rc = seq_user_dev(sv, d_b, d_x, res);
  LSB_CHK_HIP(hipMemcpy(x, d_x, bytes, hipMemcpyDeviceToHost));
  /* cached graphs must not outlive the buffers they were captured with */
  drop_graphs(sv);
  lsb_hip_free(d_b), lsb_hip_free(d_x);
  return rc;
}

int lsb_hip_solver_seq_info(const lsb_hip_solver *sv, unsigned *depth, unsigned *held, unsigned *restarts,
                            unsigned long long *bytes) {
  if (!sv)
    return 2;
  const struct seq_basis *q = sv->seq;
  if (depth)
    *depth = q ? q->depth : 0;
  if (held)
    *held = q ? q->held : 0;
  if (restarts)
    *restarts = q ? q->restarts : 0;
  if (bytes)
    *bytes = q ? q->bytes : 0;
  return 0;
}

int lsb_hip_solver_seq_basis_dev(lsb_hip_solver *sv, unsigned k, double *d_xk, double *d_sxk) {
  if (!lsb_initialized)
    return 1;
  if (!sv || !sv->seq || k >= sv->seq->held)
    return 2;
  const struct seq_basis *q = sv->seq;
  const double *src[2] = {q->X + (size_t)k * q->ld, q->SX + (size_t)k * q->ld};
  double *dst[2] = {d_xk, d_sxk};
  for (int i = 0; i < 2; i++) {
    if (!dst[i])
      continue;
    if (sv->d_perm)
      lsb_k_perm_scatter(sv->n_here, sv->d_perm, src[i], dst[i], g_stream);
    else
      LSB_CHK_HIP(hipMemcpyAsync(dst[i], src[i], (size_t)sv->n_here * sizeof(double), hipMemcpyDeviceToDevice,
                                 g_stream));
  }
  drain_stream(sv, "reading the basis");
  return 0;
}

/* The first call on a basis makes the four events and turns their recording on: a sequence nobody times records none */
int lsb_hip_solver_seq_last_us(lsb_hip_solver *sv, double *project_us, double *update_us) {
  if (!sv || !sv->seq)
    return 2;
  struct seq_basis *q = sv->seq;
  if (!q->timing) {
    for (int i = 0; i < 4; i++)
      LSB_CHK_HIP(hipEventCreate(&q->ev[i]));
    q->timing = 1;
  }
  float ms = 0.0f;
  if (project_us) {
    *project_us = 0.0;
    if (q->timed_project) {
      LSB_CHK_HIP(hipEventElapsedTime(&ms, q->ev[0], q->ev[1]));
      *project_us = 1e3 * ms;
    }
  }
  if (update_us) {
    *update_us = 0.0;
    if (q->timed_update) {
      LSB_CHK_HIP(hipEventElapsedTime(&ms, q->ev[2], q->ev[3]));
      *update_us = 1e3 * ms;
    }
  }
  return 0;
}
