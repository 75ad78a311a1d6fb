/*
 * What a caller's solve is, whichever driver runs it ("Host loop"): the choice of the driver, a
 * cold solve and a solve from an initial guess, the residual recomputed from x and what follows from it -- the
 * correction runs of opts.verify, the check of the direct xGMI path, the in-place restarts of BiCGSTAB and
 * Richardson -- and the public single-column entry points.
 */
#define _GNU_SOURCE
#include "hip_solver.h"

/* The one place that maps opts.krylov to code; called once per solver, by solver_finish_setup. */
const struct solve_driver *solve_driver_for(int krylov) {
  static const struct solve_driver of[] = {
      [LSB_KRYLOV_PCG] = {pcg_solve_dev, pcg_run},        [LSB_KRYLOV_PCG1] = {pcg_solve_dev, pcg_run},
      [LSB_KRYLOV_AUTO] = {pcg_solve_dev, pcg_run},       [LSB_KRYLOV_GMRES] = {gmres_solve_dev, NULL},
      [LSB_KRYLOV_BICGSTAB] = {bicgstab_solve_dev, NULL}, [LSB_KRYLOV_RICHARDSON] = {richardson_solve_dev, NULL},
      [LSB_KRYLOV_DIRECT] = {direct_solve_dev, NULL}};
  if (krylov < 0 || krylov >= (int)(sizeof of / sizeof of[0]) || !of[krylov].solve)
    errx(EXIT_FAILURE, "hip_cdna4: opts.krylov = %d names no driver", krylov);
  return &of[krylov];
}

/* x into every shard's gather vector, halos exchanged: what a product with the operator starts from.  Overwrites the
 * search-direction vector.  (One shard: the exchange enqueues nothing.) */
void gather_x(lsb_hip_solver *sv, const double *d_x) {
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    LSB_CHK_HIP(hipMemcpyAsync(s->d_pfull + s->row_begin, d_x + (s->row_begin - sv->row_first),
                               (size_t)s->n * sizeof(double), hipMemcpyDeviceToDevice, g_stream));
  }
  exchange_p(sv, 0); /* not tied to a PCG state */
}

/* q = S x in every shard, with the fp64 values whatever opts.precision says */
void op_exact(lsb_hip_solver *sv, const double *d_x) {
  gather_x(sv, d_x);
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    spmv_shard_exact(s, s->d_pfull, s->d_q, s->d_pfull + s->row_begin, s->d_parts_pq, &s->npq, NULL);
  }
}

/* ||b - S x||^2 recomputed from x with the solver's operator, communicating WITHOUT the direct xGMI path; overwrites
 * the search-direction vector and leaves S x - b in every shard's q.  twice: formed off the CSR arrays as in twice
 * the working precision (k_resid_csr2) instead of by the solver's fp64 SpMV -- what opts.verify behind a warm start
 * reports. */
static double resid2(lsb_hip_solver *sv, const double *d_b, const double *d_x, int twice) {
  static const double minus_one = -1.0;
  const int on = sv->p2p_on, halo = sv->p2p_halo;
  double rr = 0.0;
  sv->p2p_on = sv->p2p_halo = 0;
  for (int i = 0; i < sv->nshard; i++)
    LSB_CHK_HIP(hipMemcpyAsync(sv->sh[i].d_scal + 5, &minus_one, sizeof(double), hipMemcpyHostToDevice, g_stream));
  if (twice)
    gather_x(sv, d_x);
  else
    op_exact(sv, d_x);
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    const size_t o = s->row_begin - sv->row_first;
    unsigned np = 0;
    if (twice)
      lsb_k_resid_csr2(s->n, s->csr.offs, s->csr.cols, s->csr.vals, s->lanes, s->d_pfull, d_b + o, s->d_q,
                       s->d_parts_pq, &np, g_stream);
    else {
      lsb_k_axpy(s->n, s->d_scal + 5, d_b + o, s->d_q, g_stream); /* q = S x - b */
      lsb_k_dot(s->n, s->d_q, s->d_q, s->d_parts_pq, &np, g_stream);
    }
    lsb_k_reduce_final(s->d_parts_pq, np, 1, s->d_scal + 4, 0, NULL, g_stream);
  }
  allreduce_scal(sv, 4, 1, 0);
  LSB_CHK_HIP(hipMemcpyAsync(&rr, sv->sh[0].d_scal + 4, sizeof rr, hipMemcpyDeviceToHost, g_stream));
  drain_stream(sv, "true residual");
  sv->p2p_on = on, sv->p2p_halo = halo;
  return rr;
}
double true_resid2(lsb_hip_solver *sv, const double *d_b, const double *d_x) { return resid2(sv, d_b, d_x, 0); }

/* The direct xGMI path passed its self-test, but a solve that ran over it is only reported if the residual recomputed
 * from x (relative to sqrt(bb)) agrees with the recurrence's r->relres: then it is r->true_relres, and 1 the answer.
 * Otherwise: say so -- `then` ends the message --, drop the path, forget the hints; 0: the caller solves again. */
int direct_path_agrees(lsb_hip_solver *sv, const double *d_b, const double *d_x, double bb, struct lsb_hip_result *r,
                       const char *then) {
  const double rr = true_resid2(sv, d_b, d_x), tr = bb > 0.0 ? sqrt(rr / bb) : 0.0;
  if (tr <= 100.0 * fmax(r->relres, sv->o.tol) + 1e-9) {
    r->true_relres = tr;
    return 1;
  }
  fprintf(stderr, "hip_cdna4: WARNING: true residual %.3e after a solve over the direct xGMI path (recurrence: %.3e); "
                  "falling back to RCCL and %s\n", tr, r->relres, then);
  sv->p2p_on = sv->p2p_halo = 0;
  memset(sv->hint_iters, 0, sizeof sv->hint_iters);
  return 0;
}

/* what an inner solve on fp32-rounded values is asked for at the least (0: the values are exact) */
double mixed_floor_tol(const lsb_hip_solver *sv) {
  int inexact = 0;
  for (int i = 0; i < sv->nshard; i++)
    inexact |= sv->sh[i].mixed && !sv->sh[i].exact32;
  return inexact ? LSB_MIXED_INNER_TOL : 0.0;
}

/* One run of the solver's own driver from x0 = 0 to `tol` relative to ||d_b||, nothing recomputed: sv->tol_run is
 * the tolerance every driver stops on, sv->verify_run = 0 keeps GMRES, BiCGSTAB and Richardson from restarting on
 * a recomputed residual of their own.  `round`: which of PCG's iteration-count hints the run uses. */
static void driver_run(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res, double tol,
                       int round) {
  sv->tol_run = tol, sv->verify_run = 0;
  if (sv->driver->run)
    sv->driver->run(sv, d_b, d_x, res, round);
  else
    sv->driver->solve(sv, d_b, d_x, res);
}

/*
 * opts.verify and the refinement of mixed precision, on the solve's own (b, x) with bb = b.b, behind a run that
 * reported CONVERGED: the residual b - S x RECOMPUTED from x (communicating over RCCL).  The recurrence residual
 * CG stops on drifts away from it over thousands of iterations (10 M-row 5-point operator, 9302 iterations:
 * recurrence 9.9e-9, recomputed 1.2e-8 at tol 1e-8), so a solve is reported converged only when the recomputed
 * residual meets the tolerance; otherwise the driver restarts on it (S e = b - S x from e = 0 to whatever is still
 * missing, x += e), at most LSB_MAX_CORRECTIONS times.  r->true_relres >= 0 on entry: a residual already recomputed.
 * twice: resid2's -- 0 in a cold solve, whose numbers stay what they were.
 */
void verify_correct(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *r, double bb,
                    int twice) {
  const int refine = sv->sh[0].mixed && sv->o.tol > 0.0;
  if (!((sv->o.verify || refine) && r->status == LSB_STATUS_CONVERGED && sv->o.tol > 0.0 && bb > 0.0))
    return;
  const double floor_tol = mixed_floor_tol(sv);
  for (int round = 1;; round++) {
    if (r->true_relres < 0.0 || round > 1)
      r->true_relres = sqrt(resid2(sv, d_b, d_x, twice) / bb), r->spmvs++;
    if (r->true_relres <= sv->o.tol || round > LSB_MAX_CORRECTIONS)
      break;
    /* S e = S x - b (what true_resid2 left in q), then x -= e */
    if (!sv->d_vr) {
      sv->d_vr = (double *)lsb_hip_malloc((size_t)sv->n_here * sizeof(double));
      sv->d_ve = (double *)lsb_hip_malloc((size_t)sv->n_here * sizeof(double));
    }
    for (int i = 0; i < sv->nshard; i++) {
      struct shard *s = &sv->sh[i];
      LSB_CHK_HIP(hipMemcpyAsync(sv->d_vr + (s->row_begin - sv->row_first), s->d_q, (size_t)s->n * sizeof(double),
                                 hipMemcpyDeviceToDevice, g_stream));
    }
    struct lsb_hip_result rc;
    /* relative to ||S x - b|| */
    driver_run(sv, sv->d_vr, sv->d_ve, &rc, fmax(0.7 * sv->o.tol / r->true_relres, floor_tol), round);
    for (int i = 0; i < sv->nshard; i++) {
      struct shard *s = &sv->sh[i];
      const size_t o = s->row_begin - sv->row_first;
      lsb_k_axpy(s->n, s->d_scal + 5, sv->d_ve + o, d_x + o, g_stream); /* d_scal[5] = -1 */
    }
    r->iters += rc.iters, r->spmvs += rc.spmvs, r->corrections++;
    if (rc.status != LSB_STATUS_CONVERGED) {
      r->status = rc.status;
      r->true_relres = sqrt(resid2(sv, d_b, d_x, twice) / bb), r->spmvs++;
      break;
    }
  }
  if (r->status == LSB_STATUS_CONVERGED && !(r->true_relres <= sv->o.tol))
    r->status = LSB_STATUS_MAXIT; /* the corrections did not get there: not converged */
  r->relres = r->true_relres;
  drain_stream(sv, "correction");
}

/* BiCGSTAB and Richardson under opts.verify: "converged" is reported only for the residual RECOMPUTED from x; where
 * that one misses the tolerance the iteration restarts on it in place (x kept), LSB_MAX_CORRECTIONS times at the
 * most, inside the timed region.  Leaves the final state in v->h_state and r->true_relres, r->corrections; returns
 * the number of residuals recomputed. */
unsigned run_restarting(lsb_hip_solver *sv, const struct restart_run *v, struct lsb_hip_result *r) {
  const struct lsb_pcg_state *hst = v->h_state;
  unsigned nverify = 0;
  for (int round = 0;; round++) {
    v->run(v->ctx, hint_slot(sv->hint_iters, round));
    if (!(sv->verify_run && hst->status == LSB_STATUS_CONVERGED && sv->tol_run > 0.0 && hst->bb > 0.0))
      break;
    v->restart(v->ctx, r->corrections < LSB_MAX_CORRECTIONS);
    nverify++;
    LSB_CHK_HIP(hipMemcpyAsync(v->h_state, v->d_state, v->state_bytes, hipMemcpyDeviceToHost, g_stream));
    drain_stream(sv, v->what_drain);
    r->true_relres = sqrt(hst->rr / hst->bb);
    if (hst->status != LSB_STATUS_RUNNING)
      break;
    r->corrections++;
  }
  return nverify;
}

/*
 * One solve from x0 = 0 as the caller sees it, by the solver's driver: its run, then -- opts.verify, or always
 * when the direct xGMI path carried a PCG run -- the recomputed residual and what follows from it (PCG: the
 * correction runs of verify_correct; BiCGSTAB, Richardson: run_restarting).
 */
int solve_core(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res) {
  sv->start_n = 0; /* a cold solve: lsb_hip_solver_start_relres has nothing to answer */
  sv->tol_run = sv->o.tol, sv->verify_run = sv->o.verify;
  return sv->driver->solve(sv, d_b, d_x, res);
}

void x0_vecs(lsb_hip_solver *sv) {
  if (!sv->d_x0r) {
    sv->d_x0r = (double *)lsb_hip_malloc((size_t)sv->n_here * sizeof(double));
    sv->d_x0e = (double *)lsb_hip_malloc((size_t)sv->n_here * sizeof(double));
  }
}

/*
 * One solve from the x0 that d_x holds (lsb_hip_solver_solve_x0[_dev]), for every driver and every PCG form from
 * this one place: q = S x0 the way a recomputed residual forms it, k_x0_start leaves r0 = b - q and the sums
 * (r0.r0, b.b), and the solver's own driver solves S e = r0 from e = 0 to tol sqrt(b.b / r0.r0) -- relative to
 * ||r0|| what opts.tol is relative to ||b||, and exactly opts.tol when x0 = 0, where the two sums have the same
 * bits.  x = x0 + e; opts.verify and the refinement of mixed precision then see the original (b, x), as in a cold
 * solve.  b = 0: x = 0.  ||r0|| <= tol ||b||: x0 is the answer and is not touched.
 */
int solve_x0_core(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res) {
  static const double plus_one = 1.0;
  const double t0 = wall_seconds(), tol = sv->o.tol;
  const int on = sv->p2p_on, halo = sv->p2p_halo;
  double sums[2] = {0.0, 0.0};
  x0_vecs(sv);
  sv->p2p_on = sv->p2p_halo = 0;
  op_exact(sv, d_x);
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    const size_t o = s->row_begin - sv->row_first;
    unsigned np = 0;
    LSB_CHK_HIP(hipMemcpyAsync(s->d_scal + 6, &plus_one, sizeof(double), hipMemcpyHostToDevice, g_stream));
    lsb_k_x0_start(s->n, d_b + o, s->d_q, sv->d_x0r + o, s->d_parts2, &np, g_stream);
    lsb_k_reduce_final(s->d_parts2, np, 2, s->d_scal + 3, 0, NULL, g_stream);
  }
  allreduce_scal(sv, 3, 2, 0);
  LSB_CHK_HIP(hipMemcpyAsync(sums, sv->sh[0].d_scal + 3, sizeof sums, hipMemcpyDeviceToHost, g_stream));
  drain_stream(sv, "starting residual");
  sv->p2p_on = on, sv->p2p_halo = halo;
  const double r0r0 = sums[0], bb = sums[1];
  struct lsb_hip_result r;
  memset(&r, 0, sizeof r);
  r.true_relres = -1.0;
  const double start = bb > 0.0 ? sqrt(r0r0 / bb) : 0.0;
  if (bb == 0.0) { /* the cold rule, whatever x0 holds */
    LSB_CHK_HIP(hipMemsetAsync(d_x, 0, (size_t)sv->n_here * sizeof(double), g_stream));
    drain_stream(sv, "x = 0");
    r.status = LSB_STATUS_CONVERGED, r.spmvs = 1;
  } else if (tol > 0.0 && r0r0 <= tol * tol * bb) {
    r.status = LSB_STATUS_CONVERGED, r.relres = start, r.spmvs = 1;
    if (sv->o.verify)
      r.true_relres = start; /* it IS the recomputed residual */
  } else {
    driver_run(sv, sv->d_x0r, sv->d_x0e, &r, fmax(tol * sqrt(bb / r0r0), mixed_floor_tol(sv)), 0);
    for (int i = 0; i < sv->nshard; i++) {
      struct shard *s = &sv->sh[i];
      const size_t o = s->row_begin - sv->row_first;
      lsb_k_axpy(s->n, s->d_scal + 6, sv->d_x0e + o, d_x + o, g_stream); /* d_scal[6] = 1 */
    }
    r.relres *= start; /* relative to ||b|| */
    if (sv->p2p_on && !direct_path_agrees(sv, d_b, d_x, bb, &r, "solving on from this x")) {
      /* ... which is x0 + e by now; the caller is told about both runs, and about the x0 that was theirs */
      struct lsb_hip_result again;
      solve_x0_core(sv, d_b, d_x, &again);
      if (sv->form != PCG_NONE)
        r.spmvs = pcg_spmvs(sv, &r);
      again.iters += r.iters, again.spmvs += r.spmvs + 2u; /* S x0 and the residual that failed the check */
      r = again;
    } else {
      if (sv->p2p_on)
        r.spmvs++; /* the residual of the check */
      if (sv->o.krylov != LSB_KRYLOV_GMRES) { /* (which recomputes nothing in a cold solve either) */
        const double tr = r.true_relres; /* the direct path's check; opts.verify recomputes in its own way */
        r.true_relres = -1.0;
        verify_correct(sv, d_b, d_x, &r, bb, sv->o.verify != 0); /* (the refinement alone: the cold solve's residual) */
        if (r.true_relres < 0.0)
          r.true_relres = tr;
      }
      drain_stream(sv, "x = x0 + e");
      if (sv->form != PCG_NONE)
        r.spmvs = pcg_spmvs(sv, &r);
      r.spmvs++; /* S x0 */
    }
  }
  r.seconds = wall_seconds() - t0;
  start_relres_slots(sv, 1)[0] = start;
  if (res)
    *res = r;
  g_last = r;
  return 0;
}

double *start_relres_slots(lsb_hip_solver *sv, unsigned nrhs) {
  if (nrhs > sv->start_cap) {
    sv->start_rr = (double *)realloc(sv->start_rr, (size_t)nrhs * sizeof(double));
    if (!sv->start_rr)
      errx(EXIT_FAILURE, "hip_cdna4: out of memory");
    sv->start_cap = nrhs;
  }
  sv->start_n = nrhs;
  return sv->start_rr;
}

int lsb_hip_solver_start_relres(const lsb_hip_solver *sv, unsigned nrhs, double *out) {
  if (!sv || !out || nrhs == 0 || nrhs != sv->start_n)
    return 2;
  memcpy(out, sv->start_rr, (size_t)nrhs * sizeof(double));
  return 0;
}

/* The single-column entry points, cold or (warm) from the x0 that x holds.  On device vectors in the caller's
 * ordering: a padded or re-ordered solver solves in its own */
static int solve_user_dev(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res, int warm) {
  solve_dev_fn *core = warm ? solve_x0_core : solve_core;
  if (!sv->d_perm)
    return core(sv, d_b, d_x, res);
  /* b' = Q b ; solve Q S Q^T x' = b' ; x = Q^T x'   (src/cusparse.c:177,204); warm: x0' = Q x0 (a pad row: 0) */
  struct lsb_hip_result r;
  lsb_k_perm_gather(sv->n_here, sv->d_perm, d_b, sv->d_bp, g_stream);
  if (warm)
    lsb_k_perm_gather(sv->n_here, sv->d_perm, d_x, sv->d_xp, g_stream);
  const int rc = core(sv, sv->d_bp, sv->d_xp, &r);
  /* an x0 that already is the answer stays where it is, bit for bit */
  if (!(warm && r.status == LSB_STATUS_CONVERGED && r.iters == 0 && sv->start_rr[0] > 0.0)) {
    lsb_k_perm_scatter(sv->n_here, sv->d_perm, sv->d_xp, d_x, g_stream);
    drain_stream(sv, "un-permuting x");
  }
  if (res)
    *res = r;
  return rc;
}

/* on host vectors */
static int solve_user_host(lsb_hip_solver *sv, const double *b, double *x, struct lsb_hip_result *res, int warm) {
  const size_t bytes = (size_t)sv->n_user * sizeof(double);
  double *d_b = (double *)lsb_hip_malloc(bytes), *d_x = (double *)lsb_hip_malloc(bytes);
  LSB_CHK_HIP(hipMemcpy(d_b, b, bytes, hipMemcpyHostToDevice));
  if (warm)
    LSB_CHK_HIP(hipMemcpy(d_x, x, bytes, hipMemcpyHostToDevice));
  const int rc = solve_user_dev(sv, d_b, d_x, res, warm);
  LSB_CHK_HIP(hipMemcpy(x, d_x, bytes, hipMemcpyDeviceToHost));
  /* cached graphs must not outlive the buffers they were captured with */
  drop_graphs(sv);
  lsb_hip_free(d_b), lsb_hip_free(d_x);
  return rc;
}

int lsb_hip_solver_solve_dev(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (!sv || !d_b || !d_x)
    return 2;
  return solve_user_dev(sv, d_b, d_x, res, 0);
}

int lsb_hip_solver_solve_x0_dev(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (!sv || !d_b || !d_x)
    return 2;
  return solve_user_dev(sv, d_b, d_x, res, 1);
}

int lsb_hip_solver_solve(lsb_hip_solver *sv, const double *b, double *x, struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (!sv || !b || !x)
    return 2;
  return solve_user_host(sv, b, x, res, 0);
}

int lsb_hip_solver_solve_x0(lsb_hip_solver *sv, const double *b, double *x, struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (!sv || !b || !x)
    return 2;
  return solve_user_host(sv, b, x, res, 1);
}
