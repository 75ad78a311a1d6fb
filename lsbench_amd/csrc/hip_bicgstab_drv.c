/* BiCGSTAB host driver (kernels: hip_bicgstab.hip). */
#define _GNU_SOURCE
#include "hip_solver.h"

/*
 * Right-preconditioned BiCGSTAB, M^-1 = diag(dinv) (Jacobi, l1-Jacobi or none), x0 = 0, shadow
 * residual r^ = r0 = b (the iteration is written out at the head of
 * hip_bicgstab.hip).  Per iteration: two SpMVs with their fused dots (sigma = r^.v, ts = t.s) and four
 * sweeps.  The device decides when to stop (lsb_bcg_state); the host side is run_loop (hip_run.c) with
 * check_every iterations per poll.  Iterations are enqueued plainly: replaying them from the graph cache
 * (graph_launch) would be a change of behaviour that has not been measured.
 *
 * Vectors per shard: r (holds s between k_bcg_s and k_bcg_xr), v (the shard's q), t, p, r^, x, and
 * two gather vectors -- p^ = D^-1 p in the shard's own (d_pfull), s^ = D^-1 s in a second one.
 * They come out of the shard's slab (shard_upload sizes it for them).
 *
 * Over shards: exchange_p in front of each SpMV and one all-reduce per reduction point (sigma; ss;
 * ts and tt together; rr and rho' together), each shard keeping its own copy of the state and
 * taking the same decisions from the same all-reduced numbers.
 */
#define BCG_RED 8 /* doubles per shard: [0] sigma [1] ss [2] ts [3] tt [4] rr (or b.b) [5] rho' */

#define EACH(i, s, w)                                                          \
  for (int i = 0; i < sv->nshard; i++)                                         \
    for (struct shard *s = &sv->sh[i]; s; s = NULL)                            \
      for (struct bcg_work *w = &sv->bcg[i]; w; w = NULL)

static void bcg_allreduce(lsb_hip_solver *sv, unsigned off, unsigned cnt) {
  red_allreduce(sv, sv->bcg_red, BCG_RED, off, cnt);
}

/* the halos of the second gather vector (s^) */
static void exchange_shat(lsb_hip_solver *sv) {
  double **full = lsb_calloc(double *, sv->nshard);
  EACH(i, s, w) {
    (void)s;
    full[i] = w->sfull;
  }
  exchange_vec(sv, 0, full); /* not tied to a PCG state */
  free(full);
}

static void bcg_setup(lsb_hip_solver *sv) {
  if (sv->bcg)
    return;
  sv->bcg = lsb_calloc(struct bcg_work, sv->nshard);
  sv->bcg_red = (double *)lsb_hip_malloc((size_t)sv->nshard * BCG_RED * sizeof(double));
  LSB_CHK_HIP(hipMemsetAsync(sv->bcg_red, 0, (size_t)sv->nshard * BCG_RED * sizeof(double), g_stream));
  LSB_CHK_HIP(hipHostMalloc((void **)&sv->bcg_hst, 2 * sizeof(struct lsb_bcg_state), 0));
  EACH(i, s, w) {
    w->t = shard_vec(s, s->n);
    w->p = shard_vec(s, s->n);
    w->rhat = shard_vec(s, s->n);
    w->sfull = shard_vec(s, s->n_glob);
    LSB_CHK_HIP(hipMemsetAsync(w->sfull, 0, (size_t)s->n_glob * sizeof(double), g_stream));
    w->st = (struct lsb_bcg_state *)lsb_hip_malloc(sizeof(struct lsb_bcg_state));
    LSB_CHK_HIP(hipMemsetAsync(w->st, 0, sizeof *w->st, g_stream));
  }
}

void bicgstab_free(lsb_hip_solver *sv) {
  if (!sv->bcg)
    return;
  EACH(i, s, w) {
    shard_vec_free(s, w->t), shard_vec_free(s, w->p), shard_vec_free(s, w->rhat);
    shard_vec_free(s, w->sfull);
    lsb_hip_free(w->st);
  }
  free(sv->bcg), sv->bcg = NULL;
  lsb_hip_free(sv->bcg_red);
  LSB_CHK_HIP(hipHostFree(sv->bcg_hst));
}

/* Iterations per host poll, from numbers all ranks agree on: run_chunk with this iteration's bytes -- two SpMVs at
 * 12 B per non-zero and 28 vector passes counting the SpMVs' own -- and half of PCG's bounds at twice its floor, an
 * iteration being two of PCG's; opts.check_every overrides it. */
static int bcg_chunk(const lsb_hip_solver *sv) {
  if (sv->o.check_every > 0)
    return sv->o.check_every;
  const struct shard *s = &sv->sh[0];
  double bytes = 24.0 * (double)s->nnz + 224.0 * (double)s->n;
  if (sv->dist)
    bytes = 24.0 * (double)sv->agree_nnz + 224.0 * (double)sv->agree_n;
  return run_chunk(bytes, 12.0, 4, 128);
}

/* one iteration; parity = its number & 1 (which copy of rho it reads) */
static void bcg_enqueue_iter(lsb_hip_solver *sv, double *d_x, int parity) {
  const int multi = sv->multi;
  if (multi)
    exchange_p(sv, 0); /* not tied to a PCG state */
  EACH(i, s, w) { /* v = Op p^ ; sigma = r^.v */
    spmv_shard(s, s->d_pfull, s->d_q, w->rhat, s->d_parts_pq, &s->npq, &w->st->c);
    if (multi)
      lsb_k_reduce_final(s->d_parts_pq, s->npq, 1, sv->bcg_red + (size_t)i * BCG_RED, 0, &w->st->c, g_stream);
  }
  bcg_allreduce(sv, 0, 1);
  EACH(i, s, w) {
    double *red = sv->bcg_red + (size_t)i * BCG_RED;
    lsb_k_bcg_s(s->n, s->d_r, s->d_q, DINV(s), w->sfull + s->row_begin, w->st, parity,
                multi ? red : s->d_parts_pq, multi ? 1u : s->npq, s->d_parts2, &w->nss, g_stream);
    if (multi)
      lsb_k_reduce_final(s->d_parts2, w->nss, 1, red + 1, 0, &w->st->c, g_stream);
  }
  bcg_allreduce(sv, 1, 1);
  if (multi)
    exchange_shat(sv);
  EACH(i, s, w) { /* t = Op s^ ; ts = t.s ; tt = t.t */
    double *red = sv->bcg_red + (size_t)i * BCG_RED, *tt = s->d_parts2 + LSB_MAX_PARTIALS;
    spmv_shard(s, w->sfull, w->t, s->d_r, s->d_parts_pq, &s->npq, &w->st->c);
    lsb_k_bcg_tt(s->n, w->t, w->st, tt, &w->ntt, g_stream);
    if (multi)
      lsb_k_reduce_final2(s->d_parts_pq, s->npq, 1, red + 2, tt, w->ntt, 1, red + 3, &w->st->c, g_stream);
  }
  bcg_allreduce(sv, 2, 2);
  EACH(i, s, w) {
    double *red = sv->bcg_red + (size_t)i * BCG_RED, *tt = s->d_parts2 + LSB_MAX_PARTIALS,
           *p2 = s->d_parts2 + 2 * LSB_MAX_PARTIALS;
    lsb_k_bcg_xr(s->n, d_x + (s->row_begin - sv->row_first), s->d_pfull + s->row_begin, w->sfull + s->row_begin,
                 s->d_r, w->t, w->rhat, w->st, multi ? red + 1 : s->d_parts2, multi ? 1u : w->nss,
                 multi ? red + 2 : s->d_parts_pq, multi ? 1u : s->npq, multi ? red + 3 : tt,
                 multi ? 1u : w->ntt, p2, &w->np2, g_stream);
    if (multi)
      lsb_k_reduce_final(p2, w->np2, 2, red + 4, 0, &w->st->c, g_stream);
  }
  bcg_allreduce(sv, 4, 2);
  EACH(i, s, w) {
    double *red = sv->bcg_red + (size_t)i * BCG_RED, *p2 = s->d_parts2 + 2 * LSB_MAX_PARTIALS;
    lsb_k_bcg_p(s->n, s->d_r, w->p, s->d_q, DINV(s), s->d_pfull + s->row_begin, w->st, parity,
                multi ? red + 4 : p2, multi ? 1u : w->np2, g_stream);
  }
}

/* what run_loop enqueues and what a restart needs: `it` counts the iterations enqueued in this solve (its parity
 * picks the copy of rho) */
struct bcg_enq {
  lsb_hip_solver *sv;
  const double *d_b;
  double *d_x;
  unsigned it;
};
static void bcg_enqueue(void *ctx, int count) {
  struct bcg_enq *e = ctx;
  for (int i = 0; i < count; i++, e->it++)
    bcg_enqueue_iter(e->sv, e->d_x, (int)(e->it & 1u));
}

/* Enqueue iterations until the device state leaves RUNNING; the final state lands in bcg_hst[0] (whose c.iters
 * the caller cleared for the solve proper).  *hint: what this stretch of the previous solve took. */
static void bcg_run(void *ctx, unsigned *hint) {
  lsb_hip_solver *sv = ((struct bcg_enq *)ctx)->sv;
  const struct run_loop r = {.name = "BiCGSTAB", .d_state = sv->bcg[0].st, .h_state = sv->bcg_hst,
                             .state_bytes = sizeof(struct lsb_bcg_state),
                             .stop_off = offsetof(struct lsb_bcg_state, c.status),
                             .progress_off = offsetof(struct lsb_bcg_state, c.iters),
                             .enqueue = bcg_enqueue, .ctx = ctx, .chunk = bcg_chunk(sv), .cap = -1,
                             .what_hinted = "poll of a hinted BiCGSTAB solve",
                             .what_poll = "poll of the BiCGSTAB solve", .what_drain = "drain after the BiCGSTAB solve"};
  run_loop(sv, &r, hint);
}

/* the restart of run_restarting: r = b - Op x, r^ = p = r, x kept */
static void bcg_restart(void *ctx, int more) {
  const struct bcg_enq *e = ctx;
  lsb_hip_solver *sv = e->sv;
  const int multi = sv->multi;
  gather_x(sv, e->d_x);
  EACH(i, s, w) {
    spmv_shard(s, s->d_pfull, s->d_q, NULL, NULL, NULL, NULL);
    lsb_k_bcg_restart(s->n, e->d_b + (s->row_begin - sv->row_first), s->d_q, DINV(s), s->d_r, w->rhat, w->p,
                      s->d_pfull + s->row_begin, s->d_parts2, &w->np2, g_stream);
    if (multi)
      lsb_k_reduce_final(s->d_parts2, w->np2, 1, sv->bcg_red + (size_t)i * BCG_RED + 4, 0, NULL, g_stream);
  }
  bcg_allreduce(sv, 4, 1);
  EACH(i, s, w)
    lsb_k_bcg_restart_state(w->st, multi ? sv->bcg_red + (size_t)i * BCG_RED + 4 : s->d_parts2,
                            multi ? 1u : w->np2, more, g_stream);
}

int bicgstab_solve_dev(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res) {
  bcg_setup(sv);
  const int multi = sv->multi;
  struct lsb_bcg_state *hst = sv->bcg_hst;
  const double t0 = wall_seconds();
  EACH(i, s, w) {
    const size_t o = s->row_begin - sv->row_first;
    lsb_k_bcg_init(s->n, d_b + o, DINV(s), d_x + o, s->d_r, w->rhat, w->p, s->d_pfull + s->row_begin,
                   s->d_parts2, &w->np2, g_stream);
    if (multi)
      lsb_k_reduce_final(s->d_parts2, w->np2, 1, sv->bcg_red + (size_t)i * BCG_RED + 4, 0, NULL, g_stream);
  }
  bcg_allreduce(sv, 4, 1);
  EACH(i, s, w)
    lsb_k_bcg_init_state(w->st, multi ? sv->bcg_red + (size_t)i * BCG_RED + 4 : s->d_parts2,
                         multi ? 1u : w->np2, sv->tol_run, (int)sv->o.maxit, g_stream);
  struct lsb_hip_result r;
  memset(&r, 0, sizeof r);
  r.true_relres = -1.0;
  struct bcg_enq enq = {.sv = sv, .d_b = d_b, .d_x = d_x};
  const struct restart_run v = {.run = bcg_run, .restart = bcg_restart, .ctx = &enq, .d_state = sv->bcg[0].st,
                                .h_state = hst, .state_bytes = sizeof hst[0],
                                .what_drain = "recomputed residual of the BiCGSTAB solve"};
  hst[0].c.iters = 0;
  const unsigned nverify = run_restarting(sv, &v, &r);
  check_aux_status(sv, "BiCGSTAB solve");
  result_from_state(&r, &hst[0].c);
  r.spmvs = (unsigned)hst[0].nspmv + nverify;
  r.seconds = wall_seconds() - t0;
  if (res)
    *res = r;
  g_last = r;
  return 0;
}
