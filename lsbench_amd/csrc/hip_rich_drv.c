/* AMG as the solver: the host driver of the stationary V-cycle iteration (kernels: hip_rich.hip). */
#define _GNU_SOURCE
#include "hip_solver.h"

/*
 * Preconditioned Richardson with unit step, M^-1 = one AMG V-cycle, x0 = 0 (LSB_KRYLOV_RICHARDSON; the iteration
 * is written out at the head of hip_rich.hip): the protocol of the reference's AMG backends, which run a fixed
 * number of cycles with no tolerance (src/hypre.c:185-186, src/amgx.c:78-85) -- --maxit 2 --tol 0 here.
 *
 * Per cycle: the V-cycle's launches (amg_cycle, z into the shard's gather vector), the shard's SpMV on it
 * (q = S z), k_rich_update (x += z, r -= q, partials of r.r) and k_rich_step, the one workgroup that counts the
 * cycle and decides the stop.  The device decides (the shard's lsb_pcg_state, which the cycle's launches and
 * the SpMV gate on); the host side is run_loop (hip_run.c) with check_every cycles per poll and a cap: never more
 * cycles than maxit leaves to run.  Cycles are replayed from captured graphs under opts.use_graph (graph_launch); x
 * is the only pointer of the caller's in them, and the cache is keyed on it.
 *
 * No vector of its own: r and q are the shard's, z is its gather vector, x the caller's (or the internal one of a
 * padded / re-ordered solver), the state the shard's d_st polled through the solver's pinned h_st.
 *
 * One shard: the hierarchy couples all rows (precond_shard_amg).  Only AMG: the V-cycle with l1-Jacobi sweeps,
 * with the Chebyshev smoother on [rho / ratio, rho], or with multicolour Gauss-Seidel forward and backward (a
 * convergent smoother on every level), is an SPD M with lambda(M^-1 S) <= 1, so the iteration cannot diverge; FSAI, the Chebyshev polynomial and block-Jacobi give no such bound.
 */

void richardson_check(const struct lsb_hip_opts *o, int sharded) {
  if (o->krylov != LSB_KRYLOV_RICHARDSON)
    return;
  if (o->precond != LSB_PRECOND_AMG)
    errx(EXIT_FAILURE, "hip_cdna4: --krylov richardson runs the AMG V-cycle as the solver: --precond amg (no other "
                       "preconditioner bounds the spectrum of M^-1 S by 1)");
  if (sharded || o->nvirt > 1)
    errx(EXIT_FAILURE, "hip_cdna4: --krylov richardson runs on one shard (the AMG hierarchy couples all rows); use "
                       "it without --ngpus / --nvirt");
  if (o->persistent != 0)
    errx(EXIT_FAILURE, "hip_cdna4: --krylov richardson has no persistent form (--persistent 0)");
}

/* Cycles per host poll: run_chunk, at least 2 as for an AMG iteration of the batch (mrhs_chunk), on this cycle's
 * bytes: the V-cycle's, the SpMV at 12 B per non-zero, and 8 vector passes (the SpMV's two, the update's six);
 * opts.check_every overrides it. */
static int rich_chunk(const lsb_hip_solver *sv) {
  if (sv->o.check_every > 0)
    return sv->o.check_every;
  const struct shard *s = &sv->sh[0];
  return run_chunk((double)(12ull * s->nnz + lsb_hip_solver_amg_cycle_bytes(sv) + 64ull * s->n), 6.0, 2, 256);
}

/* what run_loop enqueues, and what a restart needs */
struct rich_enq {
  lsb_hip_solver *sv;
  const double *d_b;
  double *d_x;
};

static void rich_enqueue_cycles(void *ctx, int cycles) {
  const struct rich_enq *e = ctx;
  struct shard *s = &e->sv->sh[0];
  unsigned *nrr = &e->sv->rich_nrr;
  const struct amg_run c = {.a = s->amg, .vec = s->amg->vec, .r = s->d_r, .z = s->d_pfull, .st = s->d_st};
  for (int i = 0; i < cycles; i++) {
    amg_cycle(&c);                                                /* z = M^-1 r */
    spmv_shard(s, s->d_pfull, s->d_q, NULL, NULL, NULL, s->d_st); /* q = S z */
    lsb_k_rich_update(s->n, s->d_pfull, s->d_q, e->d_x, s->d_r, s->d_st, s->d_parts2, nrr, g_stream);
    lsb_k_rich_step(s->d_st, s->d_parts2, *nrr, g_stream);
  }
}

#define RICH_GRAPH_MAX 64 /* cycles per graph: a cycle is dozens of launches, and longer graphs cost more to build
                             than they save */
static void rich_enqueue(void *ctx, int cycles) {
  const struct rich_enq *e = ctx;
  while (cycles > 0) {
    const int c = cycles < RICH_GRAPH_MAX ? cycles : RICH_GRAPH_MAX;
    if (e->sv->o.use_graph)
      graph_launch(&e->sv->rich_graphs, c, e->d_x, rich_enqueue_cycles, ctx);
    else
      rich_enqueue_cycles(ctx, c);
    cycles -= c;
  }
}

/* Enqueue cycles until the device state leaves RUNNING; the final state lands in h_st[0] (whose iters the caller
 * cleared for the solve proper).  *hint: what this stretch of the previous solve took.  Never more cycles than maxit
 * leaves: once they are all enqueued, the poll behind them finds a final status. */
static void rich_run(void *ctx, unsigned *hint) {
  lsb_hip_solver *sv = ((struct rich_enq *)ctx)->sv;
  const struct run_loop r = {.name = "the Richardson iteration", .d_state = sv->sh[0].d_st, .h_state = sv->h_st,
                             .state_bytes = sizeof(struct lsb_pcg_state),
                             .stop_off = offsetof(struct lsb_pcg_state, status),
                             .progress_off = offsetof(struct lsb_pcg_state, iters),
                             .enqueue = rich_enqueue, .ctx = ctx, .chunk = rich_chunk(sv),
                             .cap = (long)sv->o.maxit - sv->h_st[0].iters, /* cycles the device can still run */
                             .what_hinted = "poll of a hinted Richardson solve",
                             .what_poll = "poll of the Richardson solve",
                             .what_drain = "drain after the Richardson solve"};
  run_loop(sv, &r, hint);
}

/* the restart of run_restarting: the cycles go on from r = b - S x, x kept */
static void rich_restart(void *ctx, int more) {
  const struct rich_enq *e = ctx;
  struct shard *s = &e->sv->sh[0];
  unsigned *nrr = &e->sv->rich_nrr;
  gather_x(e->sv, e->d_x);
  spmv_shard(s, s->d_pfull, s->d_q, NULL, NULL, NULL, NULL);
  lsb_k_rich_restart(s->n, e->d_b, s->d_q, s->d_r, s->d_parts2, nrr, g_stream);
  lsb_k_rich_restart_state(s->d_st, s->d_parts2, *nrr, more, g_stream);
}

int richardson_solve_dev(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res) {
  unsigned *nrr = &sv->rich_nrr;
  struct shard *s = &sv->sh[0];
  struct lsb_pcg_state *hst = sv->h_st;
  const double t0 = wall_seconds();
  lsb_k_rich_init(s->n, d_b, d_x, s->d_r, s->d_parts2, nrr, g_stream);
  lsb_k_rich_init_state(s->d_st, s->d_parts2, *nrr, sv->tol_run, (int)sv->o.maxit, g_stream);
  struct lsb_hip_result r;
  memset(&r, 0, sizeof r);
  r.true_relres = -1.0;
  struct rich_enq e = {sv, d_b, d_x};
  const struct restart_run v = {.run = rich_run, .restart = rich_restart, .ctx = &e, .d_state = s->d_st, .h_state = hst,
                                .state_bytes = sizeof hst[0],
                                .what_drain = "recomputed residual of the Richardson solve"};
  hst[0].iters = 0;
  const unsigned nverify = run_restarting(sv, &v, &r);
  check_aux_status(sv, "Richardson solve");
  result_from_state(&r, &hst[0]);
  r.spmvs = r.iters + nverify; /* one product per cycle counted, one per recomputed residual */
  r.seconds = wall_seconds() - t0;
  if (res)
    *res = r;
  g_last = r;
  return 0;
}
