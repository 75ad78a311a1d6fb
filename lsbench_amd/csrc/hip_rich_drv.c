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
 * the SpMV gate on); the host enqueues check_every cycles at a time, one chunk ahead of the poll, as the other
 * loops do, and never more cycles than maxit leaves to run.  Chunks are replayed from captured graphs under
 * opts.use_graph; x is the only pointer of the caller's in them, and the cache is keyed on it.
 *
 * No vector of its own: r and q are the shard's, z is its gather vector, x the caller's (or the internal one of a
 * padded / re-ordered solver), the state the shard's d_st polled through the solver's pinned h_st.
 *
 * One shard: the hierarchy couples all rows (precond_shard_amg).  Only AMG: the V-cycle with l1-Jacobi sweeps,
 * or with the Chebyshev smoother on [rho / ratio, rho], is an SPD M with lambda(M^-1 S) <= 1, so the iteration
 * cannot diverge; FSAI, the Chebyshev polynomial and block-Jacobi give no such bound.
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

static struct rich_work *rich_setup(lsb_hip_solver *sv) {
  if (!sv->rich)
    sv->rich = lsb_calloc(struct rich_work, 1);
  return sv->rich;
}

void richardson_drop_graphs(lsb_hip_solver *sv) {
  struct rich_work *w = sv->rich;
  for (int i = 0; w && i < LSB_NGRAPH; i++)
    if (w->g[i].exec) {
      LSB_CHK_HIP(hipGraphExecDestroy(w->g[i].exec));
      w->g[i].exec = NULL;
    }
}

void richardson_free(lsb_hip_solver *sv) {
  richardson_drop_graphs(sv);
  free(sv->rich), sv->rich = NULL;
}

/* Cycles per host poll: mrhs_chunk's rule for an AMG iteration -- about 0.3 ms of device work at an assumed
 * 4 TB/s, at least 2 -- on this cycle's bytes: the V-cycle's, the SpMV at 12 B per non-zero, and 8 vector passes
 * (the SpMV's two, the update's six).  An estimate: the poll runs one chunk ahead, so the size only bounds the
 * no-op launches enqueued past the stop; opts.check_every overrides it. */
static int rich_chunk(const lsb_hip_solver *sv) {
  if (sv->o.check_every > 0)
    return sv->o.check_every;
  const struct shard *s = &sv->sh[0];
  double us = (double)(12ull * s->nnz + lsb_hip_solver_amg_cycle_bytes(sv) + 64ull * s->n) / 4.0e6;
  if (us < 6.0)
    us = 6.0;
  const int c = (int)(300.0 / us);
  return c < 2 ? 2 : c > 256 ? 256 : c;
}

static void rich_enqueue_cycle(lsb_hip_solver *sv, double *d_x) {
  struct shard *s = &sv->sh[0];
  const struct amg_run c = {.a = s->amg, .vec = s->amg->vec, .r = s->d_r, .z = s->d_pfull, .st = s->d_st};
  amg_cycle(&c);                                                           /* z = M^-1 r */
  spmv_shard(s, s->d_pfull, s->d_q, NULL, NULL, NULL, s->d_st);            /* q = S z */
  lsb_k_rich_update(s->n, s->d_pfull, s->d_q, d_x, s->d_r, s->d_st, s->d_parts2, &sv->rich->nrr, g_stream);
  lsb_k_rich_step(s->d_st, s->d_parts2, sv->rich->nrr, g_stream);
}

/* hipGraph of `cycles` cycles writing to d_x */
#define RICH_GRAPH_MAX 64 /* cycles per graph: a cycle is dozens of launches, and longer graphs cost more to build
                             than they save */
static hipGraphExec_t rich_graph(lsb_hip_solver *sv, int cycles, double *d_x) {
  struct rich_work *w = sv->rich;
  for (int i = 0; i < LSB_NGRAPH; i++)
    if (w->g[i].exec && w->g[i].cycles == cycles && w->g[i].x == d_x)
      return w->g[i].exec;
  const int slot = w->gnext;
  w->gnext = (w->gnext + 1) % LSB_NGRAPH;
  if (w->g[slot].exec)
    LSB_CHK_HIP(hipGraphExecDestroy(w->g[slot].exec));
  hipGraph_t g;
  LSB_CHK_HIP(hipStreamBeginCapture(g_stream, hipStreamCaptureModeThreadLocal));
  for (int i = 0; i < cycles; i++)
    rich_enqueue_cycle(sv, d_x);
  LSB_CHK_HIP(hipStreamEndCapture(g_stream, &g));
  LSB_CHK_HIP(hipGraphInstantiate(&w->g[slot].exec, g, NULL, NULL, 0));
  LSB_CHK_HIP(hipGraphDestroy(g));
  w->g[slot].cycles = cycles, w->g[slot].x = d_x;
  return w->g[slot].exec;
}

static void rich_enqueue(lsb_hip_solver *sv, double *d_x, int cycles) {
  while (cycles > 0) {
    const int c = cycles < RICH_GRAPH_MAX ? cycles : RICH_GRAPH_MAX;
    if (sv->o.use_graph)
      LSB_CHK_HIP(hipGraphLaunch(rich_graph(sv, c, d_x), g_stream));
    else
      for (int i = 0; i < c; i++)
        rich_enqueue_cycle(sv, d_x);
    cycles -= c;
  }
}

/* Enqueue cycles until the device state leaves RUNNING; the final state lands in h_st[0].  *hint: what this
 * stretch of the previous solve took -- the benchmark protocol repeats the same solve -- enqueued in one go.
 * Never more cycles than maxit leaves: once they are all enqueued, the poll behind them finds a final status. */
static void rich_run(lsb_hip_solver *sv, double *d_x, unsigned *hint) {
  struct lsb_pcg_state *hst = sv->h_st;
  struct shard *s = &sv->sh[0];
  const int chunk = rich_chunk(sv);
  const int before = hst[0].iters; /* (0 for the solve proper: the caller clears it) */
  long left = (long)sv->o.maxit - before; /* cycles the device can still run */
#define ENQUEUE_CYCLES(count)                                                  \
  do {                                                                         \
    const long c_ = (count) < left ? (long)(count) : left;                     \
    if (c_ > 0)                                                                \
      rich_enqueue(sv, d_x, (int)c_), left -= c_;                              \
  } while (0)
#define ENQUEUE_POLL(slot)                                                     \
  do {                                                                         \
    LSB_CHK_HIP(hipMemcpyAsync(&hst[slot], s->d_st, sizeof hst[0], hipMemcpyDeviceToHost, g_stream)); \
    LSB_CHK_HIP(hipEventRecord(sv->ev_poll[slot], g_stream));                  \
  } while (0)
  int fin = -1;
  if (*hint > 0) {
    ENQUEUE_CYCLES((long)*hint);
    ENQUEUE_POLL(0);
    wait_event(sv, sv->ev_poll[0], "poll of a hinted Richardson solve");
    if (hst[0].status != LSB_STATUS_RUNNING)
      fin = 0;
  }
  if (fin < 0) {
    int cur = 0;
    ENQUEUE_CYCLES(chunk);
    ENQUEUE_POLL(0);
    for (;;) {
      const long had = left;
      ENQUEUE_CYCLES(chunk); /* one chunk ahead of the poll */
      ENQUEUE_POLL(cur ^ 1);
      wait_event(sv, sv->ev_poll[cur], "poll of the Richardson solve");
      if (hst[cur].status != LSB_STATUS_RUNNING) {
        fin = cur;
        break;
      }
      cur ^= 1;
      if (had <= 0) /* cannot happen: every cycle maxit allows ran before that poll */
        errx(EXIT_FAILURE, "hip_cdna4: the Richardson iteration ran past maxit without a status");
    }
    drain_stream(sv, "drain after the Richardson solve"); /* the speculative chunk */
  }
#undef ENQUEUE_CYCLES
#undef ENQUEUE_POLL
  if (fin != 0)
    hst[0] = hst[fin];
  *hint = (unsigned)(hst[0].iters - before);
}

int richardson_solve_dev(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res) {
  struct rich_work *w = rich_setup(sv);
  struct shard *s = &sv->sh[0];
  struct lsb_pcg_state *hst = sv->h_st;
  const double t0 = wall_seconds();
  lsb_k_rich_init(s->n, d_b, d_x, s->d_r, s->d_parts2, &w->nrr, g_stream);
  lsb_k_rich_init_state(s->d_st, s->d_parts2, w->nrr, sv->o.tol, (int)sv->o.maxit, g_stream);
  struct lsb_hip_result r;
  memset(&r, 0, sizeof r);
  r.true_relres = -1.0;
  unsigned nverify = 0;
  hst[0].iters = 0;
  for (int round = 0;; round++) {
    rich_run(sv, d_x, &sv->hint_iters[round < LSB_MAX_CORRECTIONS ? round : LSB_MAX_CORRECTIONS]);
    if (!(sv->o.verify && hst[0].status == LSB_STATUS_CONVERGED && sv->o.tol > 0.0 && hst[0].bb > 0.0))
      break;
    /* "converged" is reported only for the residual RECOMPUTED from x; where that one misses the tolerance the
     * cycles go on from it (r = b - S x, x kept), LSB_MAX_CORRECTIONS times at the most, inside the timed region */
    LSB_CHK_HIP(hipMemcpyAsync(s->d_pfull, d_x, (size_t)s->n * sizeof(double), hipMemcpyDeviceToDevice, g_stream));
    spmv_shard(s, s->d_pfull, s->d_q, NULL, NULL, NULL, NULL);
    lsb_k_rich_restart(s->n, d_b, s->d_q, s->d_r, s->d_parts2, &w->nrr, g_stream);
    lsb_k_rich_restart_state(s->d_st, s->d_parts2, w->nrr, r.corrections < LSB_MAX_CORRECTIONS, g_stream);
    nverify++;
    LSB_CHK_HIP(hipMemcpyAsync(&hst[0], s->d_st, sizeof hst[0], hipMemcpyDeviceToHost, g_stream));
    drain_stream(sv, "recomputed residual of the Richardson solve");
    r.true_relres = sqrt(hst[0].rr / hst[0].bb);
    if (hst[0].status != LSB_STATUS_RUNNING)
      break;
    r.corrections++;
  }
  check_aux_status(sv, "Richardson solve");
  r.iters = (unsigned)hst[0].iters;
  r.status = hst[0].status;
  r.relres = hst[0].bb > 0.0 ? sqrt(hst[0].rr / hst[0].bb) : 0.0;
  r.spmvs = r.iters + nverify; /* one product per cycle counted, one per recomputed residual */
  r.seconds = wall_seconds() - t0;
  if (res)
    *res = r;
  g_last = r;
  return 0;
}
