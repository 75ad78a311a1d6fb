/* AMG as the solver on blocks of right-hand sides: the host driver (kernels: hip_rich_m.hip; the cycle: amg_cycle at
 * width kp, hip_amg_drv.c; the single-column driver: hip_rich_drv.c). */
#define _GNU_SOURCE
#include "hip_solver.h"

/*
 * lsb_hip_solver_amg_solve_multi[_dev]: the stationary V-cycle iteration of richardson_solve_dev on nrhs columns at
 * once.  A cycle is streams of the hierarchy's matrices, one product with S and six vector passes; a block of kp
 * columns reads every one of those matrices once for all of its columns and pays the same launches.  This is the
 * protocol of the reference's AMG backends (maxit 2, tol 0 in fp64; maxit 1, tol 0 with the fp32 cycle) on a block.
 *
 * 2 .. 8 columns run as one block of kp = 2, 4 or 8 (block_width), padded with zero columns -- CONVERGED from the
 * start, frozen, not reported; more run in blocks of 8 and a remainder; one column IS lsb_hip_solver_solve_dev.  The
 * block vectors B, X, R, Z and Q = S Z are internal and interleaved, in the solver's own numbering (lsb_k_mrhs_pack /
 * _unpack apply the permutation of a padded or re-ordered solver), so a cycle -- and a captured graph of cycles --
 * does not depend on the caller's pointers: the graphs of a work area are keyed on the count alone.
 *
 * A cycle: the V-cycle on the block R (fp64: hip_mrhs_amg.hip / hip_amg_cheb.hip, fp32: hip_amg_f32_m.hip), the SpMM
 * Q = S Z by lsb_k_spmm_csr at the lane count of the blocks' SpMM (the shard's), k_richm_update, k_richm_step.  Every
 * column has its own lsb_pcg_state inside the block's lsb_mrhs_state and stops on its own; a stopped column is frozen,
 * the block runs until every column has stopped (`running`, the gate of every launch).  The host side is run_loop on
 * `running`: rich_chunk's rule on the block's bytes or opts.check_every, the previous block's count in one go, never
 * more cycles than maxit leaves.
 *
 * opts.verify is the single driver's rule per column: after the block stops one SpMM forms S X, the columns called
 * converged get r = b - S x and their recomputed norm decides -- verified, or cycle on in place (x kept, cycles counted
 * on) while the column has restarts left (LSB_MAX_CORRECTIONS), else MAXIT.
 *
 * Served (richm_serves): krylov RICHARDSON with precond AMG on one shard in one process, fp64 values, smoothed by
 * l1-Jacobi (cycling in fp64 or fp32) or by the Chebyshev smoother (fp64).  Every other solver answers 2 and nothing
 * is allocated; a solver that never sees a block allocates nothing here.  Warm starts on blocks are not built.
 */
static int richm_serves(const lsb_hip_solver *sv) {
  const struct lsb_hip_opts *o = &sv->o;
  const struct amg_dev *a = sv->sh[0].amg;
  return !sv->multi && sv->nshard == 1 && !sv->dist && o->precision == LSB_PREC_FP64 &&
         o->krylov == LSB_KRYLOV_RICHARDSON && o->precond == LSB_PRECOND_AMG && a && !a->mcgs &&
         !(a->cheb && a->prec == LSB_AMG_PREC_FP32) && o->persistent <= 0 && !sv->ps.use &&
         (unsigned long long)sv->sh[0].n * LSB_MRHS_MAX < (1ull << 32);
}

static struct richm_work *richm_setup(lsb_hip_solver *sv, unsigned kp) {
  struct richm_work *w = &sv->rm[kp == 2 ? 0 : kp == 4 ? 1 : 2];
  if (w->blk.kp)
    return w;
  if (!sv->mr_hst) /* (mrhs_free's) */
    LSB_CHK_HIP(hipHostMalloc((void **)&sv->mr_hst, 2 * sizeof(struct lsb_mrhs_state), 0));
  /* behind the four blocks: the records of the SpMM (z_c . q_c, which nobody reads), those of the sweeps, the state */
  const size_t rsp = (size_t)LSB_MAX_PARTIALS * kp * sizeof(double);
  const size_t rsw = (size_t)LSB_STREAM_GRID_CAP * kp * sizeof(double);
  const size_t stb = (sizeof(struct lsb_mrhs_state) + 255) & ~(size_t)255;
  char *behind = block_work_slab(sv, &w->blk, kp, 4, rsp + rsw + stb); /* b, x, r and p = Q */
  w->rec_spmm = (double *)behind;
  w->rec = (double *)(behind + rsp);
  w->st = (struct lsb_mrhs_state *)(behind + rsp + rsw);
  block_work_z(sv, &w->blk, 0); /* z and the cycle's block vectors, in the precision the solver cycles in */
  return w;
}

void richm_free(lsb_hip_solver *sv) {
  for (int k = 0; k < 3; k++) {
    block_work_free(&sv->rm[k].blk);
    memset(&sv->rm[k], 0, sizeof sv->rm[k]);
  }
}

/* Bytes one cycle of a block of width kp streams: the V-cycle's matrices once whatever the width and its vector passes
 * per column (lsb_hip_solver_amg_cycle_bytes' two parts, in the precision the solver cycles in), the SpMM at 12 B per
 * non-zero and 16 B per row and column, the update's six vector passes per column.  kp = 1: rich_chunk's figure. */
static unsigned long long richm_cycle_bytes(const lsb_hip_solver *sv, unsigned kp) {
  const struct shard *s = &sv->sh[0];
  unsigned long long mat, vec;
  amg_cycle_bytes_split(s->amg, &mat, &vec);
  return mat + vec * kp + 12ull * s->nnz + 16ull * s->n * kp + 48ull * s->n * kp;
}

unsigned long long lsb_hip_solver_amg_solve_multi_bytes(const lsb_hip_solver *sv, unsigned nrhs) {
  if (!sv || nrhs == 0 || !richm_serves(sv))
    return 0;
  return richm_cycle_bytes(sv, nrhs == 1 ? 1u : block_width(nrhs > LSB_MRHS_MAX ? LSB_MRHS_MAX : nrhs));
}

/* cycles per host poll: rich_chunk's rule on the block's bytes */
static int richm_chunk(const lsb_hip_solver *sv, unsigned kp) {
  if (sv->o.check_every > 0)
    return sv->o.check_every;
  return run_chunk((double)richm_cycle_bytes(sv, kp), 6.0, 2, 256);
}

/* what run_loop enqueues */
struct richm_enq {
  lsb_hip_solver *sv;
  struct richm_work *w;
};

static void richm_enqueue_cycles(void *ctx, int cycles) {
  const struct richm_enq *e = ctx;
  const struct shard *s = &e->sv->sh[0];
  struct richm_work *w = e->w;
  const struct block_work *k = &w->blk;
  const struct amg_run c = {.a = s->amg, .vec = k->av, .kp = k->kp, .r = k->r, .z = k->z, .records = NULL,
                            .nrecords = NULL, .mst = w->st};
  for (int i = 0; i < cycles; i++) {
    unsigned nsp = 0;
    amg_cycle(&c); /* Z = M^-1 R */
    lsb_k_spmm_csr(k->kp, s->n, s->csr.offs, s->csr.cols, s->csr.vals, e->sv->mr_lanes, k->z, k->p, NULL, w->rec_spmm,
                   &nsp, w->st, g_stream); /* Q = S Z */
    lsb_k_richm_update(k->kp, s->n, k->z, k->p, k->x, k->r, w->st, w->rec, &w->nrec, g_stream);
    lsb_k_richm_step(k->kp, w->st, w->rec, w->nrec, g_stream);
  }
}

#define RICHM_GRAPH_MAX 64 /* cycles per graph, as the single driver's RICH_GRAPH_MAX */
static void richm_enqueue(void *ctx, int cycles) {
  const struct richm_enq *e = ctx;
  while (cycles > 0) {
    const int c = cycles < RICHM_GRAPH_MAX ? cycles : RICHM_GRAPH_MAX;
    if (e->sv->o.use_graph)
      graph_launch(&e->w->blk.g, c, NULL, richm_enqueue_cycles, ctx);
    else
      richm_enqueue_cycles(ctx, c);
    cycles -= c;
  }
}

/* Enqueue cycles until no column is running; the final state lands in mr_hst[0] (whose nspmm the caller cleared for the
 * solve proper).  cap: the cycles the device can still run -- once they are all enqueued the poll behind them finds
 * `running` cleared. */
static void richm_run(lsb_hip_solver *sv, struct richm_work *w, long cap, unsigned *hint) {
  struct richm_enq e = {sv, w};
  const struct run_loop r = {.name = "the Richardson iteration on a block", .d_state = w->st, .h_state = sv->mr_hst,
                             .state_bytes = sizeof(struct lsb_mrhs_state),
                             .stop_off = offsetof(struct lsb_mrhs_state, running), .stop_is_running = 1,
                             .progress_off = offsetof(struct lsb_mrhs_state, nspmm),
                             .enqueue = richm_enqueue, .ctx = &e, .chunk = richm_chunk(sv, w->blk.kp), .cap = cap,
                             .what_hinted = "poll of a hinted Richardson block",
                             .what_poll = "poll of the Richardson block",
                             .what_drain = "drain after the Richardson block"};
  run_loop(sv, &r, hint);
}

/* one block: nb <= 8 columns of the caller's */
static void richm_block(lsb_hip_solver *sv, unsigned nb, const double *d_B, size_t ldb, double *d_X, size_t ldx,
                        struct lsb_hip_result *res) {
  struct richm_work *w = richm_setup(sv, block_width(nb));
  const struct shard *s = &sv->sh[0];
  const struct block_work *k = &w->blk;
  struct lsb_mrhs_state *hst = sv->mr_hst;
  const unsigned kp = k->kp, n = s->n;
  unsigned nverify[LSB_MRHS_MAX] = {0};
  const double t0 = wall_seconds();
  lsb_k_mrhs_pack(n, kp, nb, sv->d_perm, d_B, ldb, k->b, g_stream);
  lsb_k_richm_init(kp, n, k->b, k->x, k->r, w->rec, &w->nrec, g_stream);
  lsb_k_richm_init_state(kp, w->st, w->rec, w->nrec, sv->o.tol, (int)sv->o.maxit, g_stream);
  hst[0].nspmm = 0;
  long cap = (long)sv->o.maxit;
  for (int round = 0;; round++) {
    richm_run(sv, w, cap, hint_slot(w->hint, round));
    if (!(sv->o.verify && sv->o.tol > 0.0))
      break;
    int any = 0;
    for (unsigned c = 0; c < nb; c++)
      if (hst[0].c[c].status == LSB_STATUS_CONVERGED && hst[0].c[c].bb > 0.0)
        any = 1, nverify[c]++;
    if (!any)
      break;
    /* "converged" is reported only for the residual RECOMPUTED from x: Q = S X, un-gated */
    unsigned nsp = 0;
    lsb_k_spmm_csr(kp, n, s->csr.offs, s->csr.cols, s->csr.vals, sv->mr_lanes, k->x, k->p, NULL, w->rec_spmm, &nsp,
                   NULL, g_stream);
    lsb_k_richm_restart(kp, n, k->b, k->p, k->r, w->st, w->rec, &w->nrec, g_stream);
    lsb_k_richm_restart_state(kp, w->st, w->rec, w->nrec, LSB_MAX_CORRECTIONS, g_stream);
    LSB_CHK_HIP(hipMemcpyAsync(&hst[0], w->st, sizeof hst[0], hipMemcpyDeviceToHost, g_stream));
    drain_stream(sv, "recomputed residuals of the Richardson block");
    if (!hst[0].running)
      break;
    cap = 0; /* what the restarted column with the fewest cycles behind it may still run */
    for (unsigned c = 0; c < kp; c++)
      if (hst[0].c[c].status == LSB_STATUS_RUNNING && (long)sv->o.maxit - hst[0].c[c].iters > cap)
        cap = (long)sv->o.maxit - hst[0].c[c].iters;
  }
  lsb_k_mrhs_unpack(n, kp, nb, sv->d_perm, k->x, d_X, ldx, g_stream);
  drain_stream(sv, "un-packing the Richardson block");
  const double seconds = wall_seconds() - t0;
  for (unsigned c = 0; c < nb; c++) {
    struct lsb_hip_result r;
    memset(&r, 0, sizeof r);
    result_from_state(&r, &hst[0].c[c]);
    r.true_relres = hst[0].true_relres[c];
    r.corrections = (unsigned)hst[0].corrections[c];
    r.spmvs = r.iters + nverify[c]; /* one product per cycle counted, one per recomputed residual */
    r.seconds = seconds;
    res[c] = r;
  }
}

int lsb_hip_solver_amg_solve_multi_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_B, size_t ldb, double *d_X,
                                       size_t ldx, struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, 0, d_B, ldb, d_X, ldx) || !richm_serves(sv))
    return 2;
  if (nrhs == 1)
    return lsb_hip_solver_solve_dev(sv, d_B, d_X, res);
  struct lsb_hip_result *tmp = res ? res : lsb_calloc(struct lsb_hip_result, nrhs);
  sv->start_n = 0; /* cold solves: lsb_hip_solver_start_relres has nothing to answer */
  for (unsigned c0 = 0; c0 < nrhs; c0 += LSB_MRHS_MAX) {
    const unsigned nb = nrhs - c0 < LSB_MRHS_MAX ? nrhs - c0 : LSB_MRHS_MAX;
    richm_block(sv, nb, d_B + (size_t)c0 * ldb, ldb, d_X + (size_t)c0 * ldx, ldx, tmp + c0);
  }
  g_last = tmp[nrhs - 1];
  if (!res)
    free(tmp);
  return 0;
}

int lsb_hip_solver_amg_solve_multi(lsb_hip_solver *sv, unsigned nrhs, const double *B, size_t ldb, double *X,
                                   size_t ldx, struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, 0, B, ldb, X, ldx) || !richm_serves(sv))
    return 2;
  return block_solve_host(lsb_hip_solver_amg_solve_multi_dev, 0, sv, nrhs, B, ldb, X, ldx, res);
}

/* Z_c = M^-1 R_c, one V-cycle per column of the block in the precision the solver cycles in, un-gated, through the
 * same pack / unpack: the first launches of a cycle of the iteration on their own */
int lsb_hip_solver_amg_cycle_multi_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_R, size_t ldr, double *d_Z,
                                       size_t ldz) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, 0, d_R, ldr, d_Z, ldz) || !richm_serves(sv))
    return 2;
  if (nrhs == 1)
    return lsb_hip_solver_precond_dev(sv, d_R, d_Z);
  const struct shard *s = &sv->sh[0];
  for (unsigned c0 = 0; c0 < nrhs; c0 += LSB_MRHS_MAX) {
    const unsigned nb = nrhs - c0 < LSB_MRHS_MAX ? nrhs - c0 : LSB_MRHS_MAX;
    const struct block_work *k = &richm_setup(sv, block_width(nb))->blk;
    const struct amg_run c = {.a = s->amg, .vec = k->av, .kp = k->kp, .r = k->r, .z = k->z, .records = NULL,
                              .nrecords = NULL, .mst = NULL};
    lsb_k_mrhs_pack(s->n, k->kp, nb, sv->d_perm, d_R + (size_t)c0 * ldr, ldr, k->r, g_stream);
    amg_cycle(&c);
    lsb_k_mrhs_unpack(s->n, k->kp, nb, sv->d_perm, k->z, d_Z + (size_t)c0 * ldz, ldz, g_stream);
  }
  drain_stream(sv, "lsb_hip_solver_amg_cycle_multi_dev");
  return 0;
}
