/* Several right-hand sides: host driver (kernels: hip_mrhs.hip, hip_mrhs_x0.hip, hip_mrhs_amg.hip, hip_mrhs_fsai.hip;
 * the work area, the service rules and Z = M^-1 R it shares with the block-CG driver: hip_block.c). */
#define _GNU_SOURCE
#include "hip_solver.h"

/*
 * lsb_hip_solver_solve_multi[_dev]: nrhs INDEPENDENT Jacobi-PCG recurrences (x0 = 0, or -- solve_multi_x0_dev -- the
 * X0 the caller's X holds: mrhs_batch; M^-1 = diag(dinv):
 * Jacobi, l1-Jacobi or none) advanced by the same launches -- per iteration the SpMM Q = S P off the
 * shard's CSR arrays with its fused per-column p.q, k_mrhs_update_xr and k_mrhs_update_p.  Every column has
 * its own alpha, beta, norms, iteration count and status (lsb_mrhs_state); a column that has stopped is
 * frozen while the others run on, and the batch runs until every column has stopped.  This is not block-CG.
 *
 * 2 .. 8 columns run as one batch of kp = 2, 4 or 8, padded with zero columns (b = 0: frozen from the
 * start); more run in batches of 8 and a remainder; one column IS lsb_hip_solver_solve_dev.  The block
 * vectors b, x, r, p, q are internal (interleaved, internal numbering: k_mrhs_pack / k_mrhs_unpack apply the
 * permutation of a padded or re-ordered solver), so an iteration -- and a captured graph of iterations --
 * does not depend on the caller's pointers.  The device decides when to stop; the host side is run_loop
 * (hip_run.c): check_every iterations per poll, or the previous batch's count in one go.
 *
 * opts.verify: after the batch stops one SpMM recomputes b - S x of every column; the columns the recurrence
 * called converged but whose recomputed residual misses the tolerance restart IN PLACE (r = b - S x,
 * p = D^-1 r, x kept, bb and the threshold unchanged, iterations counted on), all others stay frozen;
 * LSB_MAX_CORRECTIONS rounds at the most, a column that still misses is MAXIT.
 *
 * LSB_PRECOND_AMG: z = M^-1 r is one V-cycle on the block r (amg_cycle at width kp: every matrix of the hierarchy is
 * streamed once for all columns, each column with the bits of the single-column cycle), so z is a block of its
 * own and an iteration is SpMM, k_amg_mrhs_update_xr, the cycle, k_amg_mrhs_update_p: the fine level's last
 * sweep leaves (r.z, r.r) of every column, there is no dot-product launch.  The cycle is gated on `running`
 * like the SpMM; the restart of opts.verify runs one un-gated cycle on r = b - S x.
 *
 * LSB_PRECOND_FSAI with opts.fsai_blocks: z = G^T (G r) is a block of its own as well, and the x / r sweep rides in the
 * two products (hip_mrhs_fsai.hip): an iteration is SpMM, k_mrhs_fsai_xr_gr (alpha, x, t = G r' with r' formed in the
 * gather), k_mrhs_fsai_gt_dots (z = G^T t, r' stored in place, the records of (r.z, r.r)), k_amg_mrhs_update_p.  There
 * is ONE residual block: init, a warm start and a verify restart write it and run the two products un-gated as SpMMs
 * off G and G^T where the AMG branch runs its cycle.  Without opts.fsai_blocks such a solver answers 2 and
 * allocates nothing.
 *
 * Served: block_serves (hip_block.c) -- one shard in one process, fp64 values, krylov PCG or AUTO, precond JACOBI /
 * L1JACOBI / NONE / AMG, and FSAI where opts.fsai_blocks is set.
 * Every other solver answers 2: nothing falls back to a loop of single solves.  An AMG solver smoothed by multicolour
 * Gauss-Seidel is not served either -- its cycle is not built on blocks -- but its SpMM is (block_spmm_serves).
 */
static int mrhs_amg(const lsb_hip_solver *sv) { return sv->o.precond == LSB_PRECOND_AMG; }

static struct mrhs_work *mrhs_setup(lsb_hip_solver *sv, unsigned kp) {
  struct mrhs_work *w = &sv->mr[kp == 2 ? 0 : kp == 4 ? 1 : 2];
  if (w->blk.kp)
    return w;
  if (!sv->mr_hst)
    LSB_CHK_HIP(hipHostMalloc((void **)&sv->mr_hst, 2 * sizeof(struct lsb_mrhs_state), 0));
  /* behind the blocks (FSAI: z and t are two of them): the records of the SpMM and of the sweeps, then the state */
  const size_t ppq = (size_t)LSB_MAX_PARTIALS * kp * sizeof(double);
  /* (an AMG or FSAI solver's records of (r.z, r.r) come from a row kernel's grid, not from a sweep's) */
  const size_t pp2 = (size_t)(block_zblock(sv) ? LSB_MAX_PARTIALS : LSB_STREAM_GRID_CAP) * 2 * kp * sizeof(double);
  const size_t stb = (sizeof(struct lsb_mrhs_state) + 255) & ~(size_t)255;
  char *behind = block_work_slab(sv, &w->blk, kp, block_fsai(sv) ? 7 : 5, ppq + pp2 + stb);
  w->parts_pq = (double *)behind;
  w->parts2 = (double *)(behind + ppq);
  w->st = (struct lsb_mrhs_state *)(behind + ppq + pp2);
  if (mrhs_amg(sv) && block_serves(sv)) /* z and the blocks of the cycle's vectors (not under mcgs: the SpMM alone) */
    block_work_z(sv, &w->blk, 0);
  return w;
}

void mrhs_free(lsb_hip_solver *sv) {
  for (int k = 0; k < 3; k++) {
    block_work_free(&sv->mr[k].blk);
    lsb_hip_free(sv->mr[k].parts_bb);
    memset(&sv->mr[k], 0, sizeof sv->mr[k]);
  }
  if (sv->mr_hst)
    LSB_CHK_HIP(hipHostFree(sv->mr_hst));
  sv->mr_hst = NULL;
}

/* Bytes one iteration of a batch of nrhs columns must move: the CSR arrays once whatever the width (12 B per
 * non-zero + the row offsets), the SpMM's x in and y out and the 9 passes of the classic form's sweeps per
 * column, the inverse diagonal once per sweep for all columns where it is a vector. */
unsigned long long lsb_hip_solver_multi_iteration_bytes(const lsb_hip_solver *sv, unsigned nrhs) {
  if (!sv || nrhs == 0 || !block_serves(sv) || mrhs_amg(sv)) /* (a V-cycle has another shape) */
    return 0;
  const struct shard *s = &sv->sh[0];
  const unsigned kp = nrhs == 1 ? 1u : block_width(nrhs > LSB_MRHS_MAX ? LSB_MRHS_MAX : nrhs);
  /* FSAI on blocks: S, G and G^T once each whatever the width, and 16 vector passes per column -- the SpMM 2 (p in,
   * q out); k_mrhs_fsai_xr_gr 6 (q and r gathered, p and x of the own rows in, x and t out); k_mrhs_fsai_gt_dots 5 (t
   * gathered, q and r of the own rows in, r and z out); k_amg_mrhs_update_p 3 (z and p in, p out) */
  if (block_fsai(sv))
    return 12ull * (s->nnz + s->fs_g.nnz + s->fs_gt.nnz) + 12ull * (s->n + 1ull) + 8ull * s->n * 16ull * kp;
  return 12ull * s->nnz + 4ull * (s->n + 1ull) + 8ull * s->n * (11ull * kp + (s->dinv_uniform ? 0u : 2u));
}

/* Iterations per host poll: run_chunk on this iteration's bytes; even, so that a chunk leaves the parity where it
 * found it.  An AMG solver: the same rule on an estimate of the SpMM, the sweeps and the cycle (its matrices once
 * per launch that streams them, its vector passes per column), at least 2 where the diagonal preconditioners keep
 * 8 -- an AMG iteration of a large grid is milliseconds and a solve a few dozen of them, so a speculative chunk of
 * 8 would be a noticeable part of it. */
static int mrhs_chunk(const lsb_hip_solver *sv, unsigned kp) {
  if (sv->o.check_every > 0)
    return (sv->o.check_every + 1) & ~1;
  const struct shard *s = &sv->sh[0];
  const int amg = mrhs_amg(sv);
  double bytes = (double)lsb_hip_solver_multi_iteration_bytes(sv, kp);
  if (amg)
    bytes = (double)(12ull * s->nnz + s->amg->cycle_mat_bytes + 8ull * kp * (11ull * s->n + s->amg->cycle_vec_rows));
  return run_chunk(bytes, 6.0, amg ? 2 : 8, 256) & ~1;
}

static void spmm_shard(lsb_hip_solver *sv, struct mrhs_work *w, const double *x, double *y, const double *bres,
                       unsigned *npq, const struct lsb_mrhs_state *st) {
  const struct shard *s = &sv->sh[0];
  lsb_k_spmm_csr(w->blk.kp, s->n, s->csr.offs, s->csr.cols, s->csr.vals, sv->mr_lanes, x, y, bres, w->parts_pq, npq,
                 st, g_stream);
}

/* z = M^-1 r of every column, un-gated: the V-cycle, or FSAI's two products.  The records of x.y of those two, which
 * nobody reads, go into parts2: every caller's next launch writes that anew, while parts_pq may still hold a verify
 * round's residual norms for the launches behind this one */
static void mrhs_zapply(const lsb_hip_solver *sv, const struct mrhs_work *w) {
  block_zapply(sv, &w->blk, w->blk.r, w->parts2);
}

static void mrhs_enqueue_iter(lsb_hip_solver *sv, struct mrhs_work *w, int parity) {
  const struct shard *s = &sv->sh[0];
  const struct block_work *k = &w->blk;
  unsigned npq = 0, np2 = 0;
  spmm_shard(sv, w, k->p, k->q, NULL, &npq, w->st);
  if (block_fsai(sv)) {
    lsb_k_mrhs_fsai_xr_gr(k->kp, s->n, s->fs_g.offs, s->fs_g.cols, s->fs_g.vals, block_fsai_lanes(sv, &s->fs_g), k->p,
                          k->q, k->x, k->r, k->t, w->st, parity, w->parts_pq, npq, g_stream);
    lsb_k_mrhs_fsai_gt_dots(k->kp, s->n, s->fs_gt.offs, s->fs_gt.cols, s->fs_gt.vals, block_fsai_lanes(sv, &s->fs_gt),
                            k->t, k->q, k->r, k->z, w->parts2, &np2, w->st, parity, g_stream);
    lsb_k_amg_mrhs_update_p(k->kp, s->n, k->z, k->p, w->st, parity, w->parts2, np2, g_stream);
    return;
  }
  if (mrhs_amg(sv)) {
    lsb_k_amg_mrhs_update_xr(k->kp, s->n, k->p, k->q, k->x, k->r, w->st, parity, w->parts_pq, npq, g_stream);
    /* the cycle gated on `running`, its last sweep leaving the records of (r.z, r.r) */
    const struct amg_run c = {.a = s->amg, .vec = k->av, .kp = k->kp, .r = k->r, .z = k->z,
                              .records = w->parts2, .nrecords = &np2, .mst = w->st};
    amg_cycle(&c);
    lsb_k_amg_mrhs_update_p(k->kp, s->n, k->z, k->p, w->st, parity, w->parts2, np2, g_stream);
    return;
  }
  lsb_k_mrhs_update_xr(k->kp, s->n, k->p, k->q, DINV(s), k->x, k->r, w->st, parity, w->parts_pq, npq, w->parts2, &np2,
                       g_stream);
  lsb_k_mrhs_update_p(k->kp, s->n, k->r, DINV(s), k->p, w->st, parity, w->parts2, np2, g_stream);
}

/* what block_enqueue runs for run_loop */
struct mrhs_enq {
  lsb_hip_solver *sv;
  struct mrhs_work *w;
};
static void mrhs_enqueue_iters(void *ctx, int iters) {
  const struct mrhs_enq *e = ctx;
  for (int i = 0; i < iters; i++)
    mrhs_enqueue_iter(e->sv, e->w, i & 1);
}

/* Enqueue iterations until no column is running; the final state lands in mr_hst[0] (whose nspmm the caller cleared
 * for the solve proper).  *hint: the launches this stretch of the previous batch took. */
static void mrhs_run(lsb_hip_solver *sv, struct mrhs_work *w, unsigned *hint) {
  struct mrhs_enq e = {sv, w};
  struct block_enq be = {sv, &w->blk, mrhs_enqueue_iters, &e};
  const struct run_loop r = {.name = "a batch of right-hand sides", .d_state = w->st, .h_state = sv->mr_hst,
                             .state_bytes = sizeof(struct lsb_mrhs_state),
                             .stop_off = offsetof(struct lsb_mrhs_state, running), .stop_is_running = 1,
                             .progress_off = offsetof(struct lsb_mrhs_state, nspmm),
                             .enqueue = block_enqueue, .ctx = &be, .chunk = mrhs_chunk(sv, w->blk.kp), .even = 1,
                             .max_piece = sv->o.use_graph ? 1024 : 0, .cap = -1,
                             .what_hinted = "poll of a hinted batch", .what_poll = "poll of the batch",
                             .what_drain = "drain after the batch"};
  run_loop(sv, &r, hint);
}

/* one batch: nb <= 8 columns of the caller's blocks; start != NULL: from the X0 that d_X holds, and where the
 * columns' starting residuals go */
static void mrhs_batch(lsb_hip_solver *sv, unsigned nb, const double *d_B, size_t ldb, double *d_X, size_t ldx,
                       struct lsb_hip_result *res, double *start) {
  struct mrhs_work *w = mrhs_setup(sv, block_width(nb));
  const struct shard *s = &sv->sh[0];
  struct lsb_mrhs_state *hst = sv->mr_hst;
  const struct block_work *k = &w->blk;
  const unsigned kp = k->kp, n = s->n;
  unsigned np2 = 0, npq = 0, nverify = 0;
  const double t0 = wall_seconds();
  lsb_k_mrhs_pack(n, kp, nb, sv->d_perm, d_B, ldb, k->b, g_stream);
  if (start) {
    /* The batch's state lives on the device, with b.b and the threshold per column, so a start from X0 is no
     * correction solve: x = X0, r = b - S x0 by the SpMM of a verify round, p = M^-1 r through the un-gated
     * cycle or the diagonal, and a state from scratch in which the columns that start within the tolerance (or
     * have b = 0: their x is zeroed) are frozen.  A column with x0 = 0 gets the bits of the branch below. */
    unsigned nbb = 0;
    if (!w->parts_bb)
      w->parts_bb = (double *)lsb_hip_malloc((size_t)LSB_STREAM_GRID_CAP * 2 * kp * sizeof(double));
    lsb_k_mrhs_pack(n, kp, nb, sv->d_perm, d_X, ldx, k->x, g_stream);
    lsb_k_mrhs_x0_bb(kp, n, k->b, w->parts_bb, &nbb, g_stream);
    spmm_shard(sv, w, k->x, k->r, k->b, &npq, NULL);
    if (block_zblock(sv)) {
      lsb_k_amg_mrhs_x0_start(kp, n, k->x, w->parts_bb, nbb, g_stream);
      mrhs_zapply(sv, w);
      lsb_k_amg_mrhs_init_p(kp, n, k->r, k->z, k->p, w->parts2, &np2, g_stream);
    } else
      lsb_k_mrhs_x0_start(kp, n, k->r, DINV(s), k->x, k->p, w->parts_bb, nbb, w->parts2, &np2, g_stream);
    lsb_k_mrhs_init_state(kp, w->st, w->parts2, np2, w->parts_bb, nbb, sv->o.tol, (int)sv->o.maxit, g_stream);
  } else {
    if (block_zblock(sv)) { /* x = 0, r = b ; z = M^-1 b ; p = z and (b.z, b.b) */
      lsb_k_amg_mrhs_init(kp, n, k->b, k->x, k->r, g_stream);
      mrhs_zapply(sv, w);
      lsb_k_amg_mrhs_init_p(kp, n, k->b, k->z, k->p, w->parts2, &np2, g_stream);
    } else
      lsb_k_mrhs_init(kp, n, k->b, DINV(s), k->x, k->r, k->p, w->parts2, &np2, g_stream);
    lsb_k_mrhs_init_state(kp, w->st, w->parts2, np2, NULL, 0, sv->o.tol, (int)sv->o.maxit, g_stream);
  }
  hst[0].nspmm = 0;
  for (int round = 0;; round++) {
    mrhs_run(sv, w, hint_slot(w->hint, round));
    if (!(sv->o.verify && sv->o.tol > 0.0))
      break;
    int any = 0;
    for (unsigned c = 0; c < nb; c++)
      any |= hst[0].c[c].status == LSB_STATUS_CONVERGED && hst[0].c[c].bb > 0.0;
    if (!any)
      break;
    /* "converged" is reported only for the residual RECOMPUTED from x */
    const int more = round < LSB_MAX_CORRECTIONS;
    spmm_shard(sv, w, k->x, k->q, k->b, &npq, NULL);
    if (block_zblock(sv)) { /* r = b - S x, z = M^-1 r, p = z and r.z, for the restarting columns */
      lsb_k_amg_mrhs_restart_r(kp, n, k->q, k->r, w->st, w->parts_pq, npq, more, g_stream);
      mrhs_zapply(sv, w);
      lsb_k_amg_mrhs_restart_p(kp, n, k->r, k->z, k->p, w->st, w->parts_pq, npq, more, w->parts2, &np2, g_stream);
    } else
      lsb_k_mrhs_restart(kp, n, k->q, DINV(s), k->r, k->p, w->st, w->parts_pq, npq, more, w->parts2, &np2, g_stream);
    lsb_k_mrhs_restart_state(kp, w->st, w->parts_pq, npq, w->parts2, np2, more, g_stream);
    nverify++;
    LSB_CHK_HIP(hipMemcpyAsync(&hst[0], w->st, sizeof hst[0], hipMemcpyDeviceToHost, g_stream));
    drain_stream(sv, "recomputed residuals of the batch");
    if (!hst[0].running)
      break;
  }
  lsb_k_mrhs_unpack(n, kp, nb, sv->d_perm, k->x, d_X, ldx, g_stream);
  drain_stream(sv, "un-packing the batch");
  const double seconds = wall_seconds() - t0;
  for (unsigned c = 0; c < nb; c++) {
    struct lsb_hip_result r;
    memset(&r, 0, sizeof r);
    result_from_state(&r, &hst[0].c[c]);
    r.true_relres = hst[0].true_relres[c];
    if (r.true_relres >= 0.0)
      r.relres = r.true_relres;
    r.corrections = (unsigned)hst[0].corrections[c];
    r.seconds = seconds;
    r.spmvs = (unsigned)hst[0].nspmm + nverify + (start ? 1u : 0u);
    res[c] = r;
    if (start)
      start[c] = hst[0].start_relres[c];
  }
}

static int solve_multi_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_B, size_t ldb, double *d_X, size_t ldx,
                           struct lsb_hip_result *res, int warm) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, 0, d_B, ldb, d_X, ldx) || !block_serves(sv))
    return 2;
  if (nrhs == 1)
    return warm ? lsb_hip_solver_solve_x0_dev(sv, d_B, d_X, res) : lsb_hip_solver_solve_dev(sv, d_B, d_X, res);
  struct lsb_hip_result *tmp = res ? res : lsb_calloc(struct lsb_hip_result, nrhs);
  double *start = warm ? start_relres_slots(sv, nrhs) : NULL;
  if (!warm)
    sv->start_n = 0;
  for (unsigned c0 = 0; c0 < nrhs; c0 += LSB_MRHS_MAX) {
    const unsigned nb = nrhs - c0 < LSB_MRHS_MAX ? nrhs - c0 : LSB_MRHS_MAX;
    mrhs_batch(sv, nb, d_B + (size_t)c0 * ldb, ldb, d_X + (size_t)c0 * ldx, ldx, tmp + c0, warm ? start + c0 : NULL);
  }
  g_last = tmp[nrhs - 1];
  if (!res)
    free(tmp);
  return 0;
}

int lsb_hip_solver_solve_multi_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_B, size_t ldb, double *d_X,
                                   size_t ldx, struct lsb_hip_result *res) {
  return solve_multi_dev(sv, nrhs, d_B, ldb, d_X, ldx, res, 0);
}

int lsb_hip_solver_solve_multi_x0_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_B, size_t ldb, double *d_X,
                                      size_t ldx, struct lsb_hip_result *res) {
  return solve_multi_dev(sv, nrhs, d_B, ldb, d_X, ldx, res, 1);
}

int lsb_hip_solver_solve_multi(lsb_hip_solver *sv, unsigned nrhs, const double *B, size_t ldb, double *X, size_t ldx,
                               struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, 0, B, ldb, X, ldx) || !block_serves(sv))
    return 2;
  return block_solve_host(lsb_hip_solver_solve_multi_dev, 1, sv, nrhs, B, ldb, X, ldx, res); /* X: whatever it answers */
}

/* Y = Op X: the SpMM of the iteration on its own, through the same pack / unpack */
int lsb_hip_solver_spmm_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_X, size_t ldx, double *d_Y,
                            size_t ldy) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, 0, d_X, ldx, d_Y, ldy) || !block_spmm_serves(sv))
    return 2;
  const struct shard *s = &sv->sh[0];
  for (unsigned c0 = 0; c0 < nrhs; c0 += LSB_MRHS_MAX) {
    const unsigned nb = nrhs - c0 < LSB_MRHS_MAX ? nrhs - c0 : LSB_MRHS_MAX;
    struct mrhs_work *w = mrhs_setup(sv, block_width(nb));
    unsigned npq = 0;
    lsb_k_mrhs_pack(s->n, w->blk.kp, nb, sv->d_perm, d_X + (size_t)c0 * ldx, ldx, w->blk.p, g_stream);
    spmm_shard(sv, w, w->blk.p, w->blk.q, NULL, &npq, NULL);
    lsb_k_mrhs_unpack(s->n, w->blk.kp, nb, sv->d_perm, w->blk.q, d_Y + (size_t)c0 * ldy, ldy, g_stream);
  }
  drain_stream(sv, "lsb_hip_solver_spmm_dev");
  return 0;
}

/* Z_c = M^-1 R_c, one V-cycle per column of the block -- or FSAI's two products -- through the same pack / unpack:
 * the preconditioner of an iteration on its own, un-gated.  A solver that solve_multi does not serve under AMG or
 * FSAI answers 2. */
int lsb_hip_solver_precond_multi_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_R, size_t ldr, double *d_Z,
                                     size_t ldz) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, 0, d_R, ldr, d_Z, ldz) || !block_serves(sv) || !block_zblock(sv))
    return 2;
  const struct shard *s = &sv->sh[0];
  for (unsigned c0 = 0; c0 < nrhs; c0 += LSB_MRHS_MAX) {
    const unsigned nb = nrhs - c0 < LSB_MRHS_MAX ? nrhs - c0 : LSB_MRHS_MAX;
    struct mrhs_work *w = mrhs_setup(sv, block_width(nb));
    lsb_k_mrhs_pack(s->n, w->blk.kp, nb, sv->d_perm, d_R + (size_t)c0 * ldr, ldr, w->blk.r, g_stream);
    mrhs_zapply(sv, w);
    lsb_k_mrhs_unpack(s->n, w->blk.kp, nb, sv->d_perm, w->blk.z, d_Z + (size_t)c0 * ldz, ldz, g_stream);
  }
  drain_stream(sv, "lsb_hip_solver_precond_multi_dev");
  return 0;
}

/* entries of G and of G^T of an FSAI solver (what lsb_hip_solver_multi_iteration_bytes counts); 2 for any other */
int lsb_hip_solver_fsai_nnz(const lsb_hip_solver *sv, unsigned long long *g, unsigned long long *gt) {
  if (!sv || sv->o.precond != LSB_PRECOND_FSAI || !sv->sh[0].fs_g.offs)
    return 2;
  if (g)
    *g = sv->sh[0].fs_g.nnz;
  if (gt)
    *gt = sv->sh[0].fs_gt.nnz;
  return 0;
}
