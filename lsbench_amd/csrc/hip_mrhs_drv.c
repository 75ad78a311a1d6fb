/* Several right-hand sides: host driver (kernels: hip_mrhs.hip, hip_mrhs_x0.hip, hip_mrhs_amg.hip, hip_mrhs_fsai.hip). */
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
 * Served: one shard in one process, fp64 values, krylov PCG or AUTO, precond JACOBI / L1JACOBI / NONE / AMG, and FSAI
 * where opts.fsai_blocks is set.
 * Every other solver answers 2: nothing falls back to a loop of single solves.  An AMG solver smoothed by multicolour
 * Gauss-Seidel is not served either -- its cycle is not built on blocks -- but its SpMM is (spmm_serves).
 */
static int mrhs_mcgs(const lsb_hip_solver *sv) {
  return sv->o.precond == LSB_PRECOND_AMG && sv->sh[0].amg && sv->sh[0].amg->mcgs;
}

static int spmm_serves(const lsb_hip_solver *sv) {
  const struct lsb_hip_opts *o = &sv->o;
  return !sv->multi && sv->nshard == 1 && !sv->dist && o->precision == LSB_PREC_FP64 &&
         (o->krylov == LSB_KRYLOV_PCG || o->krylov == LSB_KRYLOV_AUTO) &&
         (o->precond == LSB_PRECOND_JACOBI || o->precond == LSB_PRECOND_L1JACOBI ||
          o->precond == LSB_PRECOND_NONE ||
          (o->precond == LSB_PRECOND_AMG && sv->sh[0].amg && sv->sh[0].amg->prec == LSB_AMG_PREC_FP64) ||
          (o->precond == LSB_PRECOND_FSAI && o->fsai_blocks && sv->sh[0].fs_g.offs && sv->sh[0].fs_gt.offs)) &&
         o->persistent <= 0 && !sv->ps.use && (unsigned long long)sv->sh[0].n * LSB_MRHS_MAX < (1ull << 32);
}

static int mrhs_serves(const lsb_hip_solver *sv) { return spmm_serves(sv) && !mrhs_mcgs(sv); }

static int mrhs_amg(const lsb_hip_solver *sv) { return sv->o.precond == LSB_PRECOND_AMG; }

static int mrhs_fsai(const lsb_hip_solver *sv) { return sv->o.precond == LSB_PRECOND_FSAI; }

/* z is a block of its own, written between the x / r update and lsb_k_amg_mrhs_update_p */
static int mrhs_zblock(const lsb_hip_solver *sv) { return mrhs_amg(sv) || mrhs_fsai(sv); }

static unsigned batch_width(unsigned nrhs) { return nrhs <= 2 ? 2u : nrhs <= 4 ? 4u : 8u; }

static void mrhs_lanes_init(lsb_hip_solver *sv) {
  /* lanes per row of the SpMM: the shard's (from its mean row length); LSBENCH_HIP_MRHS_LANES is the A/B switch */
  const char *e = getenv("LSBENCH_HIP_MRHS_LANES");
  sv->mr_lanes = e && atoi(e) > 0 ? (unsigned)atoi(e) : sv->sh[0].lanes;
  /* ... of G and of G^T under FSAI: each matrix's own; LSBENCH_HIP_MRHS_FSAI_LANES is the A/B switch for both (the
   * single-column kernels never see it) */
  e = getenv("LSBENCH_HIP_MRHS_FSAI_LANES");
  sv->mr_fs_lanes = e && atoi(e) > 0 ? (unsigned)atoi(e) : 0;
}

/* for the block-CG driver (hip_bcg_drv.c) */
int mrhs_serves_diag(const lsb_hip_solver *sv) { return mrhs_serves(sv) && !mrhs_zblock(sv); }
unsigned mrhs_batch_width(unsigned nrhs) { return batch_width(nrhs); }
unsigned mrhs_spmm_lanes(lsb_hip_solver *sv) {
  if (!sv->mr_hst) /* (mrhs_setup has not run: the same rule, nothing allocated) */
    mrhs_lanes_init(sv);
  return sv->mr_lanes;
}

static struct mrhs_work *mrhs_setup(lsb_hip_solver *sv, unsigned kp) {
  struct mrhs_work *w = &sv->mr[kp == 2 ? 0 : kp == 4 ? 1 : 2];
  if (w->kp)
    return w;
  const struct shard *s = &sv->sh[0];
  if (!sv->mr_hst) {
    LSB_CHK_HIP(hipHostMalloc((void **)&sv->mr_hst, 2 * sizeof(struct lsb_mrhs_state), 0));
    mrhs_lanes_init(sv);
  }
  /* 256-byte aligned pieces of one allocation, the blocks first: their placement relative to one another is
   * the same in every solver */
  const size_t blk = (((size_t)s->n * kp * sizeof(double)) + 255) & ~(size_t)255;
  const size_t ppq = (size_t)LSB_MAX_PARTIALS * kp * sizeof(double);
  /* (an AMG or FSAI solver's records of (r.z, r.r) come from a row kernel's grid, not from a sweep's) */
  const size_t pp2 = (size_t)(mrhs_zblock(sv) ? LSB_MAX_PARTIALS : LSB_STREAM_GRID_CAP) * 2 * kp * sizeof(double);
  const size_t nblk = mrhs_fsai(sv) ? 7 : 5; /* FSAI: z and t behind the five */
  const size_t stb = (sizeof(struct lsb_mrhs_state) + 255) & ~(size_t)255;
  w->mem = (char *)lsb_hip_malloc(nblk * blk + ppq + pp2 + stb);
  LSB_CHK_HIP(hipMemsetAsync(w->mem, 0, nblk * blk + ppq + pp2 + stb, g_stream));
  w->b = (double *)w->mem, w->x = (double *)(w->mem + blk), w->r = (double *)(w->mem + 2 * blk);
  w->p = (double *)(w->mem + 3 * blk), w->q = (double *)(w->mem + 4 * blk);
  w->parts_pq = (double *)(w->mem + nblk * blk);
  w->parts2 = (double *)(w->mem + nblk * blk + ppq);
  w->st = (struct lsb_mrhs_state *)(w->mem + nblk * blk + ppq + pp2);
  if (mrhs_fsai(sv))
    w->z = (double *)(w->mem + 5 * blk), w->t = (double *)(w->mem + 6 * blk);
  if (mrhs_amg(sv) && !mrhs_mcgs(sv)) { /* z and the blocks of the cycle's vectors */
    w->av = lsb_calloc(struct amg_vecs, s->amg->nlev);
    w->amg_mem = amg_block_vecs(s->amg, kp, w->av);
    w->z = (double *)w->amg_mem;
  }
  w->kp = kp;
  return w;
}

void mrhs_free(lsb_hip_solver *sv) {
  for (int k = 0; k < 3; k++) {
    graph_drop(&sv->mr[k].g);
    lsb_hip_free(sv->mr[k].mem), lsb_hip_free(sv->mr[k].amg_mem), lsb_hip_free(sv->mr[k].parts_bb);
    free(sv->mr[k].av);
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
  if (!sv || nrhs == 0 || !mrhs_serves(sv) || mrhs_amg(sv)) /* (a V-cycle has another shape) */
    return 0;
  const struct shard *s = &sv->sh[0];
  const unsigned kp = nrhs == 1 ? 1u : batch_width(nrhs > LSB_MRHS_MAX ? LSB_MRHS_MAX : nrhs);
  /* FSAI on blocks: S, G and G^T once each whatever the width, and 16 vector passes per column -- the SpMM 2 (p in,
   * q out); k_mrhs_fsai_xr_gr 6 (q and r gathered, p and x of the own rows in, x and t out); k_mrhs_fsai_gt_dots 5 (t
   * gathered, q and r of the own rows in, r and z out); k_amg_mrhs_update_p 3 (z and p in, p out) */
  if (mrhs_fsai(sv))
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

/* Z = one V-cycle on the block R of this width (records, nrecords, st: struct amg_run's) */
static void mrhs_cycle(const lsb_hip_solver *sv, const struct mrhs_work *w, double *records, unsigned *nrecords,
                       const struct lsb_mrhs_state *st) {
  const struct amg_run c = {.a = sv->sh[0].amg, .vec = w->av, .kp = w->kp, .r = w->r, .z = w->z,
                            .records = records, .nrecords = nrecords, .mst = st};
  amg_cycle(&c);
}

static void spmm_shard(lsb_hip_solver *sv, struct mrhs_work *w, const double *x, double *y, const double *bres,
                       unsigned *npq, const struct lsb_mrhs_state *st) {
  const struct shard *s = &sv->sh[0];
  lsb_k_spmm_csr(w->kp, s->n, s->csr.offs, s->csr.cols, s->csr.vals, sv->mr_lanes, x, y, bres, w->parts_pq, npq, st,
                 g_stream);
}

static unsigned fs_lanes(const lsb_hip_solver *sv, const struct fsai_csr *c) {
  return sv->mr_fs_lanes ? sv->mr_fs_lanes : c->lanes;
}

/* for the preconditioned half of the block-CG driver: solve_multi's service rule where z is a block of its own, and the
 * lanes per row of G (gt = 0) or of G^T */
int mrhs_serves_zblock(const lsb_hip_solver *sv) { return mrhs_serves(sv) && mrhs_zblock(sv); }
unsigned mrhs_fsai_lanes(lsb_hip_solver *sv, int gt) {
  if (!sv->mr_hst)
    mrhs_lanes_init(sv);
  return fs_lanes(sv, gt ? &sv->sh[0].fs_gt : &sv->sh[0].fs_g);
}

/* Z = G^T (G R) of this width, un-gated: two SpMMs off the factor's CSRs.  Their records of x.y, which nobody reads,
 * go into parts2: every caller's next launch writes that anew, while parts_pq may still hold a verify round's
 * residual norms for the launches behind this one */
static void mrhs_fsai_apply(const lsb_hip_solver *sv, const struct mrhs_work *w) {
  const struct shard *s = &sv->sh[0];
  unsigned np = 0;
  lsb_k_spmm_csr(w->kp, s->n, s->fs_g.offs, s->fs_g.cols, s->fs_g.vals, fs_lanes(sv, &s->fs_g), w->r, w->t, NULL,
                 w->parts2, &np, NULL, g_stream);
  lsb_k_spmm_csr(w->kp, s->n, s->fs_gt.offs, s->fs_gt.cols, s->fs_gt.vals, fs_lanes(sv, &s->fs_gt), w->t, w->z, NULL,
                 w->parts2, &np, NULL, g_stream);
}

/* z = M^-1 r of every column, un-gated: the V-cycle, or FSAI's two products */
static void mrhs_zapply(const lsb_hip_solver *sv, const struct mrhs_work *w) {
  if (mrhs_fsai(sv))
    mrhs_fsai_apply(sv, w);
  else
    mrhs_cycle(sv, w, NULL, NULL, NULL);
}

static void mrhs_enqueue_iter(lsb_hip_solver *sv, struct mrhs_work *w, int parity) {
  const struct shard *s = &sv->sh[0];
  unsigned npq = 0, np2 = 0;
  spmm_shard(sv, w, w->p, w->q, NULL, &npq, w->st);
  if (mrhs_fsai(sv)) {
    lsb_k_mrhs_fsai_xr_gr(w->kp, s->n, s->fs_g.offs, s->fs_g.cols, s->fs_g.vals, fs_lanes(sv, &s->fs_g), w->p, w->q,
                          w->x, w->r, w->t, w->st, parity, w->parts_pq, npq, g_stream);
    lsb_k_mrhs_fsai_gt_dots(w->kp, s->n, s->fs_gt.offs, s->fs_gt.cols, s->fs_gt.vals, fs_lanes(sv, &s->fs_gt), w->t,
                            w->q, w->r, w->z, w->parts2, &np2, w->st, parity, g_stream);
    lsb_k_amg_mrhs_update_p(w->kp, s->n, w->z, w->p, w->st, parity, w->parts2, np2, g_stream);
    return;
  }
  if (mrhs_amg(sv)) {
    lsb_k_amg_mrhs_update_xr(w->kp, s->n, w->p, w->q, w->x, w->r, w->st, parity, w->parts_pq, npq, g_stream);
    mrhs_cycle(sv, w, w->parts2, &np2, w->st);
    lsb_k_amg_mrhs_update_p(w->kp, s->n, w->z, w->p, w->st, parity, w->parts2, np2, g_stream);
    return;
  }
  lsb_k_mrhs_update_xr(w->kp, s->n, w->p, w->q, DINV(s), w->x, w->r, w->st, parity, w->parts_pq, npq, w->parts2,
                       &np2, g_stream);
  lsb_k_mrhs_update_p(w->kp, s->n, w->r, DINV(s), w->p, w->st, parity, w->parts2, np2, g_stream);
}

/* what run_loop enqueues: one linear chain on internal buffers, so its graphs are keyed on the count alone */
struct mrhs_enq {
  lsb_hip_solver *sv;
  struct mrhs_work *w;
};
static void mrhs_enqueue_iters(void *ctx, int iters) {
  const struct mrhs_enq *e = ctx;
  for (int i = 0; i < iters; i++)
    mrhs_enqueue_iter(e->sv, e->w, i & 1);
}
static void mrhs_enqueue(void *ctx, int iters) {
  const struct mrhs_enq *e = ctx;
  if (e->sv->o.use_graph)
    graph_launch(&e->w->g, iters, NULL, mrhs_enqueue_iters, ctx);
  else
    mrhs_enqueue_iters(ctx, iters);
}

/* Enqueue iterations until no column is running; the final state lands in mr_hst[0] (whose nspmm the caller cleared
 * for the solve proper).  *hint: the launches this stretch of the previous batch took. */
static void mrhs_run(lsb_hip_solver *sv, struct mrhs_work *w, unsigned *hint) {
  struct mrhs_enq e = {sv, w};
  const struct run_loop r = {.name = "a batch of right-hand sides", .d_state = w->st, .h_state = sv->mr_hst,
                             .state_bytes = sizeof(struct lsb_mrhs_state),
                             .stop_off = offsetof(struct lsb_mrhs_state, running), .stop_is_running = 1,
                             .progress_off = offsetof(struct lsb_mrhs_state, nspmm),
                             .enqueue = mrhs_enqueue, .ctx = &e, .chunk = mrhs_chunk(sv, w->kp), .even = 1,
                             .max_piece = sv->o.use_graph ? 1024 : 0, .cap = -1,
                             .what_hinted = "poll of a hinted batch", .what_poll = "poll of the batch",
                             .what_drain = "drain after the batch"};
  run_loop(sv, &r, hint);
}

/* one batch: nb <= 8 columns of the caller's blocks; start != NULL: from the X0 that d_X holds, and where the
 * columns' starting residuals go */
static void mrhs_batch(lsb_hip_solver *sv, unsigned nb, const double *d_B, size_t ldb, double *d_X, size_t ldx,
                       struct lsb_hip_result *res, double *start) {
  struct mrhs_work *w = mrhs_setup(sv, batch_width(nb));
  const struct shard *s = &sv->sh[0];
  struct lsb_mrhs_state *hst = sv->mr_hst;
  const unsigned kp = w->kp, n = s->n;
  unsigned np2 = 0, npq = 0, nverify = 0;
  const double t0 = wall_seconds();
  lsb_k_mrhs_pack(n, kp, nb, sv->d_perm, d_B, ldb, w->b, g_stream);
  if (start) {
    /* The batch's state lives on the device, with b.b and the threshold per column, so a start from X0 is no
     * correction solve: x = X0, r = b - S x0 by the SpMM of a verify round, p = M^-1 r through the un-gated
     * cycle or the diagonal, and a state from scratch in which the columns that start within the tolerance (or
     * have b = 0: their x is zeroed) are frozen.  A column with x0 = 0 gets the bits of the branch below. */
    unsigned nbb = 0;
    if (!w->parts_bb)
      w->parts_bb = (double *)lsb_hip_malloc((size_t)LSB_STREAM_GRID_CAP * 2 * kp * sizeof(double));
    lsb_k_mrhs_pack(n, kp, nb, sv->d_perm, d_X, ldx, w->x, g_stream);
    lsb_k_mrhs_x0_bb(kp, n, w->b, w->parts_bb, &nbb, g_stream);
    spmm_shard(sv, w, w->x, w->r, w->b, &npq, NULL);
    if (mrhs_zblock(sv)) {
      lsb_k_amg_mrhs_x0_start(kp, n, w->x, w->parts_bb, nbb, g_stream);
      mrhs_zapply(sv, w);
      lsb_k_amg_mrhs_init_p(kp, n, w->r, w->z, w->p, w->parts2, &np2, g_stream);
    } else
      lsb_k_mrhs_x0_start(kp, n, w->r, DINV(s), w->x, w->p, w->parts_bb, nbb, w->parts2, &np2, g_stream);
    lsb_k_mrhs_init_state(kp, w->st, w->parts2, np2, w->parts_bb, nbb, sv->o.tol, (int)sv->o.maxit, g_stream);
  } else {
    if (mrhs_zblock(sv)) { /* x = 0, r = b ; z = M^-1 b ; p = z and (b.z, b.b) */
      lsb_k_amg_mrhs_init(kp, n, w->b, w->x, w->r, g_stream);
      mrhs_zapply(sv, w);
      lsb_k_amg_mrhs_init_p(kp, n, w->b, w->z, w->p, w->parts2, &np2, g_stream);
    } else
      lsb_k_mrhs_init(kp, n, w->b, DINV(s), w->x, w->r, w->p, w->parts2, &np2, g_stream);
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
    spmm_shard(sv, w, w->x, w->q, w->b, &npq, NULL);
    if (mrhs_zblock(sv)) { /* r = b - S x, z = M^-1 r, p = z and r.z, for the restarting columns */
      lsb_k_amg_mrhs_restart_r(kp, n, w->q, w->r, w->st, w->parts_pq, npq, more, g_stream);
      mrhs_zapply(sv, w);
      lsb_k_amg_mrhs_restart_p(kp, n, w->r, w->z, w->p, w->st, w->parts_pq, npq, more, w->parts2, &np2, g_stream);
    } else
      lsb_k_mrhs_restart(kp, n, w->q, DINV(s), w->r, w->p, w->st, w->parts_pq, npq, more, w->parts2, &np2, g_stream);
    lsb_k_mrhs_restart_state(kp, w->st, w->parts_pq, npq, w->parts2, np2, more, g_stream);
    nverify++;
    LSB_CHK_HIP(hipMemcpyAsync(&hst[0], w->st, sizeof hst[0], hipMemcpyDeviceToHost, g_stream));
    drain_stream(sv, "recomputed residuals of the batch");
    if (!hst[0].running)
      break;
  }
  lsb_k_mrhs_unpack(n, kp, nb, sv->d_perm, w->x, d_X, ldx, g_stream);
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

static int multi_args_bad(const lsb_hip_solver *sv, unsigned nrhs, const void *a, size_t lda, const void *b,
                          size_t ldb) {
  return !sv || !a || !b || nrhs == 0 || lda < sv->n_user || ldb < sv->n_user;
}

static int solve_multi_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_B, size_t ldb, double *d_X, size_t ldx,
                           struct lsb_hip_result *res, int warm) {
  if (!lsb_initialized)
    return 1;
  if (multi_args_bad(sv, nrhs, d_B, ldb, d_X, ldx) || !mrhs_serves(sv))
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
  if (multi_args_bad(sv, nrhs, B, ldb, X, ldx) || !mrhs_serves(sv))
    return 2;
  const size_t n = sv->n_user, bytes = n * sizeof(double);
  double *d_B = (double *)lsb_hip_malloc(bytes * nrhs), *d_X = (double *)lsb_hip_malloc(bytes * nrhs);
  LSB_CHK_HIP(hipMemcpy2D(d_B, bytes, B, ldb * sizeof(double), bytes, nrhs, hipMemcpyHostToDevice));
  const int rc = lsb_hip_solver_solve_multi_dev(sv, nrhs, d_B, n, d_X, n, res);
  LSB_CHK_HIP(hipMemcpy2D(X, ldx * sizeof(double), d_X, bytes, bytes, nrhs, hipMemcpyDeviceToHost));
  lsb_hip_free(d_B), lsb_hip_free(d_X);
  return rc;
}

/* Y = Op X: the SpMM of the iteration on its own, through the same pack / unpack */
int lsb_hip_solver_spmm_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_X, size_t ldx, double *d_Y,
                            size_t ldy) {
  if (!lsb_initialized)
    return 1;
  if (multi_args_bad(sv, nrhs, d_X, ldx, d_Y, ldy) || !spmm_serves(sv))
    return 2;
  const struct shard *s = &sv->sh[0];
  for (unsigned c0 = 0; c0 < nrhs; c0 += LSB_MRHS_MAX) {
    const unsigned nb = nrhs - c0 < LSB_MRHS_MAX ? nrhs - c0 : LSB_MRHS_MAX;
    struct mrhs_work *w = mrhs_setup(sv, batch_width(nb));
    unsigned npq = 0;
    lsb_k_mrhs_pack(s->n, w->kp, nb, sv->d_perm, d_X + (size_t)c0 * ldx, ldx, w->p, g_stream);
    spmm_shard(sv, w, w->p, w->q, NULL, &npq, NULL);
    lsb_k_mrhs_unpack(s->n, w->kp, nb, sv->d_perm, w->q, d_Y + (size_t)c0 * ldy, ldy, g_stream);
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
  if (multi_args_bad(sv, nrhs, d_R, ldr, d_Z, ldz) || !mrhs_serves(sv) || !mrhs_zblock(sv))
    return 2;
  const struct shard *s = &sv->sh[0];
  for (unsigned c0 = 0; c0 < nrhs; c0 += LSB_MRHS_MAX) {
    const unsigned nb = nrhs - c0 < LSB_MRHS_MAX ? nrhs - c0 : LSB_MRHS_MAX;
    struct mrhs_work *w = mrhs_setup(sv, batch_width(nb));
    lsb_k_mrhs_pack(s->n, w->kp, nb, sv->d_perm, d_R + (size_t)c0 * ldr, ldr, w->r, g_stream);
    mrhs_zapply(sv, w);
    lsb_k_mrhs_unpack(s->n, w->kp, nb, sv->d_perm, w->z, d_Z + (size_t)c0 * ldz, ldz, g_stream);
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
