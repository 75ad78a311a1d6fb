/* The direct solver on blocks of right-hand sides: the host driver (kernels: hip_direct_m.hip; the single-column
 * driver and the factor: hip_direct_drv.c, lsb_direct.c). */
#define _GNU_SOURCE
#include "hip_solver.h"

/*
 * lsb_hip_solver_solve_direct_multi[_dev]: the rounds of direct_solve_dev on nrhs columns at once.  A block of kp
 * columns reads every entry of W once per product for all of them, walks the row records once and pays the same
 * launches; per column it adds kp fused multiply-adds per 8-byte load.  A column of a block has the bits of that
 * column solved alone by lsb_hip_solver_solve_dev on the same solver -- x, iters, status, relres, true_relres, spmvs --
 * which is what fixes the kernels' summation orders (hip_direct_m.hip).
 *
 * 2 .. 8 columns run as one block of kp = 2, 4 or 8 (block_width), padded with zero columns that run like any zero
 * column and are not reported; more run in blocks of 8 and a remainder; one column IS lsb_hip_solver_solve_dev.  The
 * block vectors B, X, R and T = W P V are internal and interleaved (lsb_k_mrhs_pack / _unpack as they are; the numbering
 * is the caller's, the factor's permutation is applied inside the kernels), so a round -- and a captured graph of
 * rounds -- does not depend on the caller's pointers: the graphs of a work area are keyed on the count alone.
 *
 * A round: the products (direct_tier_enqueue_m: two launches at one tier, 4 m - 2 on m tiers), k_dir_resid_m (not
 * where tol = 0 and maxit <= 1), k_dir_step_m.  Every column
 * has its own lsb_pcg_state inside the block's lsb_mrhs_state and stops on its own; a stopped column is frozen, the
 * block runs until every column has stopped (`running`, the gate of every launch).  The host side is run_loop on
 * `running`: 2 rounds per poll or opts.check_every, the previous block's count in one go, never more than maxit rounds.
 *
 * The work area of a width is made when the solver first solves a block of that width and freed with the solver: a
 * direct solver that never sees a block allocates nothing here.  Warm starts on blocks are not built.
 *
 * Every solver that is not a direct solver answers 2, as the direct solver does from solve_multi, solve_block, spmm_dev
 * and precond_multi_dev.
 *
 * A tiered factor (direct_tiered: more than one tier) is not served by these three entry points, which answer 2 on it,
 * but by lsb_hip_solver_solve_direct_tier_multi[_dev] and _direct_tier_apply_multi_dev below, which serve every direct
 * solver.  Everything here is shared: the work area holds a fifth block there (Z; Y is p).
 */
static struct dirm_work *dirm_setup(lsb_hip_solver *sv, unsigned kp) {
  struct dirm_work *w = &sv->dir->m[kp == 2 ? 0 : kp == 4 ? 1 : 2];
  if (w->blk.kp)
    return w;
  if (!sv->mr_hst) /* (mrhs_free's) */
    LSB_CHK_HIP(hipHostMalloc((void **)&sv->mr_hst, 2 * sizeof(struct lsb_mrhs_state), 0));
  /* behind the blocks: the records of the residual launch (r.r, b.b per column), then the state */
  const size_t recb = (size_t)LSB_MAX_PARTIALS * 2 * kp * sizeof(double);
  const size_t stb = (sizeof(struct lsb_mrhs_state) + 255) & ~(size_t)255;
  /* b, x, r and p = T; a tiered factor: p = Y and q = Z */
  char *behind = block_work_slab(sv, &w->blk, kp, direct_tiered(sv) ? 5 : 4, recb + stb);
  w->rec = (double *)behind;
  w->st = (struct lsb_mrhs_state *)(behind + recb);
  return w;
}

void direct_multi_free(lsb_hip_solver *sv) {
  for (int k = 0; k < 3; k++) {
    block_work_free(&sv->dir->m[k].blk);
    memset(&sv->dir->m[k], 0, sizeof sv->dir->m[k]);
  }
}

/* Bytes one round of a block of width kp(nrhs) streams (direct_round_bytes); 0 on a tiered solver */
unsigned long long lsb_hip_solver_direct_multi_round_bytes(const lsb_hip_solver *sv, unsigned nrhs) {
  if (!sv || !sv->dir || direct_tiered(sv) || nrhs == 0)
    return 0;
  return direct_round_bytes(sv, nrhs == 1 ? 1u : block_width(nrhs > LSB_MRHS_MAX ? LSB_MRHS_MAX : nrhs));
}

/* what block_enqueue runs for run_loop */
struct dirm_enq {
  lsb_hip_solver *sv;
  struct dirm_work *w;
};

static void dirm_enqueue_rounds(void *ctx, int rounds) {
  const struct dirm_enq *e = ctx;
  const struct shard *s = &e->sv->sh[0];
  struct dirm_work *w = e->w;
  const struct block_work *k = &w->blk;
  const int no_resid = !(e->sv->o.tol > 0.0) && e->sv->o.maxit <= 1; /* the reference's protocol: two launches */
  for (int i = 0; i < rounds; i++) {
    direct_tier_enqueue_m(e->sv, k, w->st);
    if (!no_resid)
      lsb_k_dir_resid_m(k->kp, s->n, s->csr.offs, s->csr.cols, s->csr.vals, s->lanes, k->b, k->x, k->r, w->rec,
                        &w->nrec, w->st, g_stream);
    lsb_k_dir_step_m(k->kp, w->st, w->rec, w->nrec, g_stream);
  }
}

/* one block: nb <= 8 columns of the caller's */
static void dirm_block(lsb_hip_solver *sv, unsigned nb, const double *d_B, size_t ldb, double *d_X, size_t ldx,
                       struct lsb_hip_result *res) {
  struct dirm_work *w = dirm_setup(sv, block_width(nb));
  const struct block_work *k = &w->blk;
  struct lsb_mrhs_state *hst = sv->mr_hst;
  const unsigned kp = k->kp, n = sv->sh[0].n;
  const double tol = sv->o.tol;
  const double t0 = wall_seconds();
  lsb_k_mrhs_pack(n, kp, nb, NULL, d_B, ldb, k->b, g_stream);
  if (sv->o.maxit == 0) /* no round stores x */
    LSB_CHK_HIP(hipMemsetAsync(k->x, 0, (size_t)n * kp * sizeof(double), g_stream));
  lsb_k_dir_init_state_m(w->st, kp, tol, (int)sv->o.maxit, g_stream);
  struct dirm_enq e = {sv, w};
  struct block_enq be = {sv, &w->blk, dirm_enqueue_rounds, &e};
  hst[0].nspmm = 0;
  const struct run_loop rl = {.name = "the direct solver on a block", .d_state = w->st, .h_state = hst,
                              .state_bytes = sizeof(struct lsb_mrhs_state),
                              .stop_off = offsetof(struct lsb_mrhs_state, running), .stop_is_running = 1,
                              .progress_off = offsetof(struct lsb_mrhs_state, nspmm),
                              .enqueue = block_enqueue, .ctx = &be,
                              .chunk = sv->o.check_every > 0 ? sv->o.check_every : 2,
                              .cap = (long)sv->o.maxit, /* rounds the device can run */
                              .what_hinted = "poll of a hinted direct block", .what_poll = "poll of the direct block",
                              .what_drain = "drain after the direct block"};
  run_loop(sv, &rl, &w->hint);
  lsb_k_mrhs_unpack(n, kp, nb, NULL, k->x, d_X, ldx, g_stream);
  drain_stream(sv, "un-packing the direct block");
  const double seconds = wall_seconds() - t0;
  for (unsigned c = 0; c < nb; c++) {
    struct lsb_hip_result r;
    memset(&r, 0, sizeof r);
    result_from_state(&r, &hst[0].c[c]);
    if (tol > 0.0) {
      r.true_relres = r.relres; /* the recomputed figure is the only one there is */
      r.spmvs = r.iters;        /* one residual per round */
    } else {
      r.relres = r.true_relres = -1.0; /* nobody formed a residual to stop on */
      r.spmvs = r.iters > 0 ? r.iters - 1 : 0;
    }
    r.seconds = seconds;
    res[c] = r;
  }
}

/* the arguments are checked and sv is a direct solver, tiered or not */
static int dirm_solve_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_B, size_t ldb, double *d_X, size_t ldx,
                          struct lsb_hip_result *res) {
  if (nrhs == 1)
    return lsb_hip_solver_solve_dev(sv, d_B, d_X, res);
  struct lsb_hip_result *tmp = res ? res : lsb_calloc(struct lsb_hip_result, nrhs);
  sv->start_n = 0; /* cold solves: lsb_hip_solver_start_relres has nothing to answer */
  for (unsigned c0 = 0; c0 < nrhs; c0 += LSB_MRHS_MAX) {
    const unsigned nb = nrhs - c0 < LSB_MRHS_MAX ? nrhs - c0 : LSB_MRHS_MAX;
    dirm_block(sv, nb, d_B + (size_t)c0 * ldb, ldb, d_X + (size_t)c0 * ldx, ldx, tmp + c0);
  }
  g_last = tmp[nrhs - 1];
  if (!res)
    free(tmp);
  return 0;
}

int lsb_hip_solver_solve_direct_multi_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_B, size_t ldb, double *d_X,
                                          size_t ldx, struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, 0, d_B, ldb, d_X, ldx) || !sv->dir || direct_tiered(sv))
    return 2;
  return dirm_solve_dev(sv, nrhs, d_B, ldb, d_X, ldx, res);
}

int lsb_hip_solver_solve_direct_multi(lsb_hip_solver *sv, unsigned nrhs, const double *B, size_t ldb, double *X,
                                      size_t ldx, struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, 0, B, ldb, X, ldx) || !sv->dir || direct_tiered(sv))
    return 2;
  return block_solve_host(lsb_hip_solver_solve_direct_multi_dev, 0, sv, nrhs, B, ldb, X, ldx, res);
}

/* Z_c = P^T W^T W P R_c once, un-gated: direct_apply_dev on a block, through the same pack / unpack */
static int dirm_apply_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_R, size_t ldr, double *d_Z, size_t ldz) {
  if (nrhs == 1)
    return lsb_hip_solver_precond_dev(sv, d_R, d_Z);
  const unsigned n = sv->sh[0].n;
  for (unsigned c0 = 0; c0 < nrhs; c0 += LSB_MRHS_MAX) {
    const unsigned nb = nrhs - c0 < LSB_MRHS_MAX ? nrhs - c0 : LSB_MRHS_MAX;
    struct dirm_work *w = dirm_setup(sv, block_width(nb));
    const struct block_work *k = &w->blk;
    lsb_k_mrhs_pack(n, k->kp, nb, NULL, d_R + (size_t)c0 * ldr, ldr, k->b, g_stream);
    direct_tier_enqueue_m(sv, k, NULL); /* once, un-gated, from B */
    lsb_k_mrhs_unpack(n, k->kp, nb, NULL, k->x, d_Z + (size_t)c0 * ldz, ldz, g_stream);
  }
  drain_stream(sv, "lsb_hip_solver_direct_apply_multi_dev");
  return 0;
}

int lsb_hip_solver_direct_apply_multi_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_R, size_t ldr, double *d_Z,
                                          size_t ldz) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, 0, d_R, ldr, d_Z, ldz) || !sv->dir || direct_tiered(sv))
    return 2;
  return dirm_apply_dev(sv, nrhs, d_R, ldr, d_Z, ldz);
}

/* ---- every direct solver, a tiered one included ----------------------------------------------------------------- */
int lsb_hip_solver_solve_direct_tier_multi_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_B, size_t ldb,
                                               double *d_X, size_t ldx, struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, 0, d_B, ldb, d_X, ldx) || !sv->dir)
    return 2;
  return dirm_solve_dev(sv, nrhs, d_B, ldb, d_X, ldx, res);
}

int lsb_hip_solver_solve_direct_tier_multi(lsb_hip_solver *sv, unsigned nrhs, const double *B, size_t ldb, double *X,
                                           size_t ldx, struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, 0, B, ldb, X, ldx) || !sv->dir)
    return 2;
  return block_solve_host(lsb_hip_solver_solve_direct_tier_multi_dev, 0, sv, nrhs, B, ldb, X, ldx, res);
}

int lsb_hip_solver_direct_tier_apply_multi_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_R, size_t ldr,
                                               double *d_Z, size_t ldz) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, 0, d_R, ldr, d_Z, ldz) || !sv->dir)
    return 2;
  return dirm_apply_dev(sv, nrhs, d_R, ldr, d_Z, ldz);
}

/* direct_round_bytes at the width of the block, one tier or more */
unsigned long long lsb_hip_solver_direct_tier_multi_round_bytes(const lsb_hip_solver *sv, unsigned nrhs) {
  if (!sv || !sv->dir || nrhs == 0)
    return 0;
  return direct_round_bytes(sv, nrhs == 1 ? 1u : block_width(nrhs > LSB_MRHS_MAX ? LSB_MRHS_MAX : nrhs));
}
