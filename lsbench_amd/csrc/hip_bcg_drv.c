/* Block-CG proper: host driver (kernels: hip_bcg.hip, and hip_bcg_m.hip for the preconditioned half below; the work
 * area, the service rules and Z = M^-1 R it shares with the driver of independent recurrences: hip_block.c). */
#define _GNU_SOURCE
#include "hip_solver.h"

/*
 * lsb_hip_solver_solve_block[_dev]: ONE Krylov space for a block of 2 .. 8 right-hand sides -- preconditioned BCGrQ
 * (the residual block kept factored as R = W sigma, W^T D^-1 W = I, by Cholesky-QR in the D^-1 inner product), x0 = 0,
 * D^-1 the solver's diagonal preconditioner (Jacobi, l1-Jacobi or none).  Where solve_multi advances nrhs independent
 * recurrences through shared launches, the columns here are coupled: the block searches the union of their Krylov
 * spaces, all columns run until all meet the stop rule (||r_c|| <= tol ||b_c|| on the recurrence, every c), and every
 * res[c] carries the block's iteration count.
 *
 * An iteration is five launches (hip_bcg.hip): the SpMM Q = S P with the records of P^T Q, k_bcg_small<GAMMA>,
 * pass A (X, W~ and the records of two Gram matrices), k_bcg_small<G> (the norms, the stop test, the next factor),
 * pass B (W, P).  The small launches have one workgroup and own the device state (lsb_blockcg_state); the device
 * decides when to stop and the host side is run_loop (hip_run.c) exactly as for a batch of independent columns:
 * check_every iterations per poll or the previous block's count in one go, a graph cache keyed on the count, internal
 * buffers only (k_mrhs_pack / k_mrhs_unpack apply the permutation of a padded or re-ordered solver).
 *
 * The block must have full rank.  The start scales G = B^T D^-1 B to unit diagonal and factors it; a pivot <= 1e-10
 * or not finite (a zero column among them) answers 3 with every status BREAKDOWN and X untouched -- the one host
 * round trip before the loop.  Inside the loop a pivot of P^T S P or of W~^T D^-1 W~ that is <= 0 or not finite stops
 * the block on the device, every column BREAKDOWN.
 *
 * opts.verify: one residual SpMM (k_spmm_csr<.., RES>, the verify round's of solve_multi) recomputes b - S x after the
 * stop and fills true_relres / relres; a column called converged that misses tol on recomputation becomes MAXIT.  The
 * in-place restart of solve_multi's verify rounds is not built for the block form.
 *
 * Served: what solve_multi serves under the diagonal preconditioners, 2 <= nrhs <= LSB_MRHS_MAX; one column is
 * lsb_hip_solver_solve_dev.  Everything else answers 2 and allocates nothing.
 */
static int blockcg_serves(const lsb_hip_solver *sv) { return block_serves(sv) && !block_zblock(sv); }

/* How a block's z = M^-1 (.) is formed: by the diagonal inside the passes (solve_block), or as a block of its own by
 * FSAI's two products or by the V-cycle (solve_block_precond, the second half of this file). */
enum blockcg_form { BK_DIAG, BK_FSAI, BK_AMG };
/* (the second half's, which the shared solve below calls) */
static void blockcg_m_setup(lsb_hip_solver *sv, struct blockcg_work *w, enum blockcg_form form);
static void blockcg_m_enqueue_iter(lsb_hip_solver *sv, struct blockcg_work *w, enum blockcg_form form);
static int blockcg_m_chunk(const lsb_hip_solver *sv, unsigned kp, enum blockcg_form form);

static struct blockcg_work *blockcg_setup(lsb_hip_solver *sv, unsigned kp) {
  struct blockcg_work *w = &sv->bk[kp == 2 ? 0 : kp == 4 ? 1 : 2];
  if (w->blk.kp)
    return w;
  if (!sv->bk_hst)
    LSB_CHK_HIP(hipHostMalloc((void **)&sv->bk_hst, 2 * sizeof(struct lsb_blockcg_state), 0));
  /* behind the five blocks, 256-byte aligned: the two record arrays, then the state */
  const unsigned tri = lsb_k_blockcg_tri(kp);
  const size_t rsp = (((size_t)LSB_MAX_PARTIALS * tri * sizeof(double)) + 255) & ~(size_t)255;
  const size_t rpa = (((size_t)LSB_STREAM_GRID_CAP * 2 * tri * sizeof(double)) + 255) & ~(size_t)255;
  const size_t stb = (sizeof(struct lsb_blockcg_state) + 255) & ~(size_t)255;
  char *behind = block_work_slab(sv, &w->blk, kp, 5, rsp + rpa + stb);
  w->rec_spmm = (double *)behind;
  w->rec_pass = (double *)(behind + rsp);
  w->st = (struct lsb_blockcg_state *)(behind + rsp + rpa);
  return w;
}

void blockcg_free(lsb_hip_solver *sv) {
  for (int k = 0; k < 3; k++) {
    block_work_free(&sv->bk[k].blk);
    memset(&sv->bk[k], 0, sizeof sv->bk[k]);
  }
  if (sv->bk_hst)
    LSB_CHK_HIP(hipHostFree(sv->bk_hst));
  sv->bk_hst = NULL;
}

/* Bytes one iteration of a block of nrhs columns must move: 12 nnz + 4 (n + 1) + 8 n (12 kp + 2 [the diagonal is a
 * vector]) -- the CSR arrays once whatever the width, and 12 vector passes per column: the SpMM 2 (P gathered, Q
 * out), pass A 6 (W, Q, P, X in; W~, X out), pass B 4 (W~, P in; W, P out); the inverse diagonal once in each of
 * the two passes.  0 where the block form is not served. */
unsigned long long lsb_hip_solver_block_iteration_bytes(const lsb_hip_solver *sv, unsigned nrhs) {
  if (!sv || nrhs == 0 || nrhs > LSB_MRHS_MAX || !blockcg_serves(sv))
    return 0;
  const struct shard *s = &sv->sh[0];
  const unsigned kp = nrhs == 1 ? 1u : block_width(nrhs);
  return 12ull * s->nnz + 4ull * (s->n + 1ull) + 8ull * s->n * (12ull * kp + (s->dinv_uniform ? 0u : 2u));
}

static void blockcg_enqueue_iter(lsb_hip_solver *sv, struct blockcg_work *w) {
  const struct shard *s = &sv->sh[0];
  const struct block_work *k = &w->blk;
  unsigned nsp = 0, npa = 0;
  lsb_k_blockcg_spmm(k->kp, s->n, s->csr.offs, s->csr.cols, s->csr.vals, sv->mr_lanes, k->p, k->q, w->rec_spmm, &nsp,
                     w->st, g_stream);
  lsb_k_blockcg_small(k->kp, LSB_BLOCKCG_GAMMA, w->st, w->rec_spmm, nsp, 0, 0.0, 0, g_stream);
  lsb_k_blockcg_pass_a(k->kp, s->n, k->w, k->q, k->p, k->x, DINV(s), w->st, w->rec_pass, &npa, g_stream);
  lsb_k_blockcg_small(k->kp, LSB_BLOCKCG_G, w->st, w->rec_pass, npa, 0, 0.0, 0, g_stream);
  lsb_k_blockcg_pass_b(k->kp, s->n, k->w, k->p, DINV(s), w->st, g_stream);
}

/* what block_enqueue runs for run_loop (a solver has one form: its preconditioner's) */
struct blockcg_enq {
  lsb_hip_solver *sv;
  struct blockcg_work *w;
  enum blockcg_form form;
};
static void blockcg_enqueue_iters(void *ctx, int iters) {
  const struct blockcg_enq *e = ctx;
  for (int i = 0; i < iters; i++) {
    if (e->form == BK_DIAG)
      blockcg_enqueue_iter(e->sv, e->w);
    else
      blockcg_m_enqueue_iter(e->sv, e->w, e->form);
  }
}

static int blockcg_chunk(const lsb_hip_solver *sv, unsigned kp) {
  if (sv->o.check_every > 0)
    return sv->o.check_every;
  return run_chunk((double)lsb_hip_solver_block_iteration_bytes(sv, kp), 10.0, 8, 256);
}

/* one block of 2 .. 8 columns in the given form; the caller has checked the arguments and the service rule */
static int blockcg_solve(lsb_hip_solver *sv, unsigned nrhs, const double *d_B, size_t ldb, double *d_X, size_t ldx,
                         struct lsb_hip_result *res, enum blockcg_form form) {
  struct blockcg_work *w = blockcg_setup(sv, block_width(nrhs));
  if (form != BK_DIAG)
    blockcg_m_setup(sv, w, form);
  const struct shard *s = &sv->sh[0];
  const struct block_work *k = &w->blk;
  struct lsb_blockcg_state *hst = sv->bk_hst;
  const unsigned kp = k->kp, n = s->n;
  unsigned nrec = 0, nverify = 0;
  int rc = 0;
  const double t0 = wall_seconds();
  lsb_k_mrhs_pack(n, kp, nrhs, sv->d_perm, d_B, ldb, k->b, g_stream);
  if (form == BK_DIAG)
    lsb_k_blockcg_init(kp, n, k->b, DINV(s), w->rec_pass, &nrec, g_stream);
  else { /* Z = M^-1 B (un-gated, no Gram sums), then the records of (B^T Z, b_c . b_c) */
    block_zapply(sv, k, k->b, w->rec_spmm);
    lsb_k_blockcg_m_gram(kp, 1, n, k->b, k->z, w->rec_pass, &nrec, w->st, g_stream);
  }
  lsb_k_blockcg_small(kp, LSB_BLOCKCG_START, w->st, w->rec_pass, nrec, nrhs, sv->o.tol, (int)sv->o.maxit, g_stream);
  /* the rank rule is looked at here, from one copy of the state, before anything of the caller's is written */
  LSB_CHK_HIP(hipMemcpyAsync(&hst[0], w->st, sizeof hst[0], hipMemcpyDeviceToHost, g_stream));
  drain_stream(sv, "the start of the block");
  if (hst[0].rank_bad)
    rc = 3;
  else {
    if (form == BK_DIAG)
      lsb_k_blockcg_start(kp, n, k->b, DINV(s), k->w, k->p, k->x, w->st, g_stream);
    else
      lsb_k_blockcg_m_start(kp, n, k->b, k->z, k->w, k->p, k->x, w->st, g_stream);
    struct blockcg_enq e = {sv, w, form};
    struct block_enq be = {sv, &w->blk, blockcg_enqueue_iters, &e};
    const struct run_loop r = {.name = "a block of right-hand sides", .d_state = w->st, .h_state = hst,
                               .state_bytes = sizeof(struct lsb_blockcg_state),
                               .stop_off = offsetof(struct lsb_blockcg_state, running), .stop_is_running = 1,
                               .progress_off = offsetof(struct lsb_blockcg_state, nspmm),
                               .enqueue = block_enqueue, .ctx = &be,
                               .chunk = form == BK_DIAG ? blockcg_chunk(sv, kp) : blockcg_m_chunk(sv, kp, form),
                               .even = 0, .max_piece = sv->o.use_graph ? 512 : 0, .cap = -1,
                               .what_hinted = "poll of a hinted block", .what_poll = "poll of the block",
                               .what_drain = "drain after the block"};
    run_loop(sv, &r, &w->hint);
    if (sv->o.verify && sv->o.tol > 0.0) {
      lsb_k_spmm_csr(kp, n, s->csr.offs, s->csr.cols, s->csr.vals, sv->mr_lanes, k->x, k->q, k->b, w->rec_spmm, &nrec,
                     NULL, g_stream);
      lsb_k_blockcg_small(kp, LSB_BLOCKCG_VERIFY, w->st, w->rec_spmm, nrec, 0, 0.0, 0, g_stream);
      nverify = 1;
      LSB_CHK_HIP(hipMemcpyAsync(&hst[0], w->st, sizeof hst[0], hipMemcpyDeviceToHost, g_stream));
    }
    lsb_k_mrhs_unpack(n, kp, nrhs, sv->d_perm, k->x, d_X, ldx, g_stream);
    drain_stream(sv, "un-packing the block");
  }
  const double seconds = wall_seconds() - t0;
  for (unsigned c = 0; c < nrhs; c++) {
    struct lsb_hip_result r;
    memset(&r, 0, sizeof r);
    r.iters = (unsigned)hst[0].iters;
    r.status = hst[0].status[c];
    r.relres = hst[0].bb[c] > 0.0 ? sqrt(hst[0].rr[c] / hst[0].bb[c]) : 0.0;
    r.true_relres = hst[0].true_relres[c];
    if (r.true_relres >= 0.0)
      r.relres = r.true_relres;
    r.seconds = seconds;
    r.spmvs = (unsigned)hst[0].nspmm + nverify;
    if (res)
      res[c] = r;
    g_last = r;
  }
  return rc;
}

int lsb_hip_solver_solve_block_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_B, size_t ldb, double *d_X,
                                   size_t ldx, struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, LSB_MRHS_MAX, d_B, ldb, d_X, ldx) || !blockcg_serves(sv))
    return 2;
  if (nrhs == 1)
    return lsb_hip_solver_solve_dev(sv, d_B, d_X, res);
  return blockcg_solve(sv, nrhs, d_B, ldb, d_X, ldx, res, BK_DIAG);
}

/* (the host-buffer forms: X is the caller's again only where the block was solved -- a block without full rank
 * answers 3 with X untouched) */
int lsb_hip_solver_solve_block(lsb_hip_solver *sv, unsigned nrhs, const double *B, size_t ldb, double *X, size_t ldx,
                               struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, LSB_MRHS_MAX, B, ldb, X, ldx) || !blockcg_serves(sv))
    return 2;
  return block_solve_host(lsb_hip_solver_solve_block_dev, 0, sv, nrhs, B, ldb, X, ldx, res);
}

/* ||r_c||^2 of the recurrence and ||b_c||^2 as the device state of the last block held them (nrhs <= 8 entries each,
 * either may be NULL): what res[c].relres was formed from.  2 where no block has been solved. */
int lsb_hip_solver_block_norms(const lsb_hip_solver *sv, unsigned nrhs, double *rr, double *bb) {
  if (!sv || !sv->bk_hst || nrhs == 0 || nrhs > LSB_MRHS_MAX)
    return 2;
  for (unsigned c = 0; c < nrhs; c++) {
    if (rr)
      rr[c] = sv->bk_hst[0].rr[c];
    if (bb)
      bb[c] = sv->bk_hst[0].bb[c];
  }
  return 0;
}

/*
 * ---- Block-CG under FSAI and AMG -------------------------------------------------------------------------------
 * lsb_hip_solver_solve_block_precond[_dev]: the method above with D^-1 replaced by the solver's M^-1 where that is a
 * symmetric operator -- FSAI's G^T G, or the V-cycle smoothed by l1-Jacobi or Chebyshev -- so the preconditioned block
 * is a stored operand Z (kernels: hip_bcg_m.hip; the SpMM, k_bcg_small, the state, run_loop, the graph cache, the
 * hint, pack / unpack, the rank rule, opts.verify and lsb_hip_solver_block_norms are the first half's, unchanged):
 *
 *   start: Z = M^-1 B (un-gated: two SpMMs off G and G^T, or one cycle) ; k_bcgm_gram<START> ; k_bcg_small<START> ;
 *          the one host round trip of the rank rule ; k_bcgm_start
 *   FSAI, 7 launches:  k_bcg_spmm, small<GAMMA>, k_bcgm_pass_a, T = G W~ (k_spmm_csr), k_bcgm_gt_gram (Z~ = G^T T with
 *                      the Gram sums riding in it), small<G>, k_bcgm_pass_b
 *   AMG, 6 + a cycle:  k_bcg_spmm, small<GAMMA>, k_bcgm_pass_a, amg_cycle(r = W~, z = Z~), k_bcgm_gram, small<G>,
 *                      k_bcgm_pass_b
 *
 * The gate.  The cycle's launches and lsb_k_spmm_csr gate on a lsb_mrhs_state, which a block does not have, so inside
 * the loop they run UN-GATED (st = NULL): once the block has stopped they churn the stale W~ for the rest of the chunk
 * into T and Z~, which nobody reads -- pass A, the Gram launches, k_bcg_small and pass B are gated on st->running and
 * X is not touched again.  The waste is bounded by the chunk: under AMG blockcg_m_chunk takes the floor of 2 that
 * solve_multi's chunk takes there, so at most one cycle is wasted on an un-hinted first solve; a hinted solve enqueues
 * the previous count.
 *
 * Served: what solve_multi serves with a z block (blockcg_m_serves): AMG in fp64 smoothed by l1-Jacobi or Chebyshev,
 * FSAI with opts.fsai_blocks; 2 <= nrhs <= LSB_MRHS_MAX, one shard, x0 = 0.  A solver under a diagonal preconditioner
 * is forwarded to solve_block_dev (the same bits); one column is lsb_hip_solver_solve_dev.  Everything else answers 2
 * and allocates nothing.
 */
static enum blockcg_form blockcg_m_form(const lsb_hip_solver *sv) {
  return sv->o.precond == LSB_PRECOND_FSAI ? BK_FSAI : BK_AMG;
}

static int blockcg_m_serves(const lsb_hip_solver *sv) { return block_serves(sv) && block_zblock(sv); }

/* on the first preconditioned block the work area grows by z -- plus t = G w and the records of k_bcgm_gt_gram's grid
 * under FSAI; under AMG z is the head of the cycle's block vectors and the Gram launch is a streaming pass (rec_pass) */
static void blockcg_m_setup(lsb_hip_solver *sv, struct blockcg_work *w, enum blockcg_form form) {
  if (w->blk.z)
    return;
  const size_t rec = (size_t)LSB_MAX_PARTIALS * 2 * lsb_k_blockcg_tri(w->blk.kp) * sizeof(double);
  w->rec_gram = (double *)block_work_z(sv, &w->blk, form == BK_FSAI ? rec : 0);
}

/* Z = M^-1 R on a block is block_zapply and T = G R block_fsai_g (hip_block.c), both un-gated.  The records of the
 * SpMMs off G and G^T, which nobody reads, go into rec_spmm: the next k_bcg_spmm or the verify round writes it anew. */
static void blockcg_m_enqueue_iter(lsb_hip_solver *sv, struct blockcg_work *w, enum blockcg_form form) {
  const struct shard *s = &sv->sh[0];
  const struct block_work *k = &w->blk;
  unsigned nsp = 0, ngr = 0;
  double *rec = form == BK_FSAI ? w->rec_gram : w->rec_pass;
  lsb_k_blockcg_spmm(k->kp, s->n, s->csr.offs, s->csr.cols, s->csr.vals, sv->mr_lanes, k->p, k->q, w->rec_spmm, &nsp,
                     w->st, g_stream);
  lsb_k_blockcg_small(k->kp, LSB_BLOCKCG_GAMMA, w->st, w->rec_spmm, nsp, 0, 0.0, 0, g_stream);
  lsb_k_blockcg_m_pass_a(k->kp, s->n, k->w, k->q, k->p, k->x, w->st, g_stream);
  if (form == BK_FSAI) {
    block_fsai_g(sv, k, k->w, w->rec_spmm);
    lsb_k_blockcg_m_gt_gram(k->kp, s->n, s->fs_gt.offs, s->fs_gt.cols, s->fs_gt.vals,
                            block_fsai_lanes(sv, &s->fs_gt), k->t, k->w, k->z, rec, &ngr, w->st, g_stream);
  } else {
    block_zapply(sv, k, k->w, NULL); /* the cycle */
    lsb_k_blockcg_m_gram(k->kp, 0, s->n, k->w, k->z, rec, &ngr, w->st, g_stream);
  }
  lsb_k_blockcg_small(k->kp, LSB_BLOCKCG_G, w->st, rec, ngr, 0, 0.0, 0, g_stream);
  lsb_k_blockcg_m_pass_b(k->kp, s->n, k->w, k->z, k->p, w->st, g_stream);
}

/* Bytes one iteration of a block of nrhs columns must move under FSAI: S, G and G^T once each whatever the width
 * (12 B per non-zero and the three row-offset arrays), and 18 vector passes per column -- the SpMM 2 (P gathered, Q
 * out), pass A 6 (W, Q, P, X in; W~, X out), the product with G 2 (W~ gathered, T out), k_bcgm_gt_gram 3 (T gathered,
 * W~ in, Z~ out), pass B 5 (W~, Z~, P in; W, P out).  Under AMG 0, as lsb_hip_solver_multi_iteration_bytes (a V-cycle
 * has another shape); a diagonal preconditioner: lsb_hip_solver_block_iteration_bytes; 0 where nothing is served. */
unsigned long long lsb_hip_solver_block_precond_iteration_bytes(const lsb_hip_solver *sv, unsigned nrhs) {
  if (!sv || nrhs == 0 || nrhs > LSB_MRHS_MAX)
    return 0;
  if (blockcg_serves(sv))
    return lsb_hip_solver_block_iteration_bytes(sv, nrhs);
  if (!blockcg_m_serves(sv) || blockcg_m_form(sv) != BK_FSAI)
    return 0;
  const struct shard *s = &sv->sh[0];
  const unsigned kp = nrhs == 1 ? 1u : block_width(nrhs);
  return 12ull * (s->nnz + s->fs_g.nnz + s->fs_gt.nnz) + 12ull * (s->n + 1ull) + 8ull * s->n * 18ull * kp;
}

/* iterations per host poll: blockcg_chunk's rule on this form's bytes; under AMG on solve_multi's estimate of the SpMM,
 * the passes and the cycle, with its floor of 2 (see "The gate" above) */
static int blockcg_m_chunk(const lsb_hip_solver *sv, unsigned kp, enum blockcg_form form) {
  if (sv->o.check_every > 0)
    return sv->o.check_every;
  if (form == BK_FSAI)
    return run_chunk((double)lsb_hip_solver_block_precond_iteration_bytes(sv, kp), 10.0, 8, 256);
  const struct shard *s = &sv->sh[0];
  return run_chunk((double)(12ull * s->nnz + s->amg->cycle_mat_bytes + 8ull * kp * (16ull * s->n + s->amg->cycle_vec_rows)),
                   10.0, 2, 256);
}

int lsb_hip_solver_solve_block_precond_dev(lsb_hip_solver *sv, unsigned nrhs, const double *d_B, size_t ldb,
                                           double *d_X, size_t ldx, struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, LSB_MRHS_MAX, d_B, ldb, d_X, ldx))
    return 2;
  if (blockcg_serves(sv))
    return lsb_hip_solver_solve_block_dev(sv, nrhs, d_B, ldb, d_X, ldx, res);
  if (!blockcg_m_serves(sv))
    return 2;
  if (nrhs == 1)
    return lsb_hip_solver_solve_dev(sv, d_B, d_X, res);
  return blockcg_solve(sv, nrhs, d_B, ldb, d_X, ldx, res, blockcg_m_form(sv));
}

int lsb_hip_solver_solve_block_precond(lsb_hip_solver *sv, unsigned nrhs, const double *B, size_t ldb, double *X,
                                       size_t ldx, struct lsb_hip_result *res) {
  if (!lsb_initialized)
    return 1;
  if (block_args_bad(sv, nrhs, LSB_MRHS_MAX, B, ldb, X, ldx) || !(blockcg_serves(sv) || blockcg_m_serves(sv)))
    return 2;
  return block_solve_host(lsb_hip_solver_solve_block_precond_dev, 0, sv, nrhs, B, ldb, X, ldx, res);
}
