/* The direct solver: the host driver (kernels: hip_direct.hip; the factor: lsb_direct.c; its solves on blocks of
 * right-hand sides: hip_direct_m_drv.c). */
#define _GNU_SOURCE
#include "hip_solver.h"

/*
 * LSB_KRYLOV_DIRECT.  What the reference's CPU backend does -- factorise once, untimed, then time solves
 * (src/cholmod-impl.h:25-26, 59-62) -- with a factor a GPU can apply without a chain of dependent triangular levels:
 * the explicit inverse W = L^-1 of P S P^T = L L^T under a nested-dissection ordering, a skyline of sum-of-depths
 * entries.  A solve is x = P^T W^T (W (P b)): two launches, no iteration, no dot product, no host poll inside.
 *
 * Creation: direct_factor orders, counts and factorises on the host BEFORE anything is allocated on the device (the
 * refusals: over the entry budget, not positive definite), direct_upload puts the factor on the device and deals
 * the rows of k_dir_rows.  opts.precond is not consulted and opts.reorder ignored: the factor is the method, and it
 * carries its own permutation inside the kernels, so b and x stay in the caller's numbering.
 *
 * A solve: the state (k_dir_init_state), then rounds -- k_dir_rows, k_dir_cols, the residual r = b - S x off the
 * shard's plain CSR (k_dir_resid) and k_dir_step, which counts the round and decides the stop on the recomputed
 * residual.  Rounds after the first are iterative refinement.  tol = 0: exactly maxit rounds, no residual behind the
 * last one; maxit = 1 then enqueues no residual launch at all.  The device decides (the shard's lsb_pcg_state, which
 * every launch of a round is gated on); the host side is run_loop, 2 rounds per poll, never more than maxit leaves,
 * rounds replayed from captured graphs under opts.use_graph.  A solve from an initial guess is solve_x0_core's:
 * S e = b - S x0 from e = 0 by this driver.
 *
 * No vector of its own but t = W P r: r is the shard's, x the caller's, the state the shard's d_st polled through the
 * solver's pinned h_st.
 */

#define DIR_LDS_CAP 7680u /* doubles of P r a workgroup of k_dir_rows stages (60 KB); a wider window is gathered */
#define DIR_BLOCK_MIN 4096ull /* entries per workgroup of k_dir_rows at the least */

void direct_check(struct lsb_hip_opts *o, int sharded) {
  if (o->krylov != LSB_KRYLOV_DIRECT)
    return;
  if (sharded || o->nvirt > 1)
    errx(EXIT_FAILURE, "hip_cdna4: --krylov direct runs on one shard (the factor couples all rows); use it without "
                       "--ngpus / --nvirt");
  if (o->persistent != 0)
    errx(EXIT_FAILURE, "hip_cdna4: --krylov direct has no persistent form (--persistent 0)");
  if (o->precision == LSB_PREC_MIXED) {
    warnx("hip_cdna4: mixed precision is an iterative refinement around CG; --krylov direct runs in fp64");
    o->precision = LSB_PREC_FP64;
  }
  o->precond = LSB_PRECOND_NONE; /* not consulted: nothing is set up for it */
  o->reorder = 0;                /* the factor orders for itself */
}

static void direct_over_budget(unsigned n, unsigned long long entries, int at_least) {
  errx(EXIT_FAILURE, "hip_cdna4: --krylov direct: the inverse factor of this operator (%u rows) has %s%llu entries, "
                     "more than the %llu it may have (LSB_DIRECT_MAX_ENTRIES: the direct solver is for operators of a "
                     "few thousand to a few tens of thousands of rows)",
       n, at_least ? "at least " : "", entries, (unsigned long long)LSB_DIRECT_MAX_ENTRIES);
}

struct lsb_skyinv *direct_factor(const struct csr *S, const struct lsb_hip_opts *o, unsigned *height,
                                 double *seconds) {
  const double t0 = wall_seconds();
  const unsigned n = S->nrows;
  unsigned *perm = (unsigned *)malloc((size_t)(n ? n : 1) * sizeof(unsigned));
  unsigned long long lower = 0;
  const int rc = perm ? lsb_csr_nd_bounded(S, perm, LSB_DIRECT_MAX_ENTRIES, &lower) : 2;
  if (rc == 3)
    direct_over_budget(n, lower, 1);
  if (rc)
    errx(EXIT_FAILURE, "hip_cdna4: --krylov direct: out of memory computing the nested-dissection ordering");
  const unsigned long long entries = lsb_csr_skyline_count(S, perm, height);
  if (entries > LSB_DIRECT_MAX_ENTRIES)
    direct_over_budget(n, entries, 0);
  int why = 0;
  struct lsb_skyinv *W = lsb_csr_skyline_inverse(S, perm, &why);
  free(perm);
  if (why == 1)
    errx(EXIT_FAILURE, "hip_cdna4: --krylov direct needs a symmetric positive definite operator (a pivot of its "
                       "Cholesky factor is <= 0 or not finite)");
  if (why == 2)
    direct_over_budget(n, entries, 0);
  if (!W)
    errx(EXIT_FAILURE, "hip_cdna4: --krylov direct: out of memory computing the inverse factor");
  *seconds = wall_seconds() - t0;
  if (o->verbose)
    fprintf(stderr, "hip_cdna4: direct: nested dissection, %u rows, %llu entries of W = L^-1 (%.1f per row), tree "
                    "height %u, %.1f MB, set up in %.3f s on the host\n",
            n, entries, n ? (double)entries / n : 0.0, *height, 8.0e-6 * (double)entries, *seconds);
  return W;
}

/* lanes per row of k_dir_rows, from the row's length alone: about four entries per lane, 1 .. 64 */
static unsigned dir_lanes(unsigned len) {
  unsigned L = 1;
  while (L < 64 && 4 * L < len)
    L <<= 1;
  return L;
}

unsigned direct_row_lanes(unsigned len) { return dir_lanes(len); }

unsigned long long direct_block_target(unsigned long long entries) {
  return entries / 1024 < DIR_BLOCK_MIN ? DIR_BLOCK_MIN : entries / 1024;
}

/* groups: consecutive rows of one lane count, a wavefront's worth; workgroups: groups of about equal entry count */
void direct_deal_rows(const unsigned *first, const unsigned long long *woff, unsigned r0, unsigned r1,
                      unsigned long long target, unsigned cap, unsigned *grp, unsigned *ngrp_io, unsigned *blk,
                      unsigned *bwin, unsigned *nblk_io, unsigned *widest_io, unsigned *lds_m) {
  const unsigned gfirst = *ngrp_io;
  if (cap == 0 || cap > DIR_LDS_CAP)
    cap = DIR_LDS_CAP;
  unsigned ngrp = gfirst, nblk = *nblk_io, widest = *widest_io;
  for (unsigned k = r0; k < r1;) {
    const unsigned L = dir_lanes(k - first[k] + 1);
    unsigned nr = 1;
    while (k + nr < r1 && nr < 64 / L && dir_lanes(k + nr - first[k + nr] + 1) == L)
      nr++;
    grp[2 * ngrp] = k, grp[2 * ngrp + 1] = nr << 8 | L, ngrp++;
    k += nr;
  }
  for (unsigned g = gfirst; g < ngrp;) {
    unsigned long long have = 0;
    unsigned wlo = r1, g1 = g;
    while (g1 < ngrp && (g1 == g || have < target)) {
      const unsigned q0 = grp[2 * g1], q1 = q0 + (grp[2 * g1 + 1] >> 8);
      for (unsigned k = q0; k < q1; k++)
        if (first[k] < wlo)
          wlo = first[k];
      have += woff[q1] - woff[q0];
      g1++;
    }
    const unsigned khi = grp[2 * (g1 - 1)] + (grp[2 * (g1 - 1) + 1] >> 8) - 1, ww = khi - wlo + 1;
    blk[nblk] = g, bwin[2 * nblk] = wlo, bwin[2 * nblk + 1] = ww, nblk++;
    if (ww <= cap && ww > widest)
      widest = ww;
    for (unsigned q = 0; lds_m && q < 3; q++) /* ... and of the block kernels at 2, 4, 8 columns: ww kp doubles within the same cap */
      if (ww <= cap / (2u << q) && ww > lds_m[q])
        lds_m[q] = ww;
    g = g1;
  }
  *ngrp_io = ngrp, *nblk_io = nblk, *widest_io = widest;
}

void direct_upload(lsb_hip_solver *sv, struct lsb_skyinv *W, unsigned height, double seconds) {
  const unsigned n = W->n;
  struct direct_dev *d = lsb_calloc(struct direct_dev, 1);
  const unsigned long long entries = W->woff[n];
  /* what the kernels rely on, checked here once: a row's run lies inside 0 .. k, the tree climbs, runs are runs */
  for (unsigned k = 0; k < n; k++)
    if (W->first[k] > k || W->woff[k + 1] - W->woff[k] != k - W->first[k] + 1 || W->perm[k] >= n ||
        !(W->parent[k] > k && W->parent[k] <= n) || W->run_end[k] < k || W->run_end[k] >= n ||
        (k > 0 && W->first[k] < k && W->first[k] > W->first[k - 1]))
      errx(EXIT_FAILURE, "hip_cdna4: --krylov direct: the inverse factor is malformed at row %u", k);
  unsigned *grp = lsb_calloc(unsigned, 2 * (size_t)n), *blk = lsb_calloc(unsigned, (size_t)n + 1);
  unsigned *bwin = lsb_calloc(unsigned, 2 * (size_t)n), ngrp = 0, nblk = 0, widest = 0;
  direct_deal_rows(W->first, W->woff, 0, n, direct_block_target(entries), 0, grp, &ngrp, blk, bwin, &nblk, &widest,
                   d->lds_m);
  blk[nblk] = ngrp;
  d->k.n = n, d->k.nblk = nblk, d->k.ngrp = ngrp, d->k.lds_doubles = widest;
  d->k.vals = d->mem[0] = dev_upload(W->vals, (size_t)(entries ? entries : 1) * sizeof(double));
  d->k.woff = d->mem[1] = dev_upload(W->woff, ((size_t)n + 1) * sizeof(unsigned long long));
  d->k.first = d->mem[2] = dev_upload(W->first, (size_t)n * sizeof(unsigned));
  d->k.perm = d->mem[3] = dev_upload(W->perm, (size_t)n * sizeof(unsigned));
  d->k.parent = d->mem[4] = dev_upload(W->parent, (size_t)n * sizeof(unsigned));
  d->k.run_end = d->mem[5] = dev_upload(W->run_end, (size_t)n * sizeof(unsigned));
  d->k.grp = d->mem[6] = dev_upload(grp, 2 * (size_t)ngrp * sizeof(unsigned));
  d->k.blk = d->mem[7] = dev_upload(blk, ((size_t)nblk + 1) * sizeof(unsigned));
  d->k.bwin = d->mem[8] = dev_upload(bwin, 2 * (size_t)nblk * sizeof(unsigned));
  d->d_t = (double *)lsb_hip_malloc((size_t)n * sizeof(double));
  LSB_CHK_HIP(hipMemsetAsync(d->d_t, 0, (size_t)n * sizeof(double), g_stream));
  LSB_CHK_HIP(hipStreamSynchronize(g_stream)); /* host staging is freed next */
  d->entries = entries, d->height = height, d->setup_s = seconds;
  if (sv->o.verbose)
    fprintf(stderr, "hip_cdna4: direct: %u row groups in %u workgroups, windows of up to %u doubles in LDS, %.1f MB on "
                    "the device\n", ngrp, nblk, widest, 1e-6 * (8.0 * (double)entries + 36.0 * n));
  free(grp), free(blk), free(bwin);
  lsb_skyinv_free(W);
  sv->dir = d;
}

void direct_free(lsb_hip_solver *sv) {
  struct direct_dev *d = sv->dir;
  if (!d)
    return;
  graph_drop(&d->graphs);
  direct_multi_free(sv);
  direct_tier_free(sv);
  for (unsigned i = 0; i < sizeof d->mem / sizeof d->mem[0]; i++)
    lsb_hip_free(d->mem[i]);
  lsb_hip_free(d->d_t);
  free(d);
  sv->dir = NULL;
}

/* what run_loop enqueues */
struct dir_enq {
  lsb_hip_solver *sv;
  const double *d_b;
  double *d_x;
};

static void dir_enqueue_rounds(void *ctx, int rounds) {
  const struct dir_enq *e = ctx;
  struct shard *s = &e->sv->sh[0];
  struct direct_dev *d = e->sv->dir;
  const int no_resid = !(e->sv->tol_run > 0.0) && e->sv->o.maxit <= 1; /* the reference's protocol: two launches */
  for (int i = 0; i < rounds; i++) {
    if (d->tier)
      direct_tier_enqueue(e->sv, e->d_b, s->d_r, e->d_x, 0);
    else {
      lsb_k_dir_rows(&d->k, e->d_b, s->d_r, d->d_t, s->d_st, 0, g_stream);
      lsb_k_dir_cols(&d->k, d->d_t, e->d_x, s->d_st, 0, g_stream);
    }
    if (!no_resid)
      lsb_k_dir_resid(s->n, s->csr.offs, s->csr.cols, s->csr.vals, s->lanes, e->d_b, e->d_x, s->d_r, s->d_parts2,
                      &d->nrec, s->d_st, g_stream);
    lsb_k_dir_step(s->d_st, s->d_parts2, d->nrec, g_stream);
  }
}

static void dir_enqueue(void *ctx, int rounds) {
  const struct dir_enq *e = ctx;
  if (e->sv->o.use_graph)
    graph_launch(&e->sv->dir->graphs, rounds, e->d_x, dir_enqueue_rounds, ctx);
  else
    dir_enqueue_rounds(ctx, rounds);
}

int direct_solve_dev(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res) {
  struct shard *s = &sv->sh[0];
  struct direct_dev *d = sv->dir;
  struct lsb_pcg_state *hst = sv->h_st;
  const double t0 = wall_seconds();
  if (d->graph_b != d_b) /* the cached graphs hold the b they were captured with */
    graph_drop(&d->graphs), d->graph_b = d_b;
  if (sv->o.maxit == 0) /* no round stores x */
    LSB_CHK_HIP(hipMemsetAsync(d_x, 0, (size_t)s->n * sizeof(double), g_stream));
  lsb_k_dir_init_state(s->d_st, sv->tol_run, (int)sv->o.maxit, g_stream);
  struct dir_enq e = {sv, d_b, d_x};
  hst[0].iters = 0;
  const struct run_loop rl = {.name = "the direct solver", .d_state = s->d_st, .h_state = hst,
                              .state_bytes = sizeof(struct lsb_pcg_state),
                              .stop_off = offsetof(struct lsb_pcg_state, status),
                              .progress_off = offsetof(struct lsb_pcg_state, iters),
                              .enqueue = dir_enqueue, .ctx = &e,
                              .chunk = sv->o.check_every > 0 ? sv->o.check_every : 2,
                              .cap = (long)sv->o.maxit, /* rounds the device can run */
                              .what_hinted = "poll of a hinted direct solve",
                              .what_poll = "poll of the direct solve",
                              .what_drain = "drain after the direct solve"};
  run_loop(sv, &rl, hint_slot(sv->hint_iters, 0));
  struct lsb_hip_result r;
  memset(&r, 0, sizeof r);
  result_from_state(&r, &hst[0]);
  if (sv->tol_run > 0.0) {
    r.true_relres = r.relres; /* the recomputed figure is the only one there is */
    r.spmvs = r.iters;        /* one residual per round */
  } else {
    r.relres = r.true_relres = -1.0; /* nobody formed a residual to stop on */
    r.spmvs = r.iters > 0 ? r.iters - 1 : 0;
  }
  r.seconds = wall_seconds() - t0;
  if (res)
    *res = r;
  g_last = r;
  return 0;
}

int direct_apply_dev(lsb_hip_solver *sv, const double *d_r, double *d_z) {
  struct shard *s = &sv->sh[0];
  struct direct_dev *d = sv->dir;
  LSB_CHK_HIP(hipMemsetAsync(&s->d_st->status, 0, sizeof(int), g_stream)); /* the launches are gated on it */
  if (d->tier)
    direct_tier_enqueue(sv, d_r, d_r, d_z, 1);
  else {
    lsb_k_dir_rows(&d->k, d_r, d_r, d->d_t, s->d_st, 1, g_stream);
    lsb_k_dir_cols(&d->k, d->d_t, d_z, s->d_st, 1, g_stream);
  }
  drain_stream(sv, "lsb_hip_solver_precond_dev");
  return 0;
}

int lsb_hip_solver_direct_info(const lsb_hip_solver *sv, unsigned long long *entries, unsigned *height,
                               unsigned long long *bytes_per_round) {
  if (!sv || !sv->dir)
    return 2;
  const struct direct_dev *d = sv->dir;
  if (entries)
    *entries = d->entries;
  if (height)
    *height = d->height;
  if (bytes_per_round) /* the two products: W twice, first / woff per row twice, P r in, t out and in, x out */
    *bytes_per_round = d->tier ? direct_tier_round_bytes(sv) : 16ull * d->entries + (24ull + 32ull) * d->k.n;
  return 0;
}
