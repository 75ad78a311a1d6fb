/* The direct solver: the host driver -- creation, upload, the single-column solve and apply, the info calls and the
 * enqueues of the products (kernels: hip_direct.hip, hip_direct_t.hip, hip_direct_tm.hip; the factor: lsb_direct.c,
 * struct lsb_tierinv; its solves on blocks of right-hand sides: hip_direct_m_drv.c). */
#define _GNU_SOURCE
#include "hip_solver.h"

/*
 * LSB_KRYLOV_DIRECT.  What the reference's CPU backend does -- factorise once, untimed, then time solves
 * (src/cholmod-impl.h:25-26, 59-62) -- with a factor a GPU can apply without a chain of dependent triangular levels:
 * the explicit inverse W = L^-1 of P S P^T = L L^T under a nested-dissection ordering, a skyline of sum-of-depths
 * entries.  A solve is x = P^T W^T (W (P b)): two launches, no iteration, no dot product, no host poll inside.
 *
 * The single skyline has n + sum |below| |separator| entries, which is why operators of more than a few tens of
 * thousands of rows are refused.  Nearly all of them are the dense rows of the high separators over everything below.
 * lsb_hip_solver_create_direct(A, opts, tiers) cuts the tree into tiers by subtree size: only the diagonal blocks
 * W_tt = (L_tt)^-1 are kept as skylines, and the blocks below the diagonal stay what they are in L: sparse.  An
 * application is then a block forward and a block backward substitution over the tiers, 4 m - 2 launches for m tiers,
 * ordered by the launches alone.  There is ONE device layout (struct lsb_dirt_dev) and one set of product kernels:
 * the single skyline is the factor with ntier == 1 (lsb_hip_solver_create, tiers = 1, and tiers = 0 where one tier
 * fits) -- no coupling, no z, two launches.  "Tiered" is ntier > 1 (direct_tiered).
 *
 * Creation: direct_factor orders, counts (tiers = 0 takes the fewest that fit) and factorises on the host BEFORE
 * anything is allocated on the device (the refusals: over the entry budget, not positive definite),
 * direct_tier_upload puts the factor on the device and deals the rows of k_dirt_rows.  opts.precond is not consulted
 * and opts.reorder ignored: the factor is the method, and it carries its own permutation inside the kernels, so b and
 * x stay in the caller's numbering.
 *
 * A solve: the state (k_dir_init_state), then rounds -- the products (direct_tier_enqueue), the residual r = b - S x
 * off the shard's plain CSR (k_dir_resid) and k_dir_step, which counts the round and decides the stop on the
 * recomputed residual.  Rounds after the first are iterative refinement.  tol = 0: exactly maxit rounds, no residual
 * behind the last one; maxit = 1 then enqueues no residual launch at all.  The device decides (the shard's
 * lsb_pcg_state, which every launch of a round is gated on); the host side is run_loop, 2 rounds per poll, never more
 * than maxit leaves, rounds replayed from captured graphs under opts.use_graph.  A solve from an initial guess is
 * solve_x0_core's: S e = b - S x0 from e = 0 by this driver.
 *
 * Vectors of its own: y (direct_dev.d_t; at one tier t = W P r) and, tiered, z, in the factor's numbering.  r is the
 * shard's, x the caller's, the state the shard's d_st polled through the solver's pinned h_st.
 */

#define DIR_LDS_CAP 7680u /* doubles of its operand a workgroup of k_dirt_rows stages (60 KB); a wider window is gathered */
#define DIR_BLOCK_MIN 4096ull /* entries per workgroup of k_dirt_rows at the least */

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

/* tiers = 1: the single skyline, refused early (the lower bound of the ordering) or by the count of the finished
 * ordering.  tiers = 0: the fewest tiers that fit, by the symbolic count alone -- one, where the single skyline fits:
 * the same factor as tiers = 1 */
struct lsb_tierinv *direct_factor(const struct csr *S, const struct lsb_hip_opts *o, int tiers, unsigned *height,
                                  double *seconds) {
  const double t0 = wall_seconds();
  const unsigned n = S->nrows;
  unsigned *perm = (unsigned *)malloc((size_t)(n ? n : 1) * sizeof(unsigned));
  unsigned long long w = 0, c = 0;
  unsigned m = tiers ? (unsigned)tiers : 1;
  if (tiers == 1) {
    unsigned long long lower = 0;
    const int rc = perm ? lsb_csr_nd_bounded(S, perm, LSB_DIRECT_MAX_ENTRIES, &lower) : 2;
    if (rc == 3)
      direct_over_budget(n, lower, 1);
    if (rc)
      errx(EXIT_FAILURE, "hip_cdna4: --krylov direct: out of memory computing the nested-dissection ordering");
    w = lsb_csr_skyline_count(S, perm, height);
    if (w > LSB_DIRECT_MAX_ENTRIES)
      direct_over_budget(n, w, 0);
  } else {
    if (!perm || lsb_csr_nd(S, perm))
      errx(EXIT_FAILURE, "hip_cdna4: --krylov direct: out of memory computing the nested-dissection ordering");
    for (;; m++) {
      if (lsb_csr_tiered_count(S, perm, m, &w, &c, height))
        errx(EXIT_FAILURE, "hip_cdna4: --krylov direct: out of memory counting the tiered inverse factor");
      if (w + 3 * c <= LSB_DIRECT_MAX_ENTRIES || tiers || m == LSB_DIRECT_MAX_TIERS)
        break;
    }
    if (w + 3 * c > LSB_DIRECT_MAX_ENTRIES)
      errx(EXIT_FAILURE, "hip_cdna4: --krylov direct: in %u tiers the inverse factor of this operator (%u rows) has "
                         "%llu entries and its coupling %llu, which count three times: more than the %llu entries it "
                         "may have (LSB_DIRECT_MAX_ENTRIES)%s",
           m, n, w, c, (unsigned long long)LSB_DIRECT_MAX_ENTRIES,
           tiers ? "" : "; that is the largest number of tiers there is (LSB_DIRECT_MAX_TIERS)");
  }
  int why = 0;
  struct lsb_tierinv *T = lsb_csr_tiered_inverse(S, perm, m, &why);
  free(perm);
  if (why == 1)
    errx(EXIT_FAILURE, "hip_cdna4: --krylov direct needs a symmetric positive definite operator (a pivot of its "
                       "Cholesky factor is <= 0 or not finite)");
  if (why == 2 && m == 1)
    direct_over_budget(n, w, 0);
  if (!T)
    errx(EXIT_FAILURE, "hip_cdna4: --krylov direct: out of memory computing the inverse factor");
  *seconds = wall_seconds() - t0;
  if (o->verbose && T->ntier == 1)
    fprintf(stderr, "hip_cdna4: direct: nested dissection, %u rows, %llu entries of W = L^-1 (%.1f per row), tree "
                    "height %u, %.1f MB, set up in %.3f s on the host\n",
            n, w, n ? (double)w / n : 0.0, *height, 8.0e-6 * (double)w, *seconds);
  else if (o->verbose)
    fprintf(stderr, "hip_cdna4: direct: nested dissection, %u rows in %u tiers (%u asked for), %llu entries of the "
                    "W_tt and %llu of the coupling, tree height %u, %.1f MB, set up in %.3f s on the host\n",
            n, T->ntier, m, w, c, *height, 1e-6 * (8.0 * (double)w + 24.0 * (double)c), *seconds);
  return T;
}

/* lanes per row of k_dirt_rows and of the coupling kernels, from the row's length alone: about four entries per lane, 1 .. 64 */
static unsigned dir_lanes(unsigned len) {
  unsigned L = 1;
  while (L < 64 && 4 * L < len)
    L <<= 1;
  return L;
}

static unsigned long long direct_block_target(unsigned long long entries) {
  return entries / 1024 < DIR_BLOCK_MIN ? DIR_BLOCK_MIN : entries / 1024;
}

/* The dealing of the skyline rows r0 .. r1 - 1 to k_dirt_rows, appended to grp (at *ngrp_io), blk and bwin (at
 * *nblk_io).  Groups: consecutive rows of one lane count, a wavefront's worth; workgroups: groups of about `target`
 * entries.  *widest_io: the widest window within `cap` doubles (0 or more than DIR_LDS_CAP: DIR_LDS_CAP); lds_m: the
 * widest of at most cap / kp rows per width kp = 2, 4, 8 of the block kernels.  The caller closes blk[*nblk_io] */
static void direct_deal_rows(const unsigned *first, const unsigned long long *woff, unsigned r0, unsigned r1,
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
    for (unsigned q = 0; q < 3; q++) /* ... and of the block kernels at 2, 4, 8 columns: ww kp doubles within the same cap */
      if (ww <= cap / (2u << q) && ww > lds_m[q])
        lds_m[q] = ww;
    g = g1;
  }
  *ngrp_io = ngrp, *nblk_io = nblk, *widest_io = widest;
}

/* the rows r0 .. r1 - 1 of a CSR (offs[row - base]) in groups of consecutive rows with one lane count, appended to
 * grp at *ngrp */
static void tier_deal_csr(const unsigned *offs, unsigned base, unsigned r0, unsigned r1, unsigned *grp,
                          unsigned *ngrp) {
  for (unsigned k = r0; k < r1;) {
    const unsigned L = dir_lanes(offs[k - base + 1] - offs[k - base]);
    unsigned nr = 1;
    while (k + nr < r1 && nr < 64 / L && dir_lanes(offs[k + nr - base + 1] - offs[k + nr - base]) == L)
      nr++;
    grp[2 * *ngrp] = k, grp[2 * *ngrp + 1] = nr << 8 | L, (*ngrp)++;
    k += nr;
  }
}

/* One tier: no coupling, no groups of coupling rows and no z on the device -- the pointers stay NULL, nothing reads
 * them */
void direct_tier_upload(lsb_hip_solver *sv, struct lsb_tierinv *T, unsigned height, double seconds) {
  const unsigned n = T->n, m = T->ntier, lo1 = T->lo[m > 1 ? 1 : m];
  struct direct_dev *d = lsb_calloc(struct direct_dev, 1);
  const unsigned long long entries = T->woff[n];
  const unsigned coupling = T->coffs[n - lo1];
  /* what the kernels rely on, checked here once.  The skylines: a row's run lies inside its tier, below k; the trees
   * climb and stay in their tier; runs are runs.  The coupling: offsets ascend, a row of C reads below its tier, a row
   * of tier t's C^T reads inside tier t */
  int bad = m < 1 || m > LSB_DIRECT_MAX_TIERS || T->lo[0] != 0 || T->lo[m] != n;
  for (unsigned t = 0; t < m && !bad; t++) {
    bad = T->lo[t] > T->lo[t + 1];
    for (unsigned k = T->lo[t]; k < T->lo[t + 1] && !bad; k++)
      bad = T->first[k] > k || T->first[k] < T->lo[t] || T->woff[k + 1] - T->woff[k] != k - T->first[k] + 1 ||
            T->perm[k] >= n || !(T->parent[k] > k && (T->parent[k] < T->lo[t + 1] || T->parent[k] == n)) ||
            T->run_end[k] < k || T->run_end[k] >= T->lo[t + 1] ||
            (k > T->lo[t] && T->first[k] < k && T->first[k] > T->first[k - 1]);
  }
  size_t nt = 0; /* offsets of C^T before tier t */
  unsigned tbase[LSB_DIRECT_MAX_TIERS] = {0};
  for (unsigned t = 1; t < m && !bad; t++) {
    tbase[t] = (unsigned)nt;
    for (unsigned i = T->lo[t]; i < T->lo[t + 1] && !bad; i++) {
      const unsigned e0 = T->coffs[i - lo1], e1 = T->coffs[i - lo1 + 1];
      bad = e0 > e1 || e1 > coupling;
      for (unsigned e = e0; e < e1 && !bad; e++)
        bad = T->ccols[e] >= T->lo[t];
    }
    for (unsigned j = 0; j < T->lo[t] && !bad; j++) {
      const unsigned e0 = T->toffs[nt + j], e1 = T->toffs[nt + j + 1];
      bad = e0 > e1 || e1 > coupling;
      for (unsigned e = e0; e < e1 && !bad; e++)
        bad = T->tcols[e] < T->lo[t] || T->tcols[e] >= T->lo[t + 1];
    }
    nt += (size_t)T->lo[t] + 1;
  }
  if (bad || (m > 1 && T->coffs[0] != 0))
    errx(EXIT_FAILURE, "hip_cdna4: --krylov direct: the inverse factor is malformed");
  /* the dealing, tier by tier: no group, workgroup or window straddles a tier */
  unsigned *grp = lsb_calloc(unsigned, 2 * (size_t)n), *blk = lsb_calloc(unsigned, (size_t)n + 1);
  unsigned *bwin = lsb_calloc(unsigned, 2 * (size_t)n), ngrp = 0, nblk = 0;
  unsigned *cgrp = m > 1 ? lsb_calloc(unsigned, 2 * (size_t)n) : NULL, ncg = 0;
  unsigned *tgrp = m > 1 ? lsb_calloc(unsigned, 2 * nt) : NULL, ntg = 0;
  unsigned widest_all = 0;
  /* LSBENCH_HIP_DIRECT_TIER_LDS: fewer doubles of a window staged than the launch could (for the tests, which reach
   * the gathered windows on small operators with it) */
  const char *env = getenv("LSBENCH_HIP_DIRECT_TIER_LDS");
  const unsigned cap = env && atoi(env) > 0 ? (unsigned)atoi(env) : 0;
  for (unsigned t = 0; t < m; t++) {
    struct lsb_dirt_tier *k = &d->k.t[t];
    k->lo = T->lo[t], k->hi = T->lo[t + 1], k->blk0 = nblk, k->tbase = tbase[t];
    direct_deal_rows(T->first, T->woff, k->lo, k->hi, direct_block_target(entries), cap, grp, &ngrp, blk, bwin, &nblk,
                     &k->lds_doubles, k->lds_m);
    k->nblk = nblk - k->blk0;
    if (k->lds_doubles > widest_all)
      widest_all = k->lds_doubles;
    k->cg0 = k->cg1 = ncg, k->tg0 = k->tg1 = ntg;
    if (t >= 1) {
      tier_deal_csr(T->coffs, lo1, k->lo, k->hi, cgrp, &ncg);
      tier_deal_csr(T->toffs + tbase[t], 0, 0, k->lo, tgrp, &ntg);
      k->cg1 = ncg, k->tg1 = ntg;
    }
  }
  blk[nblk] = ngrp;
  d->k.n = n, d->k.ntier = m;
  unsigned u = 0;
  d->k.vals = d->mem[u++] = dev_upload(T->vals, (size_t)(entries ? entries : 1) * sizeof(double));
  d->k.woff = d->mem[u++] = dev_upload(T->woff, ((size_t)n + 1) * sizeof(unsigned long long));
  d->k.first = d->mem[u++] = dev_upload(T->first, (size_t)n * sizeof(unsigned));
  d->k.perm = d->mem[u++] = dev_upload(T->perm, (size_t)n * sizeof(unsigned));
  d->k.parent = d->mem[u++] = dev_upload(T->parent, (size_t)n * sizeof(unsigned));
  d->k.run_end = d->mem[u++] = dev_upload(T->run_end, (size_t)n * sizeof(unsigned));
  d->k.grp = d->mem[u++] = dev_upload(grp, 2 * (size_t)ngrp * sizeof(unsigned));
  d->k.blk = d->mem[u++] = dev_upload(blk, ((size_t)nblk + 1) * sizeof(unsigned));
  d->k.bwin = d->mem[u++] = dev_upload(bwin, 2 * (size_t)nblk * sizeof(unsigned));
  d->d_t = (double *)lsb_hip_malloc((size_t)n * sizeof(double));
  LSB_CHK_HIP(hipMemsetAsync(d->d_t, 0, (size_t)n * sizeof(double), g_stream));
  if (m > 1) {
    d->k.coffs = d->mem[u++] = dev_upload(T->coffs, ((size_t)(n - lo1) + 1) * sizeof(unsigned));
    d->k.ccols = d->mem[u++] = dev_upload(T->ccols, (size_t)(coupling ? coupling : 1) * sizeof(unsigned));
    d->k.cvals = d->mem[u++] = dev_upload(T->cvals, (size_t)(coupling ? coupling : 1) * sizeof(double));
    d->k.toffs = d->mem[u++] = dev_upload(T->toffs, nt * sizeof(unsigned));
    d->k.tcols = d->mem[u++] = dev_upload(T->tcols, (size_t)(coupling ? coupling : 1) * sizeof(unsigned));
    d->k.tvals = d->mem[u++] = dev_upload(T->tvals, (size_t)(coupling ? coupling : 1) * sizeof(double));
    d->k.cgrp = d->mem[u++] = dev_upload(cgrp, 2 * (size_t)(ncg ? ncg : 1) * sizeof(unsigned));
    d->k.tgrp = d->mem[u++] = dev_upload(tgrp, 2 * (size_t)(ntg ? ntg : 1) * sizeof(unsigned));
    d->d_z = (double *)lsb_hip_malloc((size_t)n * sizeof(double));
    LSB_CHK_HIP(hipMemsetAsync(d->d_z, 0, (size_t)n * sizeof(double), g_stream));
  }
  LSB_CHK_HIP(hipStreamSynchronize(g_stream)); /* host staging is freed next */
  d->entries = entries, d->coupling = coupling, d->height = height, d->setup_s = seconds;
  if (sv->o.verbose && m == 1)
    fprintf(stderr, "hip_cdna4: direct: %u row groups in %u workgroups, windows of up to %u doubles in LDS, %.1f MB on "
                    "the device\n", ngrp, nblk, widest_all, 1e-6 * (8.0 * (double)entries + 36.0 * n));
  else if (sv->o.verbose)
    fprintf(stderr, "hip_cdna4: direct: %u tiers, %u row groups in %u workgroups, windows of up to %u doubles in LDS, "
                    "%u + %u groups of coupling rows, %u launches per round, %.1f MB on the device\n",
            m, ngrp, nblk, widest_all, ncg, ntg, 4 * m - 2,
            1e-6 * (8.0 * (double)entries + 24.0 * (double)coupling + 52.0 * n));
  free(grp), free(blk), free(bwin), free(cgrp), free(tgrp);
  lsb_tierinv_free(T);
  sv->dir = d;
}

void direct_free(lsb_hip_solver *sv) {
  struct direct_dev *d = sv->dir;
  if (!d)
    return;
  graph_drop(&d->graphs);
  direct_multi_free(sv);
  for (unsigned i = 0; i < sizeof d->mem / sizeof d->mem[0]; i++)
    lsb_hip_free(d->mem[i]);
  lsb_hip_free(d->d_t);
  lsb_hip_free(d->d_z);
  free(d);
  sv->dir = NULL;
}

/* One application x (+)= P^T L^-T L^-1 P r: 4 m - 2 launches, two at one tier.  fixed: an application on its own
 * (reads d_b whatever the state says, stores x) */
static void direct_tier_enqueue(lsb_hip_solver *sv, const double *d_b, const double *d_r, double *d_x, int fixed) {
  struct shard *s = &sv->sh[0];
  struct direct_dev *d = sv->dir;
  const struct lsb_dirt_dev *k = &d->k;
  double *y = d->d_t, *z = d->d_z;
  lsb_k_dirt_rows(k, 0, d_b, d_r, NULL, y, s->d_st, fixed, g_stream);
  for (unsigned t = 1; t < k->ntier; t++) {
    lsb_k_dirt_fwd(k, t, d_b, d_r, y, z, s->d_st, fixed, g_stream);
    lsb_k_dirt_rows(k, t, NULL, NULL, z, y, s->d_st, fixed, g_stream);
  }
  for (unsigned t = k->ntier; t-- > 0;) {
    lsb_k_dirt_cols(k, t, y, z, d_x, s->d_st, fixed, g_stream);
    if (t > 0)
      lsb_k_dirt_bwd(k, t, z, y, s->d_st, g_stream);
  }
}

/* the same launches on a block of k->kp interleaved columns: Y = k->p, Z = k->q (NULL at one tier: dirm_setup) */
void direct_tier_enqueue_m(lsb_hip_solver *sv, const struct block_work *k, const struct lsb_mrhs_state *st) {
  const struct lsb_dirt_dev *d = &sv->dir->k;
  double *y = k->p, *z = k->q;
  lsb_k_dirt_rows_m(k->kp, d, 0, k->b, k->r, NULL, y, st, g_stream);
  for (unsigned t = 1; t < d->ntier; t++) {
    lsb_k_dirt_fwd_m(k->kp, d, t, k->b, k->r, y, z, st, g_stream);
    lsb_k_dirt_rows_m(k->kp, d, t, NULL, NULL, z, y, st, g_stream);
  }
  for (unsigned t = d->ntier; t-- > 0;) {
    lsb_k_dirt_cols_m(k->kp, d, t, y, z, k->x, st, g_stream);
    if (t > 0)
      lsb_k_dirt_bwd_m(k->kp, d, t, z, y, st, g_stream);
  }
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
    direct_tier_enqueue(e->sv, e->d_b, s->d_r, e->d_x, 0);
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
  LSB_CHK_HIP(hipMemsetAsync(&s->d_st->status, 0, sizeof(int), g_stream)); /* the launches are gated on it */
  direct_tier_enqueue(sv, d_r, d_r, d_z, 1);
  drain_stream(sv, "lsb_hip_solver_precond_dev");
  return 0;
}

/* Bytes a round streams on a block of width kp (kp = 1: a single solve), fixed + kp per_column.
 * One tier, two launches: W twice with first / woff per row twice (16 per entry, 24 n) whatever the width; per column
 *   P V in, T out and in, X out (32 n).
 * Tiered, 4 m - 2 launches: the W_tt twice with first / woff per row twice, C and C^T once each at 12 B an entry (24
 *   per coupling entry), their offsets (8 n); per column the block vectors, 8 B per row and pass, every row in one
 *   tier: k_dirt_fwd reads P V and writes Z (tier 0: k_dirt_rows reads P V), k_dirt_rows reads Z and writes Y,
 *   k_dirt_cols reads Y and writes Z and X, k_dirt_bwd reads and writes Y -- nine passes, 72 n.  The gathers of Y by C
 *   and of Z by C^T are left out. */
unsigned long long direct_round_bytes(const lsb_hip_solver *sv, unsigned kp) {
  const struct direct_dev *d = sv->dir;
  if (!direct_tiered(sv))
    return 16ull * d->entries + (24ull + 32ull * kp) * d->k.n;
  return 16ull * d->entries + 24ull * d->coupling + (24ull + 8ull) * d->k.n + 72ull * kp * d->k.n;
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
  if (bytes_per_round)
    *bytes_per_round = direct_round_bytes(sv, 1);
  return 0;
}

int lsb_hip_solver_direct_tier_info(const lsb_hip_solver *sv, unsigned *ntiers, unsigned long long *w_entries,
                                    unsigned long long *coupling_entries, unsigned *tier_rows,
                                    unsigned *launches_per_round) {
  if (!sv || !sv->dir)
    return 2;
  const struct direct_dev *d = sv->dir;
  const unsigned m = d->k.ntier;
  if (ntiers)
    *ntiers = m;
  if (w_entries)
    *w_entries = d->entries;
  if (coupling_entries)
    *coupling_entries = d->coupling;
  for (unsigned t = 0; tier_rows && t < LSB_DIRECT_MAX_TIERS; t++)
    tier_rows[t] = t < m ? d->k.t[t].hi - d->k.t[t].lo : 0;
  if (launches_per_round)
    *launches_per_round = 4 * m - 2;
  return 0;
}
