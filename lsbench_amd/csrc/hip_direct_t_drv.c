/* The direct solver on a tiered inverse factor: the host driver (kernels: hip_direct_t.hip; the factor: lsb_direct.c,
 * struct lsb_tierinv; the solves themselves: hip_direct_drv.c, which dispatches on direct_dev.tier). */
#define _GNU_SOURCE
#include "hip_solver.h"

/*
 * lsb_hip_solver_create_direct(A, opts, tiers).  The single skyline W = L^-1 has n + sum |below| |separator| entries,
 * which is why hip_direct_drv.c refuses operators of more than a few tens of thousands of rows.  Nearly all of them
 * are the dense rows of the high separators over everything below.  Here the tree is cut into tiers by subtree size,
 * only the diagonal blocks W_tt = (L_tt)^-1 are kept as skylines, and the blocks below the diagonal stay what they
 * are in L: sparse.  An application is a block forward and a block backward substitution over the tiers, 4 m - 2
 * launches for m tiers, ordered by the launches alone.
 *
 * Creation as for the single skyline: ordered (lsb_csr_nd, unbounded: the bound is the single skyline's), counted
 * (lsb_csr_tiered_count; tiers = 0 takes the fewest that fit) and factorised on the host before anything is
 * allocated on the device.  tiers = 1 is lsb_hip_solver_create itself.  The solves, the warm starts, the sequences
 * and opts.verify are hip_direct_drv.c's: a round there calls direct_tier_enqueue instead of its two launches.
 * Blocks of right-hand sides: lsb_hip_solver_solve_direct_multi[_dev] and its companions keep answering 2 on a tiered
 * solver; lsb_hip_solver_solve_direct_tier_multi[_dev] (hip_direct_m_drv.c) serve it, a round of theirs calls
 * direct_tier_enqueue_m, the same launches in their block form (hip_direct_tm.hip).
 *
 * Two vectors of its own: y (direct_dev.d_t) and z, in the tier-major numbering.
 */

struct lsb_tierinv *direct_tier_factor(const struct csr *S, const struct lsb_hip_opts *o, int tiers, unsigned *height,
                                       double *seconds) {
  const double t0 = wall_seconds();
  const unsigned n = S->nrows;
  unsigned *perm = (unsigned *)malloc((size_t)(n ? n : 1) * sizeof(unsigned));
  if (!perm || lsb_csr_nd(S, perm))
    errx(EXIT_FAILURE, "hip_cdna4: --krylov direct: out of memory computing the nested-dissection ordering");
  unsigned long long w = 0, c = 0;
  unsigned m = tiers ? (unsigned)tiers : 1;
  for (;; m++) { /* tiers = 0: the fewest that fit, by the symbolic count alone */
    if (lsb_csr_tiered_count(S, perm, m, &w, &c, height))
      errx(EXIT_FAILURE, "hip_cdna4: --krylov direct: out of memory counting the tiered inverse factor");
    if (w + 3 * c <= LSB_DIRECT_MAX_ENTRIES || tiers || m == LSB_DIRECT_MAX_TIERS)
      break;
  }
  if (w + 3 * c > LSB_DIRECT_MAX_ENTRIES)
    errx(EXIT_FAILURE, "hip_cdna4: --krylov direct: in %u tiers the inverse factor of this operator (%u rows) has %llu "
                       "entries and its coupling %llu, which count three times: more than the %llu entries it may "
                       "have (LSB_DIRECT_MAX_ENTRIES)%s",
         m, n, w, c, (unsigned long long)LSB_DIRECT_MAX_ENTRIES,
         tiers ? "" : "; that is the largest number of tiers there is (LSB_DIRECT_MAX_TIERS)");
  int why = 0;
  struct lsb_tierinv *T = lsb_csr_tiered_inverse(S, perm, m, &why);
  free(perm);
  if (why == 1)
    errx(EXIT_FAILURE, "hip_cdna4: --krylov direct needs a symmetric positive definite operator (a pivot of its "
                       "Cholesky factor is <= 0 or not finite)");
  if (!T)
    errx(EXIT_FAILURE, "hip_cdna4: --krylov direct: out of memory computing the tiered inverse factor");
  *seconds = wall_seconds() - t0;
  if (o->verbose)
    fprintf(stderr, "hip_cdna4: direct: nested dissection, %u rows in %u tiers (%u asked for), %llu entries of the "
                    "W_tt and %llu of the coupling, tree height %u, %.1f MB, set up in %.3f s on the host\n",
            n, T->ntier, m, w, c, *height, 1e-6 * (8.0 * (double)w + 24.0 * (double)c), *seconds);
  return T;
}

/* the rows r0 .. r1 - 1 of a CSR (offs[row - base]) in groups of consecutive rows with one lane count, appended to
 * grp at *ngrp */
static void tier_deal_csr(const unsigned *offs, unsigned base, unsigned r0, unsigned r1, unsigned *grp,
                          unsigned *ngrp) {
  for (unsigned k = r0; k < r1;) {
    const unsigned L = direct_row_lanes(offs[k - base + 1] - offs[k - base]);
    unsigned nr = 1;
    while (k + nr < r1 && nr < 64 / L && direct_row_lanes(offs[k + nr - base + 1] - offs[k + nr - base]) == L)
      nr++;
    grp[2 * *ngrp] = k, grp[2 * *ngrp + 1] = nr << 8 | L, (*ngrp)++;
    k += nr;
  }
}

void direct_tier_upload(lsb_hip_solver *sv, struct lsb_tierinv *T, unsigned height, double seconds) {
  const unsigned n = T->n, m = T->ntier, lo1 = T->lo[m > 1 ? 1 : m];
  struct direct_dev *d = lsb_calloc(struct direct_dev, 1);
  struct direct_tier_dev *q = lsb_calloc(struct direct_tier_dev, 1);
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
    errx(EXIT_FAILURE, "hip_cdna4: --krylov direct: the tiered inverse factor is malformed");
  /* the dealing, tier by tier: no group, workgroup or window straddles a tier */
  unsigned *grp = lsb_calloc(unsigned, 2 * (size_t)n), *blk = lsb_calloc(unsigned, (size_t)n + 1);
  unsigned *bwin = lsb_calloc(unsigned, 2 * (size_t)n), ngrp = 0, nblk = 0;
  unsigned *cgrp = lsb_calloc(unsigned, 2 * (size_t)n), ncg = 0;
  unsigned *tgrp = lsb_calloc(unsigned, 2 * (size_t)(nt ? nt : 1)), ntg = 0;
  unsigned widest_all = 0;
  /* LSBENCH_HIP_DIRECT_TIER_LDS: fewer doubles of a window staged than the launch could (for the tests, which reach
   * the gathered windows on small operators with it) */
  const char *env = getenv("LSBENCH_HIP_DIRECT_TIER_LDS");
  const unsigned cap = env && atoi(env) > 0 ? (unsigned)atoi(env) : 0;
  for (unsigned t = 0; t < m; t++) {
    struct lsb_dirt_tier *k = &q->k.t[t];
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
  q->k.n = n, q->k.ntier = m;
  unsigned u = 0;
  q->k.vals = q->mem[u++] = dev_upload(T->vals, (size_t)(entries ? entries : 1) * sizeof(double));
  q->k.woff = q->mem[u++] = dev_upload(T->woff, ((size_t)n + 1) * sizeof(unsigned long long));
  q->k.first = q->mem[u++] = dev_upload(T->first, (size_t)n * sizeof(unsigned));
  q->k.perm = q->mem[u++] = dev_upload(T->perm, (size_t)n * sizeof(unsigned));
  q->k.parent = q->mem[u++] = dev_upload(T->parent, (size_t)n * sizeof(unsigned));
  q->k.run_end = q->mem[u++] = dev_upload(T->run_end, (size_t)n * sizeof(unsigned));
  q->k.grp = q->mem[u++] = dev_upload(grp, 2 * (size_t)ngrp * sizeof(unsigned));
  q->k.blk = q->mem[u++] = dev_upload(blk, ((size_t)nblk + 1) * sizeof(unsigned));
  q->k.bwin = q->mem[u++] = dev_upload(bwin, 2 * (size_t)nblk * sizeof(unsigned));
  q->k.coffs = q->mem[u++] = dev_upload(T->coffs, ((size_t)(n - lo1) + 1) * sizeof(unsigned));
  q->k.ccols = q->mem[u++] = dev_upload(T->ccols, (size_t)(coupling ? coupling : 1) * sizeof(unsigned));
  q->k.cvals = q->mem[u++] = dev_upload(T->cvals, (size_t)(coupling ? coupling : 1) * sizeof(double));
  q->k.toffs = q->mem[u++] = dev_upload(T->toffs, (nt ? nt : 1) * sizeof(unsigned));
  q->k.tcols = q->mem[u++] = dev_upload(T->tcols, (size_t)(coupling ? coupling : 1) * sizeof(unsigned));
  q->k.tvals = q->mem[u++] = dev_upload(T->tvals, (size_t)(coupling ? coupling : 1) * sizeof(double));
  q->k.cgrp = q->mem[u++] = dev_upload(cgrp, 2 * (size_t)(ncg ? ncg : 1) * sizeof(unsigned));
  q->k.tgrp = q->mem[u++] = dev_upload(tgrp, 2 * (size_t)(ntg ? ntg : 1) * sizeof(unsigned));
  d->d_t = (double *)lsb_hip_malloc((size_t)n * sizeof(double));
  q->d_z = (double *)lsb_hip_malloc((size_t)n * sizeof(double));
  LSB_CHK_HIP(hipMemsetAsync(d->d_t, 0, (size_t)n * sizeof(double), g_stream));
  LSB_CHK_HIP(hipMemsetAsync(q->d_z, 0, (size_t)n * sizeof(double), g_stream));
  LSB_CHK_HIP(hipStreamSynchronize(g_stream)); /* host staging is freed next */
  q->coupling = coupling;
  d->k.n = n, d->entries = entries, d->height = height, d->setup_s = seconds, d->tier = q;
  if (sv->o.verbose)
    fprintf(stderr, "hip_cdna4: direct: %u tiers, %u row groups in %u workgroups, windows of up to %u doubles in LDS, "
                    "%u + %u groups of coupling rows, %u launches per round, %.1f MB on the device\n",
            m, ngrp, nblk, widest_all, ncg, ntg, 4 * m - 2,
            1e-6 * (8.0 * (double)entries + 24.0 * (double)coupling + 52.0 * n));
  free(grp), free(blk), free(bwin), free(cgrp), free(tgrp);
  lsb_tierinv_free(T);
  sv->dir = d;
}

void direct_tier_free(lsb_hip_solver *sv) {
  struct direct_tier_dev *q = sv->dir ? sv->dir->tier : NULL;
  if (!q)
    return;
  for (unsigned i = 0; i < sizeof q->mem / sizeof q->mem[0]; i++)
    lsb_hip_free(q->mem[i]);
  lsb_hip_free(q->d_z);
  free(q);
  sv->dir->tier = NULL;
}

/* fixed: one application on its own (reads d_b whatever the state says, stores x) */
void direct_tier_enqueue(lsb_hip_solver *sv, const double *d_b, const double *d_r, double *d_x, int fixed) {
  struct shard *s = &sv->sh[0];
  struct direct_dev *d = sv->dir;
  const struct lsb_dirt_dev *k = &d->tier->k;
  double *y = d->d_t, *z = d->tier->d_z;
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

/* the 4 m - 2 launches of a round: the W_tt twice with first / woff per row twice; C and C^T once each at 12 B an
 * entry (24 per coupling entry), their offsets; P r in, y and z out and in, x out */
unsigned long long direct_tier_round_bytes(const lsb_hip_solver *sv) {
  const struct direct_dev *d = sv->dir;
  return 16ull * d->entries + 24ull * d->tier->coupling + (24ull + 32ull + 8ull + 40ull) * d->k.n;
}

/* the same launches on a block of k->kp interleaved columns: Y = k->p, Z = k->q */
void direct_tier_enqueue_m(lsb_hip_solver *sv, const struct block_work *k, const struct lsb_mrhs_state *st) {
  const struct lsb_dirt_dev *d = &sv->dir->tier->k;
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

/* A round on a block of width kp: fixed + kp per_column.
 *   fixed      what is loaded once for all columns: the W_tt twice (16 per entry) with first / woff per row twice
 *              (24 n), C and C^T once each at 12 B an entry (24 per coupling entry), their offsets (8 n)
 *   per_column the block vectors, 8 B per row and pass, every row in one tier: k_dirt_fwd_m reads P V and writes Z
 *              (tier 0: k_dirt_rows_m reads P V), k_dirt_rows_m reads Z and writes Y, k_dirt_cols_m reads Y and writes
 *              Z and X, k_dirt_bwd_m reads and writes Y -- nine passes, 72 n.  The gathers of Y by C and of Z by C^T
 *              are left out, as they are at one column
 * kp = 1 is direct_tier_round_bytes: 32 n + 72 n = 104 n. */
unsigned long long direct_tier_multi_round_bytes(const lsb_hip_solver *sv, unsigned kp) {
  const struct direct_dev *d = sv->dir;
  return 16ull * d->entries + 24ull * d->tier->coupling + (24ull + 8ull) * d->k.n + 72ull * kp * d->k.n;
}

int lsb_hip_solver_direct_tier_info(const lsb_hip_solver *sv, unsigned *ntiers, unsigned long long *w_entries,
                                    unsigned long long *coupling_entries, unsigned *tier_rows,
                                    unsigned *launches_per_round) {
  if (!sv || !sv->dir)
    return 2;
  const struct direct_dev *d = sv->dir;
  const unsigned m = d->tier ? d->tier->k.ntier : 1;
  if (ntiers)
    *ntiers = m;
  if (w_entries)
    *w_entries = d->entries;
  if (coupling_entries)
    *coupling_entries = d->tier ? d->tier->coupling : 0;
  for (unsigned t = 0; tier_rows && t < LSB_DIRECT_MAX_TIERS; t++)
    tier_rows[t] = t >= m ? 0 : d->tier ? d->tier->k.t[t].hi - d->tier->k.t[t].lo : d->k.n;
  if (launches_per_round)
    *launches_per_round = 4 * m - 2;
  return 0;
}
