/* Geometric multigrid on the host side (LSB_PRECOND_GMG; rules: lsb_gmg.c; kernels: hip_gmg.hip): what it refuses,
 * the set-up of a shard's levels at solver creation (untimed) -- numbers only, the one upload is the coarsest level's
 * dense inverse --, the schedule of the V-cycle, and what the C-ABI answers about it. */
#define _GNU_SOURCE
#include "hip_solver.h"

/* ---- refusals ------------ */
void gmg_check(const struct lsb_hip_opts *o, int sharded) {
  if (o->precond != LSB_PRECOND_GMG)
    return;
  if (sharded || o->nvirt > 1)
    errx(EXIT_FAILURE, "hip_cdna4: --precond gmg runs on one shard (every level couples all rows of the grid); use it "
                       "without --ngpus / --nvirt");
  if (o->reorder)
    errx(EXIT_FAILURE, "hip_cdna4: --precond gmg needs the grid's own numbering: not with a re-ordered operator "
                       "(opts.reorder)");
  if (o->krylov != LSB_KRYLOV_PCG && o->krylov != LSB_KRYLOV_AUTO)
    errx(EXIT_FAILURE, "hip_cdna4: --precond gmg runs under classic PCG (--krylov cg or auto), not %s",
         o->krylov == LSB_KRYLOV_GMRES      ? "gmres"
         : o->krylov == LSB_KRYLOV_PCG1     ? "cg1"
         : o->krylov == LSB_KRYLOV_BICGSTAB ? "bicgstab"
         : o->krylov == LSB_KRYLOV_RICHARDSON ? "richardson"
                                              : "direct");
  if (o->precision != LSB_PREC_FP64)
    errx(EXIT_FAILURE, "hip_cdna4: --precond gmg runs in fp64 (--precision fp64), not in fp32 or mixed precision");
}

/* ---- set-up ------------ */
static size_t gmg_rows(const struct lsb_gmg_level *p) { return (size_t)p->n[0] * p->n[1] * p->n[2]; }

void precond_shard_gmg(struct shard *s, const struct lsb_hip_opts *o) {
  if (s->row_begin != 0 || s->n != s->n_glob || !s->gmg_grid.dim)
    errx(EXIT_FAILURE, "hip_cdna4: --precond gmg runs on one shard (every level couples all rows of the grid); use it "
                       "without --ngpus / --nvirt");
  const double t0 = wall_seconds();
  const struct lsb_gmg_grid *g = &s->gmg_grid;
  struct gmg_dev *a = lsb_calloc(struct gmg_dev, 1);
  a->dim = g->dim;
  a->nu = o->amg_sweeps < 1 ? 1u : (o->amg_sweeps > 16 ? 16u : (unsigned)o->amg_sweeps);
  const int nlev = lsb_gmg_plan(g, o->amg_coarse < 1 ? 1u : (unsigned)o->amg_coarse,
                                o->amg_max_levels < 1 ? 1u : (unsigned)o->amg_max_levels, a->plan, LSB_GMG_MAX_LEVELS);
  if (nlev == -1)
    errx(EXIT_FAILURE, "hip_cdna4: --precond gmg: the grid %u x %u x %u is too thin: coarsening stops with more than "
                       "%d rows on the coarsest level (its inverse is dense)", g->n[0], g->n[1], g->n[2],
         LSB_GMG_COARSE_MAX);
  if (nlev < 1)
    errx(EXIT_FAILURE, "hip_cdna4: cannot plan the levels of --precond gmg");
  a->nlev = (unsigned)nlev;
  { /* the plain steps or the fused ones: LSBENCH_HIP_GMG_FUSE=0 is the A/B switch (the same bits) */
    const char *e = getenv("LSBENCH_HIP_GMG_FUSE");
    a->fused = a->nu == 1 && !(e && atoi(e) == 0);
  }
  const unsigned pitch = s->gmg_pitch ? s->gmg_pitch : g->n[0];
  if ((size_t)pitch * g->n[1] * g->n[2] != s->n)
    errx(EXIT_FAILURE, "hip_cdna4: cannot happen: a %u x %u x %u grid at pitch %u on a shard of %u rows", g->n[0],
         g->n[1], g->n[2], pitch, s->n);
  /* the levels as the kernels take them */
  for (unsigned l = 0; l < a->nlev; l++) {
    const struct lsb_gmg_level *p = &a->plan[l];
    struct lsb_gmg_lv *L = &a->lv[l];
    for (unsigned d = 0; d < 3; d++) {
      L->n[d] = p->n[d];
      L->nc[d] = l + 1 < a->nlev ? a->plan[l + 1].n[d] : 1;
      L->wlast[d] = p->delta[d] / (1.0 + p->delta[d]);
    }
    L->pitch = l ? p->n[0] : pitch;
    L->c = g->c, L->sigma = 4.0 / (double)(1u << g->dim);
    lsb_gmg_diagonals(g->dim, g->c, p->delta, L->D, L->w);
  }
  /* the vectors below the fine level, one allocation: b and two buffers per level (the coarsest: b and its solution) */
  size_t total = 0;
  for (unsigned l = 1; l < a->nlev; l++)
    total += 3 * ((gmg_rows(&a->plan[l]) + 31) & ~(size_t)31);
  if (total) {
    a->mem = (double *)lsb_hip_malloc(total * sizeof(double));
    LSB_CHK_HIP(hipMemsetAsync(a->mem, 0, total * sizeof(double), g_stream));
    double *p = a->mem;
    for (unsigned l = 1; l < a->nlev; l++) {
      const size_t len = (gmg_rows(&a->plan[l]) + 31) & ~(size_t)31;
      a->b[l] = p, a->buf[l][0] = p + len, a->buf[l][1] = p + 2 * len;
      p += 3 * len;
    }
  }
  /* the coarsest level: its operator, inverted densely on the host.  A one-level cycle on a line-padded grid applies
   * it in the padded numbering: zero rows and columns on the pad rows, whose z is then exactly 0 */
  const struct lsb_gmg_level *cl = &a->plan[a->nlev - 1];
  struct csr *C = lsb_gmg_level_csr(g->dim, g->c, cl);
  double *inv = lsb_amg_coarse_inverse(C, "--precond gmg", "the coarse inverse of --precond gmg");
  const unsigned m = C->nrows;
  a->nc = m;
  if (a->nlev == 1 && pitch != g->n[0]) {
    const unsigned np = s->n;
    if (np > LSB_GMG_COARSE_MAX)
      errx(EXIT_FAILURE, "hip_cdna4: --precond gmg: the grid %u x %u x %u is too thin: its one level has %u rows with "
                         "the lines padded to %u, more than %d (its inverse is dense)", g->n[0], g->n[1], g->n[2], np,
           pitch, LSB_GMG_COARSE_MAX);
    double *wide = lsb_calloc(double, (size_t)np * np);
    if (!wide)
      errx(EXIT_FAILURE, "hip_cdna4: out of host memory for the coarse inverse of --precond gmg (%u rows)", np);
    for (unsigned r = 0; r < m; r++)
      for (unsigned q = 0; q < m; q++)
        wide[((size_t)(r / g->n[0]) * pitch + r % g->n[0]) * np + (size_t)(q / g->n[0]) * pitch + q % g->n[0]] =
            inv[(size_t)r * m + q];
    free(inv);
    inv = wide, a->nc = np;
  }
  a->d_cinv = (double *)dev_upload(inv, (size_t)a->nc * a->nc * sizeof(double));
  a->clanes = row_lanes(a->nc);
  LSB_CHK_HIP(hipStreamSynchronize(g_stream));
  free(inv);
  lsb_csr_free(C);
  /* what one cycle streams (lsbench_hip.h, at lsb_hip_solver_gmg_cycle_bytes) */
  for (unsigned l = 0; l + 1 < a->nlev; l++) {
    const unsigned long long n = gmg_rows(&a->plan[l]), nn = gmg_rows(&a->plan[l + 1]);
    a->cycle_bytes += a->fused ? 40ull * n + 16ull * nn : (16ull + 24ull * (2ull * a->nu - 1ull) + 32ull) * n + 16ull * nn;
  }
  a->cycle_bytes += 8ull * a->nc * a->nc + 16ull * a->nc;
  a->setup_s = wall_seconds() - t0;
  if (o->verbose) {
    for (unsigned l = 0; l < a->nlev; l++)
      fprintf(stderr, "hip_cdna4: GMG level %u: %u x %u x %u points, delta %.6g %.6g %.6g%s\n", l, a->plan[l].n[0],
              a->plan[l].n[1], a->plan[l].n[2], a->plan[l].delta[0], a->plan[l].delta[1], a->plan[l].delta[2],
              l + 1 == a->nlev ? ", dense coarse inverse" : "");
    fprintf(stderr, "hip_cdna4: GMG %u-D, %u levels, %u damped Jacobi sweep%s, %s steps, %llu bytes per application, "
                    "set-up %.3f s\n", a->dim, a->nlev, a->nu, a->nu > 1 ? "s" : "", a->fused ? "fused" : "plain",
            a->cycle_bytes, a->setup_s);
  }
  s->gmg = a;
}

void gmg_finish_setup(struct shard *s) {
  struct gmg_dev *a = s->gmg;
  if (a->nlev < 2)
    return;
  a->buf[0][0] = shard_vec(s, s->n);
  LSB_CHK_HIP(hipMemsetAsync(a->buf[0][0], 0, (size_t)s->n * sizeof(double), g_stream));
  LSB_CHK_HIP(hipStreamSynchronize(g_stream));
}

void gmg_free(struct shard *s) {
  struct gmg_dev *a = s->gmg;
  if (!a)
    return;
  shard_vec_free(s, a->buf[0][0]);
  lsb_hip_free(a->mem), lsb_hip_free(a->d_cinv);
  free(a);
  s->gmg = NULL;
}

/* ---- the V-cycle ------------
 * A level's iterate ping-pongs between buf[0] and buf[1] as AMG's does (amg_cycle): down x = w b into buf[0], nu - 1
 * sweeps, the residual restricted into the next level's b; up the prolongation added where the way down left the
 * iterate, then nu sweeps -- 2 nu - 1 out-of-place steps in all, so the last one writes buf[1], on the fine level the
 * caller's z.  nu = 1 fused: k_gmg_down writes buf[0] and the next b, k_gmg_up reads buf[0] and writes buf[1].  Allocates
 * nothing and synchronises nothing: it may run inside a stream capture. */
void gmg_cycle(const struct shard *s, const double *r, double *z, const struct lsb_pcg_state *st) {
  const struct gmg_dev *a = s->gmg;
  const unsigned nu = a->nu, top = a->nlev - 1, dim = a->dim;
  for (unsigned l = 0; l < top; l++) {
    const double *b = l ? a->b[l] : r;
    double *const buf[2] = {a->buf[l][0], l ? a->buf[l][1] : z};
    if (a->fused) {
      lsb_k_gmg_down(dim, &a->lv[l], b, buf[0], a->b[l + 1], st, g_stream);
      continue;
    }
    unsigned at = 0;
    lsb_k_gmg_first(dim, &a->lv[l], b, buf[0], st, g_stream);
    for (unsigned k = 1; k < nu; k++, at ^= 1)
      lsb_k_gmg_sweep(dim, &a->lv[l], buf[at], b, buf[at ^ 1], st, g_stream);
    lsb_k_gmg_restrict(dim, &a->lv[l], buf[at], b, a->b[l + 1], st, g_stream);
  }
  lsb_k_amg_dense(a->nc, a->clanes, a->d_cinv, top ? a->b[top] : r, top ? a->buf[top][1] : z, st, g_stream);
  for (unsigned l = top; l-- > 0;) {
    const double *b = l ? a->b[l] : r;
    double *const buf[2] = {a->buf[l][0], l ? a->buf[l][1] : z};
    if (a->fused) {
      lsb_k_gmg_up(dim, &a->lv[l], buf[0], b, a->buf[l + 1][1], buf[1], st, g_stream);
      continue;
    }
    unsigned at = (nu - 1) % 2;
    lsb_k_gmg_prolong(dim, &a->lv[l], buf[at], a->buf[l + 1][1], st, g_stream);
    for (unsigned k = 0; k < nu; k++, at ^= 1)
      lsb_k_gmg_sweep(dim, &a->lv[l], buf[at], b, buf[at ^ 1], st, g_stream);
  }
}

/* ---- what the C-ABI answers ------------ */
static const struct gmg_dev *gmg_of(const lsb_hip_solver *sv) {
  return sv && sv->o.precond == LSB_PRECOND_GMG ? sv->sh[0].gmg : NULL;
}

int lsb_hip_solver_gmg_info(lsb_hip_solver *sv, unsigned *levels, unsigned dims[3], unsigned *pitch) {
  if (!lsb_initialized)
    return 1;
  const struct gmg_dev *a = gmg_of(sv);
  if (!a)
    return 2;
  if (levels)
    *levels = a->nlev;
  for (unsigned d = 0; dims && d < 3; d++)
    dims[d] = a->plan[0].n[d];
  if (pitch)
    *pitch = a->lv[0].pitch;
  return 0;
}

int lsb_hip_solver_gmg_level(lsb_hip_solver *sv, unsigned level, unsigned n[3], double delta[3]) {
  if (!lsb_initialized)
    return 1;
  const struct gmg_dev *a = gmg_of(sv);
  if (!a || level >= a->nlev)
    return 2;
  for (unsigned d = 0; d < 3; d++) {
    if (n)
      n[d] = a->plan[level].n[d];
    if (delta)
      delta[d] = a->plan[level].delta[d];
  }
  return 0;
}

unsigned long long lsb_hip_solver_gmg_cycle_bytes(const lsb_hip_solver *sv) {
  const struct gmg_dev *a = gmg_of(sv);
  return a ? a->cycle_bytes : 0;
}
