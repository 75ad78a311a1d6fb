/* AMG on the host side (LSB_PRECOND_AMG; hierarchy: lsb_amg.c; kernels: hip_amg.hip, hip_amg_cheb.hip,
 * hip_amg_f32.hip, hip_amg_f32_m.hip, hip_amg_mcgs.hip, hip_mrhs_amg.hip): the upload of the hierarchy at solver
 * creation (untimed), the ONE schedule of the V-cycle that all four flavours run -- fp64 or fp32, on one column or on
 * blocks of columns -- and what the C-ABI answers about it. */
#define _GNU_SOURCE
#include "hip_solver.h"

/* ---- set-up: the hierarchy of lsb_amg.c in the solver's precision on the device ------------ */
static void *amg_keep(struct amg_dev *a, void *p) {
  a->mem[a->nmem++] = p;
  return p;
}

/* what the uploads of both precisions check and pick: fewer than 2^31 entries; lanes from the mean row length */
static unsigned amg_mat_lanes(const struct csr *M) {
  const unsigned n = M->nrows;
  const unsigned long long nnz = M->offs[n];
  if (nnz > 0x7fffffffull)
    errx(EXIT_FAILURE, "hip_cdna4: an AMG operator has %llu entries, more than 2^31 - 1", nnz);
  return row_lanes(n ? (unsigned)((nnz + n - 1) / n) : 1);
}

static struct lsb_amg_mat amg_upload_mat(struct amg_dev *a, const struct csr *M) {
  struct lsb_amg_mat m;
  const unsigned n = M->nrows;
  const unsigned long long nnz = M->offs[n];
  m.lanes = amg_mat_lanes(M);
  m.rows = n;
  m.offs = (const int *)amg_keep(a, dev_upload(M->offs, ((size_t)n + 1) * sizeof(unsigned)));
  m.cols = (const int *)amg_keep(a, dev_upload(M->cols, (size_t)(nnz ? nnz : 1) * sizeof(unsigned)));
  m.vals = (const double *)amg_keep(a, dev_upload(M->vals, (size_t)(nnz ? nnz : 1) * sizeof(double)));
  return m;
}

/* fp32: offsets and packed {column, float} entries; the fp64 values stay on the host */
static struct amg_mat32 amg_upload_mat32(struct amg_dev *a, const struct csr *M, const char *what, unsigned l) {
  struct amg_mat32 m;
  const unsigned n = M->nrows;
  const unsigned long long nnz = M->offs[n];
  m.lanes = amg_mat_lanes(M);
  unsigned long long *w = lsb_csr_pack_f32(M);
  if (!w)
    errx(EXIT_FAILURE, "hip_cdna4: --amg-precision fp32: an entry of %s on level %u is not finite in fp32; use "
                       "--amg-precision fp64", what, l);
  m.rows = n;
  m.offs = (const int *)amg_keep(a, dev_upload(M->offs, ((size_t)n + 1) * sizeof(unsigned)));
  m.ent = (const unsigned long long *)amg_keep(a, dev_upload(w, (size_t)(nnz ? nnz : 1) * sizeof *w));
  LSB_CHK_HIP(hipStreamSynchronize(g_stream));
  free(w);
  return m;
}

/* a float copy of cnt doubles on the device; refuses what does not fit */
static float *amg_upload_f32(struct amg_dev *a, const double *v, size_t cnt, const char *what) {
  float *f = (float *)malloc((cnt ? cnt : 1) * sizeof(float));
  if (!f)
    errx(EXIT_FAILURE, "hip_cdna4: out of host memory for the fp32 AMG hierarchy");
  f[0] = 0.0f;
  for (size_t i = 0; i < cnt; i++) {
    f[i] = (float)v[i];
    if (!isfinite(v[i]) || isinf(f[i]))
      errx(EXIT_FAILURE, "hip_cdna4: --amg-precision fp32: an entry of %s is not finite in fp32; use "
                         "--amg-precision fp64", what);
  }
  float *d = (float *)amg_keep(a, dev_upload(f, (cnt ? cnt : 1) * sizeof(float)));
  LSB_CHK_HIP(hipStreamSynchronize(g_stream));
  free(f);
  return d;
}

static void *amg_zeros(struct amg_dev *a, size_t bytes) {
  void *p = amg_keep(a, lsb_hip_malloc(bytes));
  LSB_CHK_HIP(hipMemsetAsync(p, 0, bytes, g_stream));
  return p;
}

/* a level below the fine one: its four vectors of n elements of `elem` bytes, one allocation */
static void amg_level_vecs(struct amg_dev *a, struct amg_vecs *v, size_t n, size_t elem) {
  char *buf = (char *)amg_zeros(a, 4 * n * elem);
  v->b = buf, v->out = buf + n * elem, v->tmp = buf + 2 * n * elem, v->r = buf + 3 * n * elem;
}

/* level l in fp64: the matrices, the Chebyshev direction, minv, the vectors */
static void amg_upload_level(struct amg_dev *a, unsigned l, const struct lsb_amg_level *H, const double *minv) {
  struct amg_lv *L = &a->lv[l];
  L->A.d = amg_upload_mat(a, H->A);
  if (H->P) {
    L->P.d = amg_upload_mat(a, H->P);
    L->R.d = amg_upload_mat(a, H->R);
  }
  if (a->cheb && H->P)
    a->vec[l].d = amg_zeros(a, (size_t)H->n * sizeof(double));
  L->minv = amg_keep(a, dev_upload(minv, (size_t)(H->n ? H->n : 1) * sizeof(double)));
  if (l > 0) /* level 0: the caller's r and z; its two other vectors come out of the slab (amg_finish_setup) */
    amg_level_vecs(a, &a->vec[l], H->n, sizeof(double));
}

/* level l in fp32: the packed matrices, minv, the Chebyshev direction, the vectors */
static void amg_upload_level32(struct amg_dev *a, unsigned l, const struct lsb_amg_level *H, const double *minv) {
  struct amg_lv *L = &a->lv[l];
  L->A.f = amg_upload_mat32(a, H->A, "A", l);
  if (H->P) {
    L->P.f = amg_upload_mat32(a, H->P, "P", l);
    L->R.f = amg_upload_mat32(a, H->R, "R", l);
  }
  L->minv = amg_upload_f32(a, minv, H->n, "the smoother's diagonal");
  if (a->cheb && H->P)
    a->vec[l].d = amg_zeros(a, (size_t)(H->n ? H->n : 1) * sizeof(float));
  if (l > 0) /* level 0: halves of the two slab vectors (amg_finish_setup) */
    amg_level_vecs(a, &a->vec[l], H->n, sizeof(float));
}

/* Multicolour Gauss-Seidel on level l (LSB_AMG_SMOOTH_MCGS): colour it and, where the colouring stays within the
 * cap, sort the copy, check it and upload it in the solver's precision (the fp64 values stay on the host under
 * fp32).  0: the level has more colours than the cap and keeps l1-Jacobi.  m0 / n0: colour 0's entries and rows. */
static int amg_upload_mcgs(struct amg_dev *a, unsigned l, const struct lsb_amg_level *H, unsigned long long *m0,
                           unsigned *n0) {
  struct amg_lv *L = &a->lv[l];
  const unsigned n = H->n;
  unsigned nc = 0;
  int *colour = lsb_amg_colour(H->A, &nc);
  L->ncol_found = nc;
  if (nc > a->mcgs_cap) {
    free(colour);
    return 0;
  }
  struct lsb_mcgs *M = lsb_csr_mcgs(H->A, colour, nc);
  char why[256] = "no copy";
  const int rc = M ? lsb_mcgs_check(H->A, colour, M, why, sizeof why) : 1;
  if (rc)
    errx(EXIT_FAILURE, "hip_cdna4: --amg-smoother mcgs: level %u (%u rows, %u colours) fails the check of its "
                       "colour-sorted copy (%d): %s", l, n, nc, rc, why);
  const struct csr view = {n, 0, M->offs, M->cols, M->vals};
  const unsigned long long nnz = M->offs[n];
  if (a->prec == LSB_AMG_PREC_FP32)
    L->C.f = amg_upload_mat32(a, &view, "A", l);
  else
    L->C.d = amg_upload_mat(a, &view);
  unsigned char *c8 = (unsigned char *)malloc(n ? n : 1);
  if (!c8)
    errx(EXIT_FAILURE, "hip_cdna4: out of host memory for the colours of an AMG level");
  for (unsigned i = 0; i < n; i++)
    c8[i] = (unsigned char)colour[i]; /* (the cap is at most 64) */
  L->rowid = (const int *)amg_keep(a, dev_upload(M->rowid, (size_t)(n ? n : 1) * sizeof(unsigned)));
  L->colour8 = (const unsigned char *)amg_keep(a, dev_upload(c8, n ? n : 1));
  LSB_CHK_HIP(hipStreamSynchronize(g_stream));
  L->cbeg = lsb_calloc(unsigned, (size_t)nc + 1);
  memcpy(L->cbeg, M->cbeg, ((size_t)nc + 1) * sizeof(unsigned));
  L->ncol = nc;
  *m0 = M->offs[M->cbeg[1]], *n0 = M->cbeg[1];
  a->mcgs_bytes += 4ull * (n + 1) + (a->prec == LSB_AMG_PREC_FP32 ? 8ull : 12ull) * nnz + 5ull * n;
  free(c8), free(colour);
  lsb_mcgs_free(M);
  return 1;
}

static void amg_report(const struct amg_dev *a, const struct lsb_amg_hier *h, double ratio) {
  const int f32 = a->prec == LSB_AMG_PREC_FP32;
  unsigned long long nnz0 = h->lv[0].A->offs[h->lv[0].n], nnzall = 0;
  for (unsigned l = 0; l < h->nlev; l++) {
    const struct lsb_amg_level *H = &h->lv[l];
    const struct amg_lv *L = &a->lv[l];
    nnzall += H->A->offs[H->n];
    fprintf(stderr, "hip_cdna4: AMG level %u: %u rows, %u entries, %u lanes (A)", l, H->n, H->A->offs[H->n],
            f32 ? L->A.f.lanes : L->A.d.lanes);
    if (H->P)
      fprintf(stderr, ", %u / %u lanes (P / R)", f32 ? L->P.f.lanes : L->P.d.lanes, f32 ? L->R.f.lanes : L->R.d.lanes);
    if (H->P && a->cheb)
      fprintf(stderr, ", Chebyshev on [%.4g, %.4g]\n", L->lo, L->hi);
    else if (H->P && a->mcgs && L->ncol)
      fprintf(stderr, ", Gauss-Seidel in %u colours\n", L->ncol);
    else if (H->P && a->mcgs)
      fprintf(stderr, ", l1-Jacobi (%u colours, more than %u)\n", L->ncol_found, a->mcgs_cap);
    else if (H->P)
      fprintf(stderr, "\n");
    else
      fprintf(stderr, ", dense coarse inverse, %u lanes\n", a->clanes);
  }
  if (a->cheb)
    fprintf(stderr, "hip_cdna4: AMG operator complexity %.3f, %u levels, Chebyshev smoother of degree %u "
                    "(interval ratio %g), set-up %.3f s\n", nnz0 ? (double)nnzall / nnz0 : 0.0, h->nlev, a->nu,
            ratio, a->setup_s);
  else if (a->mcgs)
    fprintf(stderr, "hip_cdna4: AMG operator complexity %.3f, %u levels, %u multicolour Gauss-Seidel sweep%s forward "
                    "and backward on levels of at most %u colours (l1-Jacobi elsewhere), colour-sorted copies %llu "
                    "bytes on the device, set-up %.3f s\n", nnz0 ? (double)nnzall / nnz0 : 0.0, h->nlev, a->nu,
            a->nu > 1 ? "s" : "", a->mcgs_cap, a->mcgs_bytes, a->setup_s);
  else
    fprintf(stderr, "hip_cdna4: AMG operator complexity %.3f, %u of %u levels in the one-launch tail, %u l1-Jacobi "
                    "sweep%s, set-up %.3f s\n", nnz0 ? (double)nnzall / nnz0 : 0.0, h->nlev - a->tail, h->nlev,
            a->nu, a->nu > 1 ? "s" : "", a->setup_s);
  if (f32)
    fprintf(stderr, "hip_cdna4: AMG V-cycle in fp32 (packed entries, float vectors): %llu bytes per application, "
                    "%llu in fp64\n", a->cycle_bytes32, a->cycle_mat_bytes + 8ull * a->cycle_vec_rows);
}

/* What one cycle streams in the precision it runs in, in two parts: its matrices, and its vector passes (on blocks:
 * per column).  fp64: cycle_mat_bytes and 8 B per element pass.  fp32: 8 B per entry, 4 nc^2, 4 B per element pass;
 * level 0: r read, z written at 8 B, the copy of r written */
void amg_cycle_bytes_split(const struct amg_dev *a, unsigned long long *mat, unsigned long long *vec) {
  const unsigned long long nc2 = (unsigned long long)a->nc * a->nc;
  if (a->prec == LSB_AMG_PREC_FP32) {
    *mat = (a->cycle_mat_bytes - 8ull * nc2) / 3ull * 2ull + 4ull * nc2;
    *vec = 4ull * a->cycle_vec_rows + (a->nlev > 1 ? 12ull * a->lv[0].n : 8ull * a->nc);
  } else {
    *mat = a->cycle_mat_bytes;
    *vec = 8ull * a->cycle_vec_rows;
  }
}

void precond_shard_amg(struct shard *s, const int *offs, const int *cols, const double *vals,
                       const struct lsb_hip_opts *o) {
  /* options and refusals */
  if (s->row_begin != 0 || s->n != s->n_glob)
    errx(EXIT_FAILURE, "hip_cdna4: --precond amg runs on one shard (the hierarchy couples all rows); use it "
                       "without --ngpus / --nvirt");
  if (o->krylov == LSB_KRYLOV_GMRES || o->krylov == LSB_KRYLOV_PCG1 || o->krylov == LSB_KRYLOV_BICGSTAB)
    errx(EXIT_FAILURE, "hip_cdna4: --precond amg runs under classic PCG (--krylov cg or auto), not %s",
         o->krylov == LSB_KRYLOV_GMRES ? "gmres" : o->krylov == LSB_KRYLOV_PCG1 ? "cg1" : "bicgstab");
  const int cheb = o->amg_smoother == LSB_AMG_SMOOTH_CHEB, f32 = o->amg_precision == LSB_AMG_PREC_FP32;
  const int mcgs = o->amg_smoother == LSB_AMG_SMOOTH_MCGS;
  if (o->amg_smoother != LSB_AMG_SMOOTH_L1JACOBI && !cheb && !mcgs)
    errx(EXIT_FAILURE, "hip_cdna4: no AMG smoother %d (--amg-smoother l1, cheb or mcgs)", o->amg_smoother);
  if (o->amg_precision != LSB_AMG_PREC_FP64 && !f32)
    errx(EXIT_FAILURE, "hip_cdna4: no AMG precision %d (--amg-precision fp64 or fp32)", o->amg_precision);
  const double ratio = o->amg_cheb_ratio >= 1.5 ? o->amg_cheb_ratio : 1.5;
  const unsigned coarse = o->amg_coarse < 1 ? 1u : (unsigned)o->amg_coarse;
  const unsigned maxlev = o->amg_max_levels < 1 ? 1u : (o->amg_max_levels > 64 ? 64u : (unsigned)o->amg_max_levels);
  /* the hierarchy on the host */
  const double t0 = wall_seconds();
  struct csr view = {s->n, 0, (unsigned *)offs, (unsigned *)cols, (double *)vals};
  struct lsb_amg_hier *h = lsb_amg_setup(&view, o->amg_theta, coarse, maxlev);
  if (!h)
    errx(EXIT_FAILURE, "hip_cdna4: cannot build the AMG hierarchy");
  struct amg_dev *a = lsb_calloc(struct amg_dev, 1);
  a->nlev = h->nlev, a->nc = h->nc, a->prec = o->amg_precision, a->cheb = cheb, a->mcgs = mcgs;
  if (mcgs) { /* the cap on a level's colours: LSBENCH_HIP_AMG_MCGS_COLOURS, 1 .. 64, is the A/B switch */
    const char *e = getenv("LSBENCH_HIP_AMG_MCGS_COLOURS");
    a->mcgs_cap = e && atoi(e) >= 1 && atoi(e) <= 64 ? (unsigned)atoi(e) : LSB_AMG_MCGS_COLOURS;
  }
  a->nu = o->amg_sweeps < 1 ? 1u : (o->amg_sweeps > 16 ? 16u : (unsigned)o->amg_sweeps);
  a->mem = lsb_calloc(void *, 18 * (size_t)h->nlev + 4);
  a->lv = lsb_calloc(struct amg_lv, h->nlev);
  a->vec = lsb_calloc(struct amg_vecs, h->nlev);
  /* the one-launch tail begins at the first level of at most amg_tail_rows rows (none under Chebyshev, multicolour
   * Gauss-Seidel or fp32) */
  for (a->tail = 0; a->tail < h->nlev; a->tail++)
    if (!cheb && !mcgs && !f32 && o->amg_tail_rows > 0 && h->lv[a->tail].n <= (unsigned)o->amg_tail_rows)
      break;
  /* per level: minv, the Chebyshev data, the upload in the solver's precision, what a cycle streams of it */
  for (unsigned l = 0; l < h->nlev; l++) {
    const struct lsb_amg_level *H = &h->lv[l];
    struct amg_lv *L = &a->lv[l];
    L->n = H->n;
    unsigned long long m0 = 0;
    unsigned n0 = 0;
    const int gs = mcgs && H->P && amg_upload_mcgs(a, l, H, &m0, &n0); /* else this level keeps l1-Jacobi */
    double *minv = (double *)malloc((size_t)(H->n ? H->n : 1) * sizeof(double));
    for (unsigned i = 0; i < H->n; i++) { /* 1 / sum_j |a_ij| (l1-Jacobi), 1 / a_ii (Chebyshev, Gauss-Seidel) */
      double sum = 0.0;
      for (unsigned e = H->A->offs[i]; e < H->A->offs[i + 1]; e++)
        sum += cheb || gs ? (H->A->cols[e] == i ? H->A->vals[e] : 0.0) : fabs(H->A->vals[e]);
      minv[i] = 1.0 / sum; /* > 0: lsb_amg_setup refused a diagonal <= 0 */
    }
    if (cheb && H->P) { /* the polynomial of degree nu on [rho / ratio, rho], rho the level's Gershgorin bound */
      L->hi = lsb_amg_gershgorin(H->A), L->lo = L->hi / ratio;
      lsb_amg_cheb_coeffs(L->hi, ratio, a->nu, L->c1, L->c2);
    }
    if (f32)
      amg_upload_level32(a, l, H, minv);
    else
      amg_upload_level(a, l, H, minv);
    LSB_CHK_HIP(hipStreamSynchronize(g_stream));
    free(minv);
    if (gs) { /* lsbench_hip.h, at lsb_hip_solver_amg_cycle_bytes: the copy 2 nu times less colour 0 once, A once */
      a->cycle_mat_bytes += 12ull * ((2ull * a->nu + 1ull) * H->A->offs[H->n] - m0 + H->P->offs[H->P->nrows] +
                                     H->R->offs[H->R->nrows]);
      a->cycle_vec_rows += (8ull * a->nu + 7ull) * H->n - 2ull * n0;
    } else if (H->P) { /* A goes 2 nu times (nu - 1 sweeps, the residual, nu sweeps), P and R once; 6 nu + 5 passes */
      a->cycle_mat_bytes += 12ull * (2ull * a->nu * H->A->offs[H->n] + H->P->offs[H->P->nrows] + H->R->offs[H->R->nrows]);
      a->cycle_vec_rows += (6ull * a->nu + 5ull) * H->n;
      if (cheb) /* d: written by both step 0s, read and written by the 2 (nu - 1) other steps */
        a->cycle_vec_rows += (4ull * a->nu - 2ull) * H->n;
    }
  }
  a->cycle_mat_bytes += 8ull * h->nc * h->nc;
  a->cycle_vec_rows += 2ull * h->nc;
  if (f32) {
    unsigned long long mat, vec;
    amg_cycle_bytes_split(a, &mat, &vec);
    a->cycle_bytes32 = mat + vec;
  }
  if (f32)
    a->d_cinv = amg_upload_f32(a, h->coarse_inv, (size_t)h->nc * h->nc, "the coarse inverse");
  else
    a->d_cinv = amg_keep(a, dev_upload(h->coarse_inv, (size_t)h->nc * h->nc * sizeof(double)));
  a->clanes = row_lanes(h->nc);
  LSB_CHK_HIP(hipStreamSynchronize(g_stream));
  a->setup_s = wall_seconds() - t0;
  if (o->verbose)
    amg_report(a, h, ratio);
  lsb_amg_free(h);
  s->amg = a;
}

/* level 0's two vectors out of the vector slab; under fp64 the levels as k_amg_tail reads them to the device */
void amg_finish_setup(struct shard *s) {
  struct amg_dev *a = s->amg;
  struct amg_vecs *v = &a->vec[0];
  double *t = shard_vec(s, s->n), *r = shard_vec(s, s->n);
  LSB_CHK_HIP(hipMemsetAsync(t, 0, (size_t)s->n * sizeof(double), g_stream));
  LSB_CHK_HIP(hipMemsetAsync(r, 0, (size_t)s->n * sizeof(double), g_stream));
  struct lsb_amg_lvdev *lv = NULL;
  if (a->prec == LSB_AMG_PREC_FP32) { /* in halves: two ping-pong iterates; the copy of the caller's r, the residual */
    v->tmp = t, v->out = (float *)t + s->n;
    v->b = r, v->r = (float *)r + s->n;
  } else { /* the second smoothing buffer and the residual; b and out are the caller's r and z */
    v->tmp = t, v->r = r;
    lv = lsb_calloc(struct lsb_amg_lvdev, a->nlev);
    for (unsigned l = 0; l < a->nlev; l++) {
      const struct amg_lv *L = &a->lv[l];
      lv[l].n = L->n, lv[l].A = L->A.d, lv[l].P = L->P.d, lv[l].R = L->R.d, lv[l].minv = (const double *)L->minv;
      lv[l].b = a->vec[l].b, lv[l].out = a->vec[l].out, lv[l].tmp = a->vec[l].tmp, lv[l].r = a->vec[l].r;
    }
    a->d_lv = (struct lsb_amg_lvdev *)amg_keep(a, dev_upload(lv, (size_t)a->nlev * sizeof *lv));
  }
  LSB_CHK_HIP(hipStreamSynchronize(g_stream));
  free(lv);
}

void amg_free(struct shard *s) {
  struct amg_dev *a = s->amg;
  if (!a)
    return;
  for (unsigned k = 0; k < a->nmem; k++)
    lsb_hip_free(a->mem[k]);
  /* level 0's two slab vectors (amg_finish_setup) */
  shard_vec_free(s, a->vec[0].tmp), shard_vec_free(s, a->prec == LSB_AMG_PREC_FP32 ? a->vec[0].b : a->vec[0].r);
  for (unsigned l = 0; l < a->nlev; l++)
    free(a->lv[l].cbeg);
  free(a->mem), free(a->lv), free(a->vec), free(a);
  s->amg = NULL;
}

char *amg_block_vecs(const struct amg_dev *a, unsigned kp, struct amg_vecs *v) {
#define BLOCK_BYTES(l, cnt) (((cnt) * (size_t)a->lv[l].n * kp * sizeof(double) + 255) & ~(size_t)255)
  const size_t blk = BLOCK_BYTES(0, 1);
  size_t total = 3 * blk;
  for (unsigned l = 1; l < a->nlev; l++)
    total += BLOCK_BYTES(l, 4);
  for (unsigned l = 0; a->cheb && l + 1 < a->nlev; l++)
    total += BLOCK_BYTES(l, 1);
  char *base = (char *)lsb_hip_malloc(total), *p = base + 3 * blk;
  LSB_CHK_HIP(hipMemsetAsync(base, 0, total, g_stream));
  v[0].tmp = base + blk, v[0].r = base + 2 * blk;
  for (unsigned l = 1; l < a->nlev; p += BLOCK_BYTES(l, 4), l++) {
    const size_t nl = (size_t)a->lv[l].n * kp * sizeof(double);
    v[l].b = p, v[l].out = p + nl, v[l].tmp = p + 2 * nl, v[l].r = p + 3 * nl;
  }
  /* the Chebyshev smoother's direction blocks, behind everything an l1 solver has */
  for (unsigned l = 0; a->cheb && l + 1 < a->nlev; p += BLOCK_BYTES(l, 1), l++)
    v[l].d = p;
#undef BLOCK_BYTES
  return base;
}

/* its counterpart for the fp32 cycle on blocks (hip_amg_f32_m.hip): Z, an fp64 block, then four blocks of interleaved
 * floats per level -- the fine level too, whose b is the float copy of the caller's R.  No direction blocks: the
 * Chebyshev smoother is not built there */
char *amg_block_vecs32(const struct amg_dev *a, unsigned kp, struct amg_vecs *v) {
#define BLOCK_BYTES(l, cnt, elem) (((cnt) * (size_t)a->lv[l].n * kp * (elem) + 255) & ~(size_t)255)
  const size_t zb = BLOCK_BYTES(0, 1, sizeof(double));
  size_t total = zb;
  for (unsigned l = 0; l < a->nlev; l++)
    total += 4 * BLOCK_BYTES(l, 1, sizeof(float));
  char *base = (char *)lsb_hip_malloc(total), *p = base + zb;
  LSB_CHK_HIP(hipMemsetAsync(base, 0, total, g_stream));
  for (unsigned l = 0; l < a->nlev; l++) {
    const size_t nl = BLOCK_BYTES(l, 1, sizeof(float));
    v[l].b = p, v[l].out = p + nl, v[l].tmp = p + 2 * nl, v[l].r = p + 3 * nl;
    p += 4 * nl;
  }
#undef BLOCK_BYTES
  return base;
}

/* ---- the V-cycle ------------
 * amg_cycle is the only place that knows the step order and the ping-pong parity.  The helpers above it pick the
 * launcher of the run's flavour, and each holds what is particular to a flavour at its step:
 *   AMG_F64  one column in fp64 (hip_amg.hip)
 *   AMG_F32  one column in fp32 (hip_amg_f32.hip): float vectors between the caller's fp64 r and z
 *   AMG_BLK  kp interleaved columns in fp64 (hip_mrhs_amg.hip, hip_amg_cheb.hip): each column with AMG_F64's bits
 *   AMG_BLK32  kp interleaved columns in fp32 (hip_amg_f32_m.hip; l1-Jacobi only): each column with AMG_F32's bits,
 *            float blocks between the fp64 blocks R and Z
 * Under the Chebyshev smoother the smoothing steps are the polynomial's: the same count and parity, d in place.
 * A level smoothed by multicolour Gauss-Seidel (lv[l].ncol > 0; one column only) is the other case: its
 * iterate stays in ONE buffer, the level's out, and a step is a sweep of ncol launches in place (hip_amg_mcgs.hip). */
enum amg_flavour { AMG_F64, AMG_F32, AMG_BLK, AMG_BLK32 };

static enum amg_flavour amg_flavour(const struct amg_run *c) {
  const int f32 = c->a->prec == LSB_AMG_PREC_FP32;
  return c->kp ? (f32 ? AMG_BLK32 : AMG_BLK) : f32 ? AMG_F32 : AMG_F64;
}

/* level l's vectors; under fp64 level 0's b and out are the caller's r and z */
static struct amg_vecs amg_vecs_at(const struct amg_run *c, unsigned l) {
  struct amg_vecs v = c->vec[l];
  if (l == 0 && c->a->prec != LSB_AMG_PREC_FP32)
    v.b = (void *)c->r, v.out = c->z;
  return v;
}

/* Smoothing step k of level l, out of place: y from x; x == NULL: step 0 of the way down, from the zero guess.
 * fp32: the fine level's step from the zero guess reads the caller's fp64 r (in64), rounds it once and leaves the
 * float copy in v->b, which every later step of the level reads.  last: the level's last step of the cycle, which on
 * the fine level writes the caller's z -- fp32 stores it there widened (y64) in the place of y, blocks leave the
 * records. */
static void amg_smooth(const struct amg_run *c, unsigned l, const struct amg_vecs *v, unsigned k, const void *x,
                       void *y, int last) {
  const struct amg_lv *L = &c->a->lv[l];
  const int cheb = c->a->cheb, z = last && l == 0;
  const double c1 = L->c1[k], c2 = L->c2[k];
  double *y64 = z ? c->z : NULL, *rec = z ? c->records : NULL;
  unsigned *nrec = z ? c->nrecords : NULL;
  switch (amg_flavour(c)) {
  case AMG_F64:
    if (!x && cheb)
      lsb_k_amg_cheb_first(L->n, v->b, L->minv, c2, v->d, y, c->st, g_stream);
    else if (!x)
      lsb_k_amg_first(L->n, v->b, L->minv, y, c->st, g_stream);
    else if (cheb)
      lsb_k_amg_cheb(&L->A.d, x, v->b, L->minv, c1, c2, v->d, y, c->st, g_stream);
    else
      lsb_k_amg_csr(LSB_AMG_SWEEP, &L->A.d, x, v->b, L->minv, y, c->st, g_stream);
    break;
  case AMG_F32:
    if (!x && cheb)
      lsb_k_amg32_cheb_first(L->n, l == 0, l ? v->b : c->r, L->minv, (float)c2, v->d, y, v->b, c->st, g_stream);
    else if (!x)
      lsb_k_amg32_first(L->n, l == 0, l ? v->b : c->r, L->minv, y, v->b, c->st, g_stream);
    else if (cheb)
      lsb_k_amg32_cheb(&L->A.f, x, v->b, L->minv, (float)c1, (float)c2, v->d, y, y64, c->st, g_stream);
    else
      lsb_k_amg32_csr(LSB_AMG_SWEEP, &L->A.f, x, v->b, L->minv, y, y64, c->st, g_stream);
    break;
  case AMG_BLK:
    if (!x && cheb)
      lsb_k_amg_cheb_first_m(c->kp, L->n, v->b, L->minv, c2, v->d, y, c->mst, g_stream);
    else if (!x)
      lsb_k_amg_first_m(c->kp, L->n, v->b, L->minv, y, c->mst, g_stream);
    else if (cheb)
      lsb_k_amg_cheb_m(c->kp, &L->A.d, x, v->b, L->minv, c1, c2, v->d, y, rec, nrec, c->mst, g_stream);
    else
      lsb_k_amg_csr_m(c->kp, LSB_AMG_SWEEP, &L->A.d, x, v->b, L->minv, y, rec, nrec, c->mst, g_stream);
    break;
  case AMG_BLK32: /* (l1-Jacobi, no records: amg_cycle has checked) */
    if (!x)
      lsb_k_amg32_first_m(c->kp, L->n, l == 0, l ? v->b : c->r, L->minv, y, v->b, c->mst, g_stream);
    else
      lsb_k_amg32_csr_m(c->kp, LSB_AMG_SWEEP, &L->A.f, x, v->b, L->minv, y, y64, c->mst, g_stream);
    break;
  }
}

/* The first launch of a multicolour Gauss-Seidel level's way down, from the zero guess, over all rows of v->out:
 * colour 0 gets dinv b, the other colours 0.  fp32: in64 and the float copy of r as in amg_smooth */
static void amg_mcgs_first(const struct amg_run *c, unsigned l, const struct amg_vecs *v) {
  const struct amg_lv *L = &c->a->lv[l];
  if (amg_flavour(c) == AMG_F64)
    lsb_k_amg_mcgs_first(L->n, L->colour8, v->b, L->minv, v->out, c->st, g_stream);
  else
    lsb_k_amg32_mcgs_first(L->n, l == 0, L->colour8, l ? v->b : c->r, L->minv, v->out, v->b, c->st, g_stream);
}

/* One sweep in place on v->out, a launch per colour: forward over the colours from .. ncol - 1, or backward over
 * ncol - 1 .. 0.  last: the level's last sweep of the cycle, which on the fine level of the fp32 cycle also stores
 * every row widened to the caller's z (under fp64 out IS z) */
static void amg_mcgs_sweep(const struct amg_run *c, unsigned l, const struct amg_vecs *v, int backward, unsigned from,
                           int last) {
  const struct amg_lv *L = &c->a->lv[l];
  for (unsigned k = from; k < L->ncol; k++) {
    const unsigned col = backward ? L->ncol - 1 - k : k, p0 = L->cbeg[col], p1 = L->cbeg[col + 1];
    if (amg_flavour(c) == AMG_F64)
      lsb_k_amg_mcgs(&L->C.d, L->rowid, p0, p1, v->out, v->b, L->minv, c->st, g_stream);
    else
      lsb_k_amg32_mcgs(&L->C.f, L->rowid, p0, p1, v->out, v->b, L->minv, last && l == 0 ? c->z : NULL, c->st,
                       g_stream);
  }
}

/* the steps that are one row kernel whatever the smoother -- residual, restriction, prolongation: y = mode(m; x, b) */
static void amg_csr(const struct amg_run *c, int mode, const union amg_mat *m, const void *x, const void *b,
                    const void *minv, void *y) {
  switch (amg_flavour(c)) {
  case AMG_F64: lsb_k_amg_csr(mode, &m->d, x, b, minv, y, c->st, g_stream); break;
  case AMG_F32: lsb_k_amg32_csr(mode, &m->f, x, b, minv, y, NULL, c->st, g_stream); break;
  case AMG_BLK: lsb_k_amg_csr_m(c->kp, mode, &m->d, x, b, minv, y, NULL, NULL, c->mst, g_stream); break;
  case AMG_BLK32: lsb_k_amg32_csr_m(c->kp, mode, &m->f, x, b, minv, y, NULL, c->mst, g_stream); break;
  }
}

/* the coarsest level l: out = the dense inverse times b.  l == 0, a hierarchy of one level: fp32 goes from the
 * caller's fp64 r to its fp64 z (ends64); blocks have no sweep to leave the records and form them here */
static void amg_coarse(const struct amg_run *c, unsigned l) {
  const struct amg_dev *a = c->a;
  const struct amg_vecs v = amg_vecs_at(c, l);
  switch (amg_flavour(c)) {
  case AMG_F64: lsb_k_amg_dense(a->nc, a->clanes, a->d_cinv, v.b, v.out, c->st, g_stream); break;
  case AMG_F32:
    if (l)
      lsb_k_amg32_dense(a->nc, a->clanes, 0, a->d_cinv, v.b, v.out, c->st, g_stream);
    else
      lsb_k_amg32_dense(a->nc, a->clanes, 1, a->d_cinv, c->r, c->z, c->st, g_stream);
    break;
  case AMG_BLK:
    lsb_k_amg_dense_m(c->kp, a->nc, a->clanes, a->d_cinv, v.b, v.out, c->mst, g_stream);
    if (l == 0 && c->records)
      lsb_k_amg_dot2_m(c->kp, a->lv[0].n, c->r, c->z, c->records, c->nrecords, c->mst, g_stream);
    break;
  case AMG_BLK32:
    if (l)
      lsb_k_amg32_dense_m(c->kp, a->nc, a->clanes, 0, a->d_cinv, v.b, v.out, c->mst, g_stream);
    else
      lsb_k_amg32_dense_m(c->kp, a->nc, a->clanes, 1, a->d_cinv, c->r, c->z, c->mst, g_stream);
    break;
  }
}

/* One V-cycle.  A level's iterate ping-pongs between buf[0] = tmp and buf[1] = out, every smoothing step going from
 * buf[at] to the other.  Down: step 0 from the zero guess into tmp, nu - 1 steps, the residual, the restriction.  Up:
 * the prolongation added to the iterate where the way down left it, buf[(nu - 1) % 2], then nu steps -- 2 nu - 1
 * out-of-place steps per level in all, so the last one writes out.  One column in fp64 under l1-Jacobi stops the walk
 * at a->tail and runs the levels from there in one launch (lsb_k_amg_tail: the same bits); every other flavour takes a
 * launch per step.  A multicolour Gauss-Seidel level has no parity: in place on out, down the first launch from zero,
 * the colours 1 .. of the first forward sweep and nu - 1 forward sweeps, up nu backward sweeps, ncol launches each.
 * Allocates nothing and synchronises nothing: it may run inside a stream capture. */
void amg_cycle(const struct amg_run *c) {
  const struct amg_dev *a = c->a;
  const unsigned nu = a->nu;
  if (a->mcgs && c->kp)
    errx(EXIT_FAILURE, "hip_cdna4: cannot happen: a V-cycle on blocks of columns under --amg-smoother mcgs");
  if (amg_flavour(c) == AMG_BLK32 && (a->cheb || c->records))
    errx(EXIT_FAILURE, "hip_cdna4: cannot happen: the fp32 V-cycle on blocks of columns %s",
         a->cheb ? "under --amg-smoother cheb" : "asked for records");
  const int tail = amg_flavour(c) == AMG_F64 && a->tail < a->nlev;
  const unsigned top = tail ? a->tail : a->nlev - 1;
  for (unsigned l = 0; l < top; l++) {
    const struct amg_vecs v = amg_vecs_at(c, l);
    void *const buf[2] = {v.tmp, v.out};
    unsigned at = 0;
    if (a->lv[l].ncol) { /* in place: the iterate is out */
      at = 1;
      amg_mcgs_first(c, l, &v);
      for (unsigned k = 0; k < nu; k++)
        amg_mcgs_sweep(c, l, &v, 0, k == 0, 0);
    } else {
      amg_smooth(c, l, &v, 0, NULL, buf[0], 0);
      for (unsigned k = 1; k < nu; k++, at ^= 1)
        amg_smooth(c, l, &v, k, buf[at], buf[at ^ 1], 0);
    }
    amg_csr(c, LSB_AMG_RESID, &a->lv[l].A, buf[at], v.b, a->lv[l].minv, v.r); /* r = b - A x */
    amg_csr(c, LSB_AMG_SPMV, &a->lv[l].R, v.r, NULL, NULL, c->vec[l + 1].b);  /* the next level's b = R r */
  }
  if (tail)
    lsb_k_amg_tail(a->d_lv, a->tail, a->nlev, nu, a->d_cinv, a->nc, a->clanes, c->r, c->z, c->st, g_stream);
  else
    amg_coarse(c, top);
  for (unsigned l = top; l-- > 0;) {
    const struct amg_vecs v = amg_vecs_at(c, l);
    void *const buf[2] = {v.tmp, v.out};
    unsigned at = a->lv[l].ncol ? 1 : (nu - 1) % 2;
    amg_csr(c, LSB_AMG_ADDP, &a->lv[l].P, c->vec[l + 1].out, NULL, NULL, buf[at]); /* x += P e */
    if (a->lv[l].ncol) {
      for (unsigned k = 0; k < nu; k++)
        amg_mcgs_sweep(c, l, &v, 1, 0, k + 1 == nu);
    } else {
      for (unsigned k = 0; k < nu; k++, at ^= 1)
        amg_smooth(c, l, &v, k, buf[at], buf[at ^ 1], k + 1 == nu);
    }
  }
}

/* ---- what the C-ABI answers about the hierarchy ------------ */
static const struct amg_dev *amg_of(const lsb_hip_solver *sv) {
  return sv && sv->o.precond == LSB_PRECOND_AMG ? sv->sh[0].amg : NULL;
}

int lsb_hip_solver_amg_info(lsb_hip_solver *sv, unsigned *levels, unsigned *tail_levels) {
  if (!lsb_initialized)
    return 1;
  const struct amg_dev *a = amg_of(sv);
  if (!a)
    return 2;
  if (levels)
    *levels = a->nlev;
  if (tail_levels)
    *tail_levels = a->nlev - a->tail;
  return 0;
}

int lsb_hip_solver_amg_precision(lsb_hip_solver *sv) {
  return amg_of(sv) ? amg_of(sv)->prec : 2;
}

unsigned long long lsb_hip_solver_amg_cycle_bytes(const lsb_hip_solver *sv) {
  const struct amg_dev *a = amg_of(sv);
  if (!a)
    return 0;
  return a->prec == LSB_AMG_PREC_FP32 ? a->cycle_bytes32 : a->cycle_mat_bytes + 8ull * a->cycle_vec_rows;
}

int lsb_hip_solver_amg_colours(lsb_hip_solver *sv, unsigned level, unsigned *ncolours) {
  if (!lsb_initialized)
    return 1;
  const struct amg_dev *a = amg_of(sv);
  if (!a || !a->mcgs || level + 1 >= a->nlev)
    return 2;
  if (ncolours)
    *ncolours = a->lv[level].ncol;
  return 0;
}

int lsb_hip_solver_amg_cheb_interval(lsb_hip_solver *sv, unsigned level, double *lo, double *hi) {
  if (!lsb_initialized)
    return 1;
  const struct amg_dev *a = amg_of(sv);
  if (!a || !a->cheb || level + 1 >= a->nlev)
    return 2;
  if (lo)
    *lo = a->lv[level].lo;
  if (hi)
    *hi = a->lv[level].hi;
  return 0;
}
