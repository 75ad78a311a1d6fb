/* Interleaved blocks of right-hand sides: what their drivers -- independent recurrences (hip_mrhs_drv.c), block-CG
 * (hip_bcg_drv.c), the direct solver (hip_direct_m_drv.c) and AMG as the solver (hip_rich_m_drv.c) -- share on the
 * host.  The contracts (what is served, the gates, verify) are the drivers'. */
#define _GNU_SOURCE
#include "hip_solver.h"

/* ---- the service rules --------------------------------------------------------------------------------------------
 * One shard in one process, fp64 values, krylov PCG or AUTO, precond JACOBI / L1JACOBI / NONE / AMG in fp64, and FSAI
 * where opts.fsai_blocks is set; every other solver answers 2.  An AMG solver smoothed by multicolour Gauss-Seidel has
 * its SpMM served and nothing else: its cycle is not built on blocks. */
static int block_mcgs(const lsb_hip_solver *sv) {
  return sv->o.precond == LSB_PRECOND_AMG && sv->sh[0].amg && sv->sh[0].amg->mcgs;
}

int block_spmm_serves(const lsb_hip_solver *sv) {
  const struct lsb_hip_opts *o = &sv->o;
  return !sv->multi && sv->nshard == 1 && !sv->dist && o->precision == LSB_PREC_FP64 &&
         (o->krylov == LSB_KRYLOV_PCG || o->krylov == LSB_KRYLOV_AUTO) &&
         (o->precond == LSB_PRECOND_JACOBI || o->precond == LSB_PRECOND_L1JACOBI ||
          o->precond == LSB_PRECOND_NONE ||
          (o->precond == LSB_PRECOND_AMG && sv->sh[0].amg && sv->sh[0].amg->prec == LSB_AMG_PREC_FP64) ||
          (o->precond == LSB_PRECOND_FSAI && o->fsai_blocks && sv->sh[0].fs_g.offs && sv->sh[0].fs_gt.offs)) &&
         o->persistent <= 0 && !sv->ps.use && (unsigned long long)sv->sh[0].n * LSB_MRHS_MAX < (1ull << 32);
}

int block_serves(const lsb_hip_solver *sv) { return block_spmm_serves(sv) && !block_mcgs(sv); }

int block_fsai(const lsb_hip_solver *sv) { return sv->o.precond == LSB_PRECOND_FSAI; }

int block_zblock(const lsb_hip_solver *sv) { return sv->o.precond == LSB_PRECOND_AMG || block_fsai(sv); }

unsigned block_width(unsigned nrhs) { return nrhs <= 2 ? 2u : nrhs <= 4 ? 4u : 8u; }

int block_args_bad(const lsb_hip_solver *sv, unsigned nrhs, unsigned max_nrhs, const void *a, size_t lda,
                   const void *b, size_t ldb) {
  return !sv || !a || !b || nrhs == 0 || (max_nrhs && nrhs > max_nrhs) || lda < sv->n_user || ldb < sv->n_user;
}

/* ---- lanes per row ------------------------------------------------------------------------------------------------ */
static void block_lanes_init(lsb_hip_solver *sv) {
  /* of the SpMM: the shard's (from its mean row length); LSBENCH_HIP_MRHS_LANES is the A/B switch */
  const char *e = getenv("LSBENCH_HIP_MRHS_LANES");
  sv->mr_lanes = e && atoi(e) > 0 ? (unsigned)atoi(e) : sv->sh[0].lanes;
  /* ... of G and of G^T under FSAI: each matrix's own; LSBENCH_HIP_MRHS_FSAI_LANES is the A/B switch for both (the
   * single-column kernels never see it) */
  e = getenv("LSBENCH_HIP_MRHS_FSAI_LANES");
  sv->mr_fs_lanes = e && atoi(e) > 0 ? (unsigned)atoi(e) : 0;
}

unsigned block_fsai_lanes(const lsb_hip_solver *sv, const struct fsai_csr *c) {
  return sv->mr_fs_lanes ? sv->mr_fs_lanes : c->lanes;
}

/* ---- the work area ------------------------------------------------------------------------------------------------ */
static size_t block_bytes(const lsb_hip_solver *sv, unsigned kp) {
  return (((size_t)sv->sh[0].n * kp * sizeof(double)) + 255) & ~(size_t)255;
}

/* 256-byte aligned pieces of one allocation, the blocks first and in this order: their placement relative to one
 * another is deliberate, the same in every solver and in both drivers */
char *block_work_slab(lsb_hip_solver *sv, struct block_work *w, unsigned kp, unsigned nblk, size_t behind) {
  if (!sv->mr_lanes) /* no driver has run a block on this solver yet */
    block_lanes_init(sv);
  const size_t blk = block_bytes(sv, kp);
  w->mem = (char *)lsb_hip_malloc(nblk * blk + behind);
  LSB_CHK_HIP(hipMemsetAsync(w->mem, 0, nblk * blk + behind, g_stream));
  w->b = (double *)w->mem, w->x = (double *)(w->mem + blk), w->r = (double *)(w->mem + 2 * blk);
  w->p = (double *)(w->mem + 3 * blk);
  if (nblk >= 5)
    w->q = (double *)(w->mem + 4 * blk);
  if (nblk == 7)
    w->z = (double *)(w->mem + 5 * blk), w->t = (double *)(w->mem + 6 * blk);
  w->kp = kp;
  return w->mem + nblk * blk;
}

char *block_work_z(lsb_hip_solver *sv, struct block_work *w, size_t behind) {
  if (block_fsai(sv)) {
    const size_t blk = block_bytes(sv, w->kp);
    w->zmem = (char *)lsb_hip_malloc(2 * blk + behind);
    LSB_CHK_HIP(hipMemsetAsync(w->zmem, 0, 2 * blk + behind, g_stream));
    w->z = (double *)w->zmem, w->t = (double *)(w->zmem + blk);
    return w->zmem + 2 * blk;
  }
  const struct amg_dev *a = sv->sh[0].amg;
  w->av = lsb_calloc(struct amg_vecs, a->nlev);
  w->amg_mem = a->prec == LSB_AMG_PREC_FP32 ? amg_block_vecs32(a, w->kp, w->av) : amg_block_vecs(a, w->kp, w->av);
  w->z = (double *)w->amg_mem;
  return NULL;
}

void block_work_free(struct block_work *w) {
  graph_drop(&w->g);
  lsb_hip_free(w->mem), lsb_hip_free(w->zmem), lsb_hip_free(w->amg_mem);
  free(w->av);
  memset(w, 0, sizeof *w);
}

/* ---- Z = M^-1 R ---------------------------------------------------------------------------------------------------- */
static void block_fsai_spmm(const lsb_hip_solver *sv, const struct block_work *w, const struct fsai_csr *c,
                            const double *x, double *y, double *rec) {
  unsigned np = 0;
  lsb_k_spmm_csr(w->kp, sv->sh[0].n, c->offs, c->cols, c->vals, block_fsai_lanes(sv, c), x, y, NULL, rec, &np, NULL,
                 g_stream);
}

void block_fsai_g(const lsb_hip_solver *sv, const struct block_work *w, const double *r, double *rec) {
  block_fsai_spmm(sv, w, &sv->sh[0].fs_g, r, w->t, rec);
}

void block_zapply(const lsb_hip_solver *sv, const struct block_work *w, const double *r, double *rec) {
  if (block_fsai(sv)) { /* two SpMMs off the factor's CSRs */
    block_fsai_g(sv, w, r, rec);
    block_fsai_spmm(sv, w, &sv->sh[0].fs_gt, w->t, w->z, rec);
    return;
  }
  const struct amg_run c = {.a = sv->sh[0].amg, .vec = w->av, .kp = w->kp, .r = r, .z = w->z,
                            .records = NULL, .nrecords = NULL, .mst = NULL};
  amg_cycle(&c);
}

/* ---- the wrappers ------------------------------------------------------------------------------------------------- */
void block_enqueue(void *block_enq, int iters) {
  const struct block_enq *e = block_enq;
  if (e->sv->o.use_graph)
    graph_launch(&e->w->g, iters, NULL, e->iters, e->ctx);
  else
    e->iters(e->ctx, iters);
}

int block_solve_host(block_dev_fn *dev, int x_always, lsb_hip_solver *sv, unsigned nrhs, const double *B, size_t ldb,
                     double *X, size_t ldx, struct lsb_hip_result *res) {
  const size_t n = sv->n_user, bytes = n * sizeof(double);
  double *d_B = (double *)lsb_hip_malloc(bytes * nrhs), *d_X = (double *)lsb_hip_malloc(bytes * nrhs);
  LSB_CHK_HIP(hipMemcpy2D(d_B, bytes, B, ldb * sizeof(double), bytes, nrhs, hipMemcpyHostToDevice));
  const int rc = dev(sv, nrhs, d_B, n, d_X, n, res);
  if (x_always || rc == 0)
    LSB_CHK_HIP(hipMemcpy2D(X, ldx * sizeof(double), d_X, bytes, bytes, nrhs, hipMemcpyDeviceToHost));
  lsb_hip_free(d_B), lsb_hip_free(d_X);
  return rc;
}
