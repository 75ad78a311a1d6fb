/*
 * Jacobi-PCG on the device-resident state: the iteration forms a solver may run (one is chosen at
 * creation, pcg_choose_form), what each enqueues per iteration, one run through the host loop the drivers share
 * (hip_run.c; DESIGN.md section 4, "Host loop"), and the driver's entry point pcg_solve_dev (hip_solve.c has the
 * solve around it).
 */
#define _GNU_SOURCE
#include "hip_solver.h"

/* ------------------------------------------------------------------------ */
/* PCG                                                                       */
/* ------------------------------------------------------------------------ */
/* Which PCG iteration the solver runs (enum pcg_form), tried in this order:
 *   FSAI3    FSAI on a launch-bound operator (S, G and G^T all sub-wavefront), one shard, fp64
 *   GENERIC  any other vector preconditioner (Chebyshev, block-Jacobi, FSAI, AMG)
 *   CG1      opts.krylov = cg1, or auto across shards
 *   COL      one shard, fp64, Jacobi with one constant diagonal, on the z-column plan
 *   SUBWAVE  one shard, fp64, the sub-wavefront SpMV
 *   CLASSIC  the rest
 * Called once, by solver_finish_setup: after precond_setup (FSAI3 looks at G and G^T), before the set-up
 * passes that run solves (p2p_setup, overlap_setup, persist_setup).  That is the choice each enqueued
 * iteration used to make again: of its inputs only opts.sample_spmv changes after creation -- overlap_setup
 * zeroes it for its timing solves, on multi-shard solvers only, where neither form that reads it (FSAI3,
 * SUBWAVE) can apply.  The switches that turn the fused forms off for the tests that compare them
 * (LSBENCH_HIP_NO_FSAI_FUSE, _NO_FUSE_P, _NO_FUSE_PX) are read here alone. */
enum pcg_form pcg_choose_form(const lsb_hip_solver *sv) {
  const struct shard *s = &sv->sh[0];
  const struct lsb_hip_opts *o = &sv->o;
  if (o->krylov == LSB_KRYLOV_GMRES || o->krylov == LSB_KRYLOV_BICGSTAB || o->krylov == LSB_KRYLOV_RICHARDSON ||
      o->krylov == LSB_KRYLOV_DIRECT)
    return PCG_NONE;
  if (o->precond == LSB_PRECOND_FSAI && !sv->multi && !s->mixed && s->variant == LSB_SPMV_SUBWAVE &&
      s->fs_g.variant == LSB_SPMV_SUBWAVE && s->fs_gt.variant == LSB_SPMV_SUBWAVE && o->sample_spmv <= 0 &&
      o->krylov != LSB_KRYLOV_PCG1 && !getenv("LSBENCH_HIP_NO_FSAI_FUSE"))
    return PCG_FSAI3;
  if (generic_precond(sv))
    return PCG_GENERIC;
  /* single reduction, measured on one GPU: no gain for small operators (tests/xn3b_A_18.txt: 390 vs
   * 400 solves/s, the fused sweep is as long as the two it replaces) and +6 % time
   * on the 10M-row operator where the diagonal is a vector (96 n vs 88 n bytes; round 3, general
   * values: 251 against 236-241 us per iteration); what it saves there is a collective.
   * With ONE constant diagonal (u = c r never stored) it moves the classic form's 72 n in two
   * launches instead of three; since its sweep loads the gather vector the plain way
   * (k_cg1_update, round 3: the SpMV behind it 40 -> 24 us on config 3) it is level with the
   * classic form on one GPU -- config 3 through bench.py 136.8-138.0 against 136.0-139.8 us per
   * iteration, config 4 1186-1188 against 1182-1191 (tools/gpu_krylov_ab.sh) -- so one shard
   * keeps the classic form, the reference's algorithm as written. */
  if (o->krylov == LSB_KRYLOV_PCG1 || (o->krylov == LSB_KRYLOV_AUTO && sv->multi))
    return PCG_CG1;
  if (sv->multi || s->mixed || getenv("LSBENCH_HIP_NO_FUSE_P"))
    return PCG_CLASSIC;
  if (s->sell_form == SELL_COL && s->dinv_uniform && s->c16.tmpl.nfar >= 1 && s->c16.tmpl.nfar <= 2 &&
      s->row_begin == 0 && s->n == s->n_glob && o->precond == LSB_PRECOND_JACOBI && !getenv("LSBENCH_HIP_NO_FUSE_PX"))
    return PCG_COL; /* (event-timed too: the sample brackets the launch that carries the SpMV) */
  /* (not while SpMV launches are being event-timed: the fused launch has no SpMV of its own to
   * bracket, and pcg_run reads the sample events) */
  return s->variant == LSB_SPMV_SUBWAVE && o->sample_spmv <= 0 ? PCG_SUBWAVE : PCG_CLASSIC;
}

/* The vectors a form needs besides the shard's own, out of its slab where they fit (shard_vec): the second
 * direction buffer of SUBWAVE, COL and FSAI3, FSAI3's second residual, CG1's p and s.  Where they land sets
 * the iteration's speed (tune_blas1_nt), so they are taken when they always were: FSAI's by precond_setup
 * for every FSAI solver, whichever form it runs (the slab counts them), the others by the first init -- but
 * for the second direction buffer of a shard that can run a fused-p form (one shard, fp64, Jacobi, classic
 * PCG): shard_upload counts it into the slab and carves it right behind the gather vector. */
void form_vecs(lsb_hip_solver *sv, enum pcg_form f) {
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    if (!s->d_p1 && (f == PCG_SUBWAVE || f == PCG_COL || f == PCG_CG1 || f == PCG_FSAI3))
      s->d_p1 = shard_vec(s, s->n);
    if (!s->d_s1 && f == PCG_CG1)
      s->d_s1 = shard_vec(s, s->n);
    if (!s->d_r1 && f == PCG_FSAI3)
      s->d_r1 = shard_vec(s, s->n);
  }
}

void sample_open(lsb_hip_solver *sv, int k) {
  if (k >= 0)
    LSB_CHK_HIP(hipEventRecord(sv->ev[4 * k], g_stream));
}

/* e1 closes the SpMV interval; e2,e3 bracket NOTHING: their distance is
 * what one event marker costs in this very spot of the stream, and is
 * subtracted from e0->e1 (an event pair around a kernel otherwise reads
 * ~9 us longer than the kernel's duration in a rocprofv3 trace). */
void sample_close(lsb_hip_solver *sv, int k) {
  for (int e = 1; e < 4 && k >= 0; e++)
    LSB_CHK_HIP(hipEventRecord(sv->ev[4 * k + e], g_stream));
}

/* q = S p and p.q on every shard: behind the exchange and through the all-reduce where there are several */
static void spmv_pq(lsb_hip_solver *sv, int sample) {
  if (sv->multi) {
    exchange_and_spmv(sv, sample);
    allreduce_pq(sv, 1, 0);
    return;
  }
  struct shard *s = &sv->sh[0];
  sample_open(sv, sample);
  spmv_shard(s, s->d_pfull, s->d_q, s->d_pfull + s->row_begin, s->d_parts_pq, &s->npq, s->d_st);
  sample_close(sv, sample);
}

/* the s->np2 partial sums of (r.z, r.r) in every shard's d_parts2, summed over the shards into d_scal[1..2]
 * where there are several; gated: on the state of the running solve */
static void reduce_rz(lsb_hip_solver *sv, int gated) {
  if (!sv->multi)
    return;
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    lsb_k_reduce_final(s->d_parts2, s->np2, 2, s->d_scal + 1, 0, gated ? s->d_st : NULL, g_stream);
  }
  allreduce_scal(sv, 1, 2, gated);
}

/* how every init ends: (r.z, r.r) starts the run's state (not gated: the device state still holds the
 * previous solve's status) */
static void init_state(lsb_hip_solver *sv) {
  reduce_rz(sv, 0);
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    lsb_k_pcg_init_state(s->d_st, sv->multi ? s->d_scal + 1 : s->d_parts2, sv->multi ? 1u : s->np2, sv->tol_run,
                         (int)sv->o.maxit, g_stream);
  }
}

/* ---- classic form, and the init of the two that fuse it (SUBWAVE, COL) ---- */
static void classic_enqueue_init(lsb_hip_solver *sv, const double *d_b, double *d_x) {
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    const size_t o = s->row_begin - sv->row_first;
    lsb_k_pcg_init(s->n, d_b + o, DINV(s), d_x + o, s->d_r, s->d_pfull + s->row_begin, s->d_parts2, &s->np2,
                   g_stream);
  }
  init_state(sv);
}

static void classic_enqueue_iter(lsb_hip_solver *sv, double *d_x, int parity, int sample) {
  spmv_pq(sv, sample);
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    const size_t o = s->row_begin - sv->row_first;
    lsb_k_pcg_update_xr(s->n, s->d_pfull + s->row_begin, s->d_q, DINV(s), d_x + o, s->d_r, s->d_st, parity,
                        sv->multi ? s->d_scal : s->d_parts_pq, sv->multi ? 1u : s->npq, s->d_parts2, &s->np2,
                        sv->nt_mask, g_stream);
  }
  reduce_rz(sv, 1);
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    lsb_k_pcg_update_p(s->n, s->d_r, DINV(s), s->d_pfull + s->row_begin, s->d_pfull + s->row_begin, s->d_st,
                       parity, sv->multi ? s->d_scal + 1 : s->d_parts2, sv->multi ? 1u : s->np2, sv->nt_mask, g_stream);
  }
}

/* ---- GENERIC: PCG with z = M^-1 r as a vector (Chebyshev, block-Jacobi, FSAI, AMG) -------------
 * The classic recurrences through the same sweeps: k_pcg_update_xr with a unit
 * "diagonal" (its own r.r partial sums are superseded), the preconditioner's
 * launches, k_dot2 for (r.z, r.r), k_pcg_update_p with z in the place of r. */
static void gen_enqueue_init(lsb_hip_solver *sv, const double *d_b, double *d_x) {
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    const size_t o = s->row_begin - sv->row_first;
    unsigned np2 = 0; /* (superseded by k_dot2's below) */
    /* x = 0, r = b (p = b for the moment) */
    lsb_k_pcg_init(s->n, d_b + o, NULL, 1.0, d_x + o, s->d_r, s->d_pfull + s->row_begin,
                   s->d_parts2, &np2, g_stream);
    /* the state of the previous solve must not gate the preconditioner below */
    LSB_CHK_HIP(hipMemsetAsync(&s->d_st->status, 0, sizeof(int), g_stream));
  }
  precond_apply(sv, 0); /* z = M^-1 b */
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    LSB_CHK_HIP(hipMemcpyAsync(s->d_pfull + s->row_begin, s->d_z, (size_t)s->n * sizeof(double),
                               hipMemcpyDeviceToDevice, g_stream)); /* p = z */
    lsb_k_dot2(s->n, s->d_r, s->d_z, s->d_parts2, &s->np2, NULL, g_stream); /* (b.z, b.b) */
  }
  init_state(sv);
}

static void gen_enqueue_iter(lsb_hip_solver *sv, double *d_x, int parity, int sample) {
  spmv_pq(sv, sample);
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    const size_t o = s->row_begin - sv->row_first;
    lsb_k_pcg_update_xr(s->n, s->d_pfull + s->row_begin, s->d_q, NULL, 1.0, d_x + o, s->d_r, s->d_st,
                        parity, sv->multi ? s->d_scal : s->d_parts_pq, sv->multi ? 1u : s->npq,
                        s->d_parts2, &s->np2, sv->nt_mask, g_stream);
  }
  precond_apply(sv, 1);
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    lsb_k_dot2(s->n, s->d_r, s->d_z, s->d_parts2, &s->np2, s->d_st, g_stream);
  }
  reduce_rz(sv, 1);
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    lsb_k_pcg_update_p(s->n, s->d_z, NULL, 1.0, s->d_pfull + s->row_begin, s->d_pfull + s->row_begin,
                       s->d_st, parity, sv->multi ? s->d_scal + 1 : s->d_parts2,
                       sv->multi ? 1u : s->np2, sv->nt_mask, g_stream);
  }
}

/* ---- FSAI3: FSAI-PCG of a launch-bound operator in three launches per iteration (hip_fsai.hip):
 *   A  beta, stop test, p = z + beta p in the gather of S's rows, q = S p, p.q   (k_spmv_subwave_p)
 *   B  alpha, x += alpha p, r' = r - alpha q in the gather of G's rows, t = G r'  (k_fsai_xr_gr)
 *   C  z = G^T t, partial sums of (r'.z, r'.r')                                   (k_fsai_gt_dots)
 * p and r alternate between two buffers each; the last iteration of an enqueued run closes
 * with the stand-alone direction sweep and leaves r in the shard's own residual vector.
 * (Its init is GENERIC's.) */
static void fsai_enqueue_iter(lsb_hip_solver *sv, double *d_x, int parity, int pos) {
  struct shard *s = &sv->sh[0];
  double *pb[2] = {s->d_pfull, s->d_p1}, *rb[2] = {s->d_r, s->d_r1};
  if (pos & 1) { /* first of the run: p is in the gather vector, r in d_r, (r.z, r.r) in the state */
    sv->pcur = 0, sv->rcur = 0;
    spmv_shard(s, pb[0], s->d_q, pb[0], s->d_parts_pq, &s->npq, s->d_st);
  } else {
    lsb_k_spmv_subwave_p(s->n, s->csr.offs, s->csr.cols, s->csr.vals, s->lanes, s->d_z, NULL, 1.0, pb[sv->pcur],
                         pb[sv->pcur ^ 1], s->d_q, s->d_parts_pq, &s->npq, s->d_st, parity ^ 1, s->d_parts2,
                         s->np2, g_stream);
    sv->pcur ^= 1;
  }
  lsb_k_fsai_xr_gr(s->n, s->fs_g.offs, s->fs_g.cols, s->fs_g.vals, s->fs_g.lanes, pb[sv->pcur], s->d_q, d_x,
                   rb[sv->rcur], rb[sv->rcur ^ 1], s->d_fst, s->d_st, parity, s->d_parts_pq, s->npq, g_stream);
  sv->rcur ^= 1;
  lsb_k_fsai_gt_dots(s->n, s->fs_gt.offs, s->fs_gt.cols, s->fs_gt.vals, s->fs_gt.lanes, s->d_fst, s->d_z,
                     rb[sv->rcur], s->d_parts2, &s->np2, s->d_st, g_stream);
  if (pos & 2) { /* last of the run */
    lsb_k_pcg_update_p(s->n, s->d_z, NULL, 1.0, pb[sv->pcur], pb[0], s->d_st, parity, s->d_parts2, s->np2,
                       sv->nt_mask, g_stream);
    if (sv->rcur)
      LSB_CHK_HIP(hipMemcpyAsync(s->d_r, s->d_r1, (size_t)s->n * sizeof(double), hipMemcpyDeviceToDevice,
                                 g_stream));
  }
}

/* ---- SUBWAVE: launch-bound operators (one shard, sub-wavefront SpMV, classic form) -------------
 * The direction update rides in the NEXT iteration's SpMV (k_spmv_subwave_p), two
 * launches per iteration; the two direction buffers alternate.  Only the last
 * iteration of an enqueued run closes with the stand-alone update, which also
 * brings the direction back into the gather vector.
 * The same fold was built for the slice-template form of a structured grid
 * (k_spmv_tmpl_p, round 3: the direction update's own pass over r and p disappears, 880 -> 800 MB
 * per iteration on the 10 M-row 5-point operator), measured -- 81.4 us where k_spmv_tmpl +
 * k_pcg_update_p take 40.4 + 40.4 (rocprofv3 means inside the solve, gpurun_out/r3_fuse3): no
 * gain, both SpMV-shaped launches run at 4.0 TB/s inside the solve -- and taken out again when
 * its 7-point instantiation turned out not to be repeatable run to run once the masked slots
 * came in (gpurun_out/r3_mask, tools/gpu_tmpl_diag3.py): DESIGN.md section 4. */
static void subwave_enqueue_iter(lsb_hip_solver *sv, double *d_x, int parity, int pos) {
  struct shard *s = &sv->sh[0];
  double *buf[2] = {s->d_pfull, s->d_p1};
  if (pos & 1) { /* first of the run: the direction is in the gather vector */
    sv->pcur = 0;
    spmv_shard(s, buf[0], s->d_q, buf[0], s->d_parts_pq, &s->npq, s->d_st);
  } else { /* beta, stop test and p = D^-1 r + beta p of the previous iteration, then S p */
    lsb_k_spmv_subwave_p(s->n, s->csr.offs, s->csr.cols, s->csr.vals, s->lanes, s->d_r, DINV(s),
                         buf[sv->pcur], buf[sv->pcur ^ 1], s->d_q, s->d_parts_pq, &s->npq, s->d_st,
                         parity ^ 1, s->d_parts2, s->np2, g_stream);
    sv->pcur ^= 1;
  }
  lsb_k_pcg_update_xr(s->n, buf[sv->pcur], s->d_q, DINV(s), d_x, s->d_r, s->d_st, parity,
                      s->d_parts_pq, s->npq, s->d_parts2, &s->np2, sv->nt_mask, g_stream);
  if (pos & 2) /* last of the run */
    lsb_k_pcg_update_p(s->n, s->d_r, DINV(s), buf[sv->pcur], buf[0], s->d_st, parity, s->d_parts2,
                       s->np2, sv->nt_mask, g_stream);
}

/* ---- COL: the z-column form of a 3-D stencil with a constant diagonal ----------------------------
 * [S p | p' = dc r + beta p, x += alpha p, p'.(S p')] then [r -= alpha S p']: direction update AND the x half
 * of the first sweep ride in the next SpMV launch, the r half forms S p again instead of reading a stored q,
 * x is updated every second iteration with two directions at once (k_pcg_col_px + k_pcg_col_r: 60 instead of
 * 88 bytes per row and iteration); the run's last pending x update is applied by k_pcg_xfix.  x goes in and
 * out as 16-byte vectors: pcg_run gives an x that is not 16-byte aligned to the classic form.
 * Sampling: the launch that carries the SpMV, bracketed as the classic form brackets a plain one; a run's
 * first iteration (a plain SpMV launch) is marked in samp_skip and left out by pcg_run -- the figure is
 * k_pcg_col_px's alone. */
static void col_enqueue_iter(lsb_hip_solver *sv, double *d_x, int parity, int pos, int sample) {
  struct shard *s = &sv->sh[0];
  double *buf[2] = {s->d_pfull, s->d_p1};
  if (sample >= 0)
    sv->samp_skip[sample] = (pos & 1) != 0;
  if (pos & 1) { /* first of the run: the direction is in the gather vector, x is up to date */
    sv->pcur = 0;
    spmv_shard(s, buf[0], s->d_q, buf[0], s->d_parts_pq, &s->npq, s->d_st);
  } else {
    sample_open(sv, sample);
    lsb_k_pcg_col_px(s->sp_grid, s->col.period, s->col.plan, s->col.items, s->n, &s->c16, s->d_r, buf[sv->pcur],
                     buf[sv->pcur ^ 1], d_x, /* x updated by the run's even iterations, two steps at once */ parity == 0,
                     s->dinv_const, s->d_parts_pq, &s->npq, s->d_st, parity ^ 1, s->d_parts2, s->np2, g_stream);
    sample_close(sv, sample);
    sv->pcur ^= 1;
  }
  /* r -= alpha S p with S p formed again out of p (k_pcg_col_r): q never travels.  Its turns run through each
   * XCD's band from the END (rev = 1): k_pcg_col_px and the z-column SpMV ascend, so every launch of the iteration
   * starts on the lines the one before touched last -- r and the two directions are 232 MB of a 256 MB Infinity
   * Cache on the 10 M-row grid, and with every launch ascending each line's reuse distance was a whole launch.
   * Always, not by a timing pass: the bits of (r.z, r.r) follow the order */
  lsb_k_pcg_col_r(s->sp_grid, s->col.period, s->col.plan, s->col.items, s->n, &s->c16, buf[sv->pcur], s->d_r,
                  s->dinv_const, s->d_st,
                  parity, sv->pcur, /* x is two updates behind after an odd iteration */ parity != 0, /* rev */ 1,
                  s->d_parts_pq, s->npq, s->d_parts2, &s->np2, g_stream);
  if (pos & 2) { /* last of the run: the pending x update, then the direction back into the gather vector */
    lsb_k_pcg_xfix(s->n, buf[0], buf[1], d_x, s->d_st, g_stream);
    lsb_k_pcg_update_p(s->n, s->d_r, DINV(s), buf[sv->pcur], buf[0], s->d_st, parity, s->d_parts2, s->np2,
                       sv->nt_mask, g_stream);
  }
}

/* ---- CG1: single-reduction CG (LSB_KRYLOV_PCG1), see k_cg1_update -------------- */
static void cg1_enqueue_init(lsb_hip_solver *sv, const double *d_b, double *d_x) {
  sv->ar_fold = can_fold_allreduce(sv), sv->ar_pending = 0, sv->fold_next = 0;
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    const size_t o = s->row_begin - sv->row_first, bytes = (size_t)s->n * sizeof(double);
    /* x = 0, r = b, u = D^-1 b (into the gather vector), partials (r.u, b.b);
     * implicit u (constant diagonal): r itself goes into the gather vector and
     * u = c b lands in a scratch nobody reads */
    if (sv->cg1_implicit)
      lsb_k_pcg_init(s->n, d_b + o, DINV(s), d_x + o, s->d_pfull + s->row_begin, s->d_r,
                     s->d_parts2, &s->np2, g_stream);
    else
      lsb_k_pcg_init(s->n, d_b + o, DINV(s), d_x + o, s->d_r, s->d_pfull + s->row_begin,
                     s->d_parts2, &s->np2, g_stream);
    LSB_CHK_HIP(hipMemsetAsync(s->d_p1, 0, bytes, g_stream));
    LSB_CHK_HIP(hipMemsetAsync(s->d_s1, 0, bytes, g_stream));
  }
  init_state(sv);
  spmv_pq(sv, -1); /* w = S u, partials w.u */
}

static void cg1_enqueue_iter(lsb_hip_solver *sv, double *d_x, int parity, int sample) {
  for (int i = 0; i < sv->nshard; i++) {
    struct shard *s = &sv->sh[i];
    const size_t o = s->row_begin - sv->row_first;
    double *gr_in = s->d_parts2 + (size_t)parity * 2 * LSB_MAX_PARTIALS;
    double *gr_out = s->d_parts2 + (size_t)(parity ^ 1) * 2 * LSB_MAX_PARTIALS;
    unsigned np2 = 0;
    struct lsb_ar_collect col;
    if (sv->ar_pending) /* the SpMV before this launch sent the sums to every rank's mailbox */
      lsb_p2p_fold_collect(sv->p2p[i], &col);
    lsb_k_cg1_update(s->n, sv->cg1_implicit ? NULL : s->d_pfull + s->row_begin, s->d_q, DINV(s),
                     s->d_p1, s->d_s1, d_x + o,
                     sv->cg1_implicit ? s->d_pfull + s->row_begin : s->d_r, s->d_st, parity,
                     sv->multi ? s->d_scal + 1 : gr_in,
                     sv->multi ? 1u : s->np2, sv->multi ? s->d_scal : s->d_parts_pq,
                     sv->multi ? 1u : s->npq, sv->ar_pending ? &col : NULL, gr_out, &np2, sv->nt_mask, g_stream);
    /* reduced together with the SpMV's partial sums, in the all-reduce's launch
     * (direct path) or in the one reduction launch in front of it (RCCL) */
    s->ar2_parts = gr_out, s->ar2_n = np2, s->ar2_width = 2;
  }
  if (sv->multi) {
    sv->fold_next = sv->ar_fold == 2;
    exchange_and_spmv(sv, sample);
  } else {
    struct shard *s = &sv->sh[0];
    sample_open(sv, sample);
    spmv_shard(s, s->d_pfull, s->d_q, s->d_pfull + s->row_begin, s->d_parts_pq, &s->npq, s->d_st);
    sample_close(sv, sample);
  }
  /* w.u, r.u, r.r in ONE collective -- over the direct path sent by a launch that waits
   * for nobody (or by the SpMV's last workgroup) and collected by the next k_cg1_update */
  if (sv->multi && sv->ar_fold) {
    if (sv->ar_fold == 1)
      allreduce_pq_contribute(sv);
    sv->ar_pending = 1;
  } else if (sv->multi)
    allreduce_pq(sv, 3, 1);
}

/* ---- one dispatch ---- */
static void pcg_enqueue_init(lsb_hip_solver *sv, enum pcg_form form, const double *d_b, double *d_x) {
  form_vecs(sv, sv->form);
  switch (form) {
  case PCG_CG1:
    cg1_enqueue_init(sv, d_b, d_x);
    break;
  case PCG_GENERIC:
  case PCG_FSAI3:
    gen_enqueue_init(sv, d_b, d_x);
    break;
  default: /* CLASSIC, SUBWAVE, COL */
    classic_enqueue_init(sv, d_b, d_x);
  }
}

/* One PCG iteration, enqueued.  sample >= 0: bracket the SpMV of shard 0 with
 * events 4*sample .. 4*sample+3.  pos: bit 0 = first, bit 1 = last iteration of
 * the run being enqueued. */
static void pcg_enqueue_iter(lsb_hip_solver *sv, enum pcg_form form, double *d_x, int parity, int sample, int pos) {
  switch (form) {
  case PCG_FSAI3:
    fsai_enqueue_iter(sv, d_x, parity, pos);
    break;
  case PCG_GENERIC:
    gen_enqueue_iter(sv, d_x, parity, sample);
    break;
  case PCG_CG1:
    cg1_enqueue_iter(sv, d_x, parity, sample);
    break;
  case PCG_SUBWAVE:
    subwave_enqueue_iter(sv, d_x, parity, pos);
    break;
  case PCG_COL:
    col_enqueue_iter(sv, d_x, parity, pos, sample);
    break;
  default: /* CLASSIC */
    classic_enqueue_iter(sv, d_x, parity, sample);
  }
}

/* Bytes ONE iteration of the Krylov loop must move on shard 0: the SpMV's layout bytes
 * (lsb_hip_solver_spmv_layout_bytes) + every vector pass of the sweeps behind it.  Classic PCG:
 * k_pcg_update_xr reads x p q r and writes x r, k_pcg_update_p reads r p and writes p -- 9 passes,
 * + 2 reads of the inverse diagonal where it is a vector; the single-reduction form: 9 passes with
 * a constant diagonal (u = dc r never stored), else 11 + the diagonal.  0 where the iteration is
 * something else (GMRES, a polynomial / block / FSAI preconditioner, the one-launch and
 * two-launch forms of small operators, fp32 values, the multi-pass SpMV forms).
 * BiCGSTAB: two SpMVs + the 18 passes of its four sweeps (hip_bicgstab.hip), + 2 reads of the diagonal. */
unsigned long long lsb_hip_solver_iteration_bytes(const lsb_hip_solver *sv) {
  const struct shard *s = &sv->sh[0];
  const unsigned long long sp = lsb_hip_solver_spmv_layout_bytes(sv), n8 = 8ull * s->n;
  const unsigned vec = s->dinv_uniform ? 0u : 1u;
  if (!sp || s->mixed || sv->ps.use || sv->o.krylov == LSB_KRYLOV_RICHARDSON || /* (a cycle: amg_cycle_bytes) */
      sv->o.krylov == LSB_KRYLOV_DIRECT)                                        /* (a round: direct_info) */
    return 0;
  if (sv->o.krylov == LSB_KRYLOV_BICGSTAB)
    return 2 * sp + n8 * (18u + 2u * vec);
  switch (sv->form) {
  case PCG_CLASSIC:
    return sp + n8 * (9u + 2u * vec);
  case PCG_CG1:
    return sp + n8 * (sv->cg1_implicit ? 9u : 11u + vec);
  case PCG_COL: /* k_pcg_col_px: r p x in, p' x out; k_pcg_col_r: p' r in, r out; the layout's matrix-side bytes
                   (sp less its x-in / y-out) in both */
    return 2 * (sp - 2 * n8) + 15 * n8 / 2; /* (x and the stale direction only every second iteration: 6 and 3 passes) */
  default:
    return 0;
  }
}

int lsb_hip_solver_single_reduction(const lsb_hip_solver *sv) { return sv->form == PCG_CG1; }
/* Iterations per host poll: run_chunk on the classic iteration's bytes (the SpMV at 12 B per non-zero, the sweeps'
 * passes and the SpMV's own), at least 8, even */
static int auto_chunk(const lsb_hip_solver *sv) {
  const struct shard *s = &sv->sh[0];
  double bytes = 12.0 * (double)s->nnz + 108.0 * (double)s->n;
  if (sv->dist) /* must not depend on this rank's own shard size */
    bytes = 12.0 * (double)sv->agree_nnz + 108.0 * (double)sv->agree_n;
  return run_chunk(bytes, 6.0, 8, 256) & ~1;
}

/* `reps` local iterations of the classic form on shard 0 (SpMV + the two sweeps; no exchange, no
 * all-reduce, no stop) behind 4 untimed ones: milliseconds */
static float time_local_iters(lsb_hip_solver *sv, double *d_b, double *d_x, int reps, unsigned nt) {
  struct shard *s = &sv->sh[0];
  const unsigned n = s->n;
  double *p = s->d_pfull + s->row_begin;
  unsigned np2 = 0, npq = 0;
  lsb_k_pcg_init(n, d_b, DINV(s), d_x, s->d_r, p, s->d_parts2, &np2, g_stream);
  lsb_k_pcg_init_state(s->d_st, s->d_parts2, np2, 0.0, 1 << 30, g_stream);
  const int warm = 4;
  for (int i = 0; i < warm + reps; i++) {
    if (i == warm)
      LSB_CHK_HIP(hipEventRecord(sv->ev_t0, g_stream));
    spmv_shard(s, s->d_pfull, s->d_q, p, s->d_parts_pq, &npq, s->d_st);
    lsb_k_pcg_update_xr(n, p, s->d_q, DINV(s), d_x, s->d_r, s->d_st, i & 1, s->d_parts_pq, npq, s->d_parts2, &np2,
                        nt, g_stream);
    lsb_k_pcg_update_p(n, s->d_r, DINV(s), p, p, s->d_st, i & 1, s->d_parts2, np2, nt, g_stream);
  }
  LSB_CHK_HIP(hipEventRecord(sv->ev_t1, g_stream));
  LSB_CHK_HIP(hipEventSynchronize(sv->ev_t1));
  float ms = 0.f;
  LSB_CHK_HIP(hipEventElapsedTime(&ms, sv->ev_t0, sv->ev_t1));
  /* a run that left RUNNING (exact convergence, a p.q breakdown) turned its later launches into
   * no-ops: such a sample says nothing */
  int status = 0;
  LSB_CHK_HIP(hipMemcpy(&status, &s->d_st->status, sizeof status, hipMemcpyDeviceToHost));
  return status == LSB_STATUS_RUNNING ? ms : -1.f;
}

/* WHERE the vectors land.  Round 3 found the iteration of config 3 in two speeds -- 136 and 143-144 us,
 * SpMV in the solve 25.5 and 32 us -- from one solver to the next of ONE process: r, q and the gather
 * vector are 240 MB of the 256 MB Infinity Cache, and which of their lines fight for the same sets was
 * decided by the physical pages three separate hipMallocs happened to get.  Round 3 drew placements
 * until three fast ones agreed (up to six sets, 1.2 GB of transient allocations).  Round 4 removes the
 * draw: the shard's vectors are carved out of ONE allocation (shard_vec, hip_solver.c), a contiguous
 * run of addresses covers the cache's sets evenly, and every solver of every process runs at the fast
 * speed by construction -- 8 fresh solvers in a row 136.4-136.8 us per iteration, against 136.7-142.7
 * from separate allocations and 136.3-137.4 with round 3's lottery (tools/gpu_r4_place.sh,
 * profiles/r04_placement.txt; general values 234.8-235.9 against 235.4-238.2).  It serves every
 * configuration (shards, Chebyshev / block-Jacobi, any vector size) and costs nothing.
 * LSBENCH_HIP_NO_SLAB=1 is the A/B switch.
 * That table is the THREE-launch form's.  The two-launch form (k_pcg_col_px + k_pcg_col_r) streams r, both
 * direction buffers and x, and until round 6 only r and the first direction were in the slab: the second was
 * taken by the first init, did not fit and got a hipMalloc of its own, and a padded solver's x (d_xp) was one
 * more -- round 3's draw again.  Now shard_upload counts and carves the second direction buffer, and a padded
 * or re-ordered one-shard solver's x and b come out of shard 0's slab right behind it: r, q, p0, p1, x, b in
 * one run of addresses (lsb_hip_solver_slab_mask says which are inside; profiles/r06_col_cache.txt has the
 * eight-solver table of this form).  An UNPADDED solver's x is the caller's and lands where the caller put it. */

/* Which operands of the two BLAS-1 sweeps should be loaded NONTEMPORAL is a matter of what the next
 * launches read again, and that depends on how the vectors compare with the 256 MB Infinity Cache:
 * measured per iteration of the classic form (tools/gpu_nt_masks.sh, profiles/r03_nt_masks.txt;
 * mask bits: 0 x, 1 p and q, 2 r in k_pcg_update_xr; 3 r, 4 p in k_pcg_update_p)
 *                                   all (rounds 1, 2)   x + r of the p-sweep (9)   none (0)
 *   config 3, 80 MB vectors              156.7 us            137.0 us            147.6 us
 *   1/8 of config 3, 10 MB vectors        30.5                28.7                26.9
 *   config 4, 512 MB vectors            1297.9              1292.1              1235.8
 *   config 3's pattern, general values   248.9               238.0               253.5
 * -- with the direction p loaded nontemporal by the p-sweep the SpMV that follows finds it nowhere
 * near and runs 39-44 us on config 3; left in the caches, 25.4 us.  So the solver times a few
 * iterations of its own first shard (local launches only: no exchange, no all-reduce) under each
 * candidate at creation -- untimed set-up, like the SpMV's timing pass -- and keeps the fastest.
 * LSBENCH_HIP_BLAS1_NT=<mask> fixes it (1 = everything, the old setting). */
void tune_blas1_nt(lsb_hip_solver *sv) {
  struct shard *s = &sv->sh[0];
  const int e = sv->o.blas1_nt >= 0; /* a mask was asked for (opts.blas1_nt, LSBENCH_HIP_BLAS1_NT): no timing */
  sv->nt_mask = e ? (sv->o.blas1_nt == 1 ? 63 : sv->o.blas1_nt & 63) : 63; /* not the previous solver's choice */
  /* (the iterations with z = M^-1 r as a vector run other sweeps around the SpMV -- dot2, the
   * Chebyshev recurrence in the epilogue: the classic form's winner cost them 8-10 % on config 3
   * (profiles/r03_bench.jsonl history).  They keep every operand nontemporal but the direction the
   * SpMV behind k_pcg_update_p gathers: outer SpMV 39 -> 29-33 us, Chebyshev 4 / 16 and block-Jacobi 8
   * on config 3 0.971 / 1.285 / 0.399 -> 0.974 / 1.289 / 0.408 solves/s, tools/gpu_nt_generic.sh) */
  if (!e && generic_precond(sv) && s->nnz >= 4000000ull)
    sv->nt_mask = 63 & ~16;
  if (s->nnz < 4000000ull || generic_precond(sv) || sv->o.krylov == LSB_KRYLOV_GMRES ||
      sv->o.krylov == LSB_KRYLOV_BICGSTAB || sv->o.krylov == LSB_KRYLOV_DIRECT)
    return; /* (GMRES, BiCGSTAB and the direct solver run none of these sweeps) */
  static const int cand[] = {63, 9, 5, 0};
  const unsigned n = s->n;
  double *d_b = (double *)lsb_hip_malloc((size_t)n * sizeof(double));
  double *d_x = (double *)lsb_hip_malloc((size_t)n * sizeof(double));
  lsb_k_fill_index(n, 1u, d_b, g_stream);
  float best = 1e30f;
  int bm = sv->nt_mask;
  const int reps = 20;
  for (unsigned c = 0; c < sizeof cand / sizeof cand[0] && !e; c++) {
    const float ms = time_local_iters(sv, d_b, d_x, reps, cand[c]);
    if (sv->o.verbose > 1)
      fprintf(stderr, "hip_cdna4: nontemporal mask %2d: %.1f us per iteration of the first shard\n", cand[c],
              ms * 1e3f / reps);
    if (ms >= 0.f && ms < best)
      best = ms, bm = cand[c];
  }
  /* the single-reduction sweep (k_cg1_update) goes with the classic ones: nontemporal unless
   * "none" won */
  if (!e)
    sv->nt_mask = bm == 0 ? 0 : (bm | 32);
  /* leave the shard as the upload left it */
  LSB_CHK_HIP(hipMemsetAsync(s->d_pfull, 0, (size_t)sv->n_glob * sizeof(double), g_stream));
  LSB_CHK_HIP(hipMemsetAsync(s->d_st, 0, sizeof(struct lsb_pcg_state), g_stream));
  LSB_CHK_HIP(hipStreamSynchronize(g_stream));
  lsb_hip_free(d_b), lsb_hip_free(d_x);
}

/* ------------------------------------------------------------------------ */
/* launch-bound operators: one persistent launch per solve (hip_persist.hip)   */
/* ------------------------------------------------------------------------ */
static int persist_run(lsb_hip_solver *sv, const double *d_b, double *d_x, double tol, int maxit) {
  struct shard *s = &sv->sh[0];
  int dev = 0, khz = 100000;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0)
    khz = 100000, (void)hipGetLastError();
  LSB_CHK_HIP(hipMemsetAsync(sv->ps.d_shared, 0, 64, g_stream));
  return lsb_k_pcg_persist(s->n, sv->ps.G, sv->ps.stride, sv->ps.d_wgrow, s->csr.offs, s->csr.cols,
                           s->csr.vals, s->d_dinv, d_b, d_x, sv->ps.d_ug, sv->ps.d_shared, s->d_st, tol,
                           maxit, sv->ps.lanes, 2000ll * khz, g_stream);
}

/* Does the operator qualify, how are its rows dealt to the workgroups, and (opts.
 * persistent = -1) which form is faster on THIS operator: 40 iterations each way,
 * timed at creation -- setup is untimed, like the reference's csr_init. */
void persist_setup(lsb_hip_solver *sv) {
  const struct lsb_hip_opts *o = &sv->o;
  struct shard *s = &sv->sh[0];
  unsigned nzmax, rmax, gmax;
  const unsigned nmax = lsb_k_persist_limits(&nzmax, &rmax, &gmax);
  if (sv->multi || sv->nshard != 1 || o->persistent == 0 || o->sample_spmv > 0 ||
      o->krylov == LSB_KRYLOV_GMRES || o->krylov == LSB_KRYLOV_BICGSTAB || o->krylov == LSB_KRYLOV_DIRECT ||
      s->n > nmax || s->n < 2 ||
      (o->precond != LSB_PRECOND_JACOBI && o->precond != LSB_PRECOND_NONE &&
       o->precond != LSB_PRECOND_L1JACOBI) ||
      o->precision != LSB_PREC_FP64)
    return;
  const char *e = getenv("LSBENCH_HIP_PERSIST_WGS");
  unsigned G = e ? (unsigned)atoi(e) : 32u;
  const unsigned need = (unsigned)((s->nnz + nzmax * 3 / 4 - 1) / (nzmax * 3 / 4));
  if (G < need)
    G = need;
  if (G < (s->n + rmax - 1) / rmax)
    G = (s->n + rmax - 1) / rmax;
  if (G > s->n / 2)
    G = s->n / 2 ? s->n / 2 : 1;
  if (G > gmax || G < 1)
    return;
  /* rows to workgroups: contiguous, balanced by non-zeros */
  int *offs = (int *)malloc(((size_t)s->n + 1) * sizeof(int));
  unsigned *row = (unsigned *)malloc(((size_t)G + 1) * sizeof(unsigned));
  LSB_CHK_HIP(hipMemcpy(offs, s->csr.offs, ((size_t)s->n + 1) * sizeof(int), hipMemcpyDeviceToHost));
  int ok = 1;
  row[0] = 0;
  for (unsigned g = 1, r = 0; g <= G; g++) {
    const unsigned long long want = s->nnz * g / G;
    while (r < s->n && (unsigned long long)offs[r + 1] <= want && s->n - (r + 1) >= G - g)
      r++;
    if (g < G && r <= row[g - 1])
      r = row[g - 1] + 1; /* at least one row each */
    row[g] = g == G ? s->n : r;
    ok &= row[g] - row[g - 1] <= rmax && row[g] > row[g - 1] &&
          (unsigned)(offs[row[g]] - offs[row[g - 1]]) <= nzmax;
  }
  free(offs);
  if (!ok) {
    free(row);
    return;
  }
  sv->ps.G = G;
  e = getenv("LSBENCH_HIP_PERSIST_STRIDE"); /* 8: the working workgroups share one XCD */
  sv->ps.stride = e ? (unsigned)atoi(e) : 1u;
  if (sv->ps.stride < 1)
    sv->ps.stride = 1;
  sv->ps.lanes = s->lanes > 32 ? 32 : s->lanes;
  sv->ps.d_wgrow = (unsigned *)dev_upload(row, ((size_t)G + 1) * sizeof(unsigned));
  LSB_CHK_HIP(hipStreamSynchronize(g_stream));
  free(row);
  sv->ps.d_ug = (double *)lsb_hip_malloc((size_t)s->n * sizeof(double));
  sv->ps.d_shared = lsb_hip_malloc(lsb_k_persist_shared_bytes());
  sv->ps.ok = 1;
  if (o->persistent > 0) {
    sv->ps.use = 1;
    return;
  }
  /* auto: 40 iterations of each form on b_i = i, best of 3 */
  double *d_b = (double *)lsb_hip_malloc((size_t)s->n * sizeof(double));
  double *d_x = (double *)lsb_hip_malloc((size_t)s->n * sizeof(double));
  lsb_k_fill_index(s->n, s->row_begin + 1, d_b, g_stream);
  const struct lsb_hip_opts keep = sv->o;
  sv->o.tol = 0.0, sv->o.maxit = 40, sv->o.verify = 0;
  double best[2] = {1e30, 1e30};
  for (int form = 0; form < 2; form++) {
    sv->ps.use = form;
    for (int rep = 0; rep < 4; rep++) {
      struct lsb_hip_result r;
      solve_core(sv, d_b, d_x, &r);
      if (rep && r.seconds < best[form])
        best[form] = r.seconds;
      if (form == 1 && r.status == LSB_STATUS_COMM)
        best[1] = 1e30;
    }
  }
  sv->o = keep;
  memset(sv->hint_iters, 0, sizeof sv->hint_iters);
  drop_graphs(sv);
  sv->ps.us_launches = best[0] * 1e6, sv->ps.us_persist = best[1] * 1e6;
  sv->ps.use = best[1] < best[0];
  if (o->verbose)
    fprintf(stderr, "hip_cdna4: 40 iterations: %.1f us as one persistent launch (%u workgroups), "
                    "%.1f us as launches -> %s\n", best[1] * 1e6, G, best[0] * 1e6,
            sv->ps.use ? "persistent" : "launches");
  lsb_hip_free(d_b), lsb_hip_free(d_x);
}

/* what run_loop enqueues: iterations of one form writing to d_x, as plain launches -- every sample_spmv-th of the
 * run with its SpMV bracketed by events -- or replayed from a graph (the form a run takes depends on the solver and
 * d_x alone: the cache's key holds it) */
struct pcg_enq {
  lsb_hip_solver *sv;
  enum pcg_form form;
  double *d_x;
  int use_graph, nsamp;
  unsigned done; /* iterations enqueued so far in this run */
};
static void pcg_enqueue_iters(void *ctx, int cnt) {
  struct pcg_enq *e = ctx;
  lsb_hip_solver *sv = e->sv;
  for (int i = 0; i < cnt; i++) {
    int smp = -1;
    if (sv->o.sample_spmv > 0 && e->nsamp < MAX_SAMPLES &&
        ((e->done + (unsigned)i) % (unsigned)sv->o.sample_spmv) == 0)
      smp = e->nsamp++;
    pcg_enqueue_iter(sv, e->form, e->d_x, i & 1, smp, (i == 0) | ((i == cnt - 1) << 1));
  }
}
static void pcg_enqueue(void *ctx, int cnt) {
  struct pcg_enq *e = ctx;
  if (e->use_graph)
    graph_launch(&e->sv->graphs, cnt, e->d_x, pcg_enqueue_iters, ctx);
  else
    pcg_enqueue_iters(ctx, cnt);
  e->done += (unsigned)cnt;
}

/* One CG run from x0 = 0 to sv->tol_run; `round` = 0 for the solve proper, k for
 * its k-th correction run. */
int pcg_run(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res, int round) {
  unsigned *hint = hint_slot(sv->hint_iters, round);
  const int chunk = sv->o.check_every > 0 ? (sv->o.check_every + 1) & ~1 : auto_chunk(sv);
  memset(sv->samp_skip, 0, sizeof sv->samp_skip);
  struct pcg_enq enq = {.sv = sv, .d_x = d_x, .use_graph = sv->o.use_graph && !sv->multi && sv->o.sample_spmv <= 0,
                        /* k_pcg_col_px loads and stores x as 16-byte vectors: any other x runs the classic form */
                        .form = sv->form == PCG_COL && ((uintptr_t)d_x & 15) ? PCG_CLASSIC : sv->form};
  struct lsb_pcg_state *hst = sv->h_st; /* two pinned slots */
  double t0 = wall_seconds();
  if (sv->ps.use) {
    /* one launch, one look at the state it leaves */
    if (persist_run(sv, d_b, d_x, sv->tol_run, (int)sv->o.maxit) != 0)
      errx(EXIT_FAILURE, "hip_cdna4: the persistent solve kernel could not be launched");
    LSB_CHK_HIP(hipMemcpyAsync(&hst[0], sv->sh[0].d_st, sizeof(struct lsb_pcg_state),
                               hipMemcpyDeviceToHost, g_stream));
    LSB_CHK_HIP(hipStreamSynchronize(g_stream));
    if (hst[0].status == LSB_STATUS_COMM) {
      warnx("hip_cdna4: the persistent solve's workgroups did not all arrive (the device is "
            "shared?); using the launch-per-kernel form from here on");
      sv->ps.use = 0;
      return pcg_run(sv, d_b, d_x, res, round);
    }
    struct lsb_hip_result r;
    memset(&r, 0, sizeof r);
    result_from_state(&r, &hst[0]);
    r.seconds = wall_seconds() - t0, r.true_relres = -1.0;
    *hint = r.iters;
    if (res)
      *res = r;
    return 0;
  }

  pcg_enqueue_init(sv, enq.form, d_b, d_x);
  /* graphs beyond ~1k iterations cost more to build than they save: max_piece */
  const struct run_loop loop = {.name = "PCG", .d_state = sv->sh[0].d_st, .h_state = hst,
                                .state_bytes = sizeof(struct lsb_pcg_state),
                                .stop_off = offsetof(struct lsb_pcg_state, status),
                                .progress_off = offsetof(struct lsb_pcg_state, iters),
                                .enqueue = pcg_enqueue, .ctx = &enq, .chunk = chunk, .even = 1,
                                .max_piece = enq.use_graph ? 1024 : 0, .cap = -1,
                                .what_hinted = "poll of a hinted solve", .what_poll = "poll of the solve",
                                .what_drain = "drain after the solve"};
  hst[0].iters = 0; /* every run starts from its own init: the hint is the run's whole count */
  run_loop(sv, &loop, hint);
  if (hst[0].status == LSB_STATUS_COMM)
    lsb_give_up("hip_cdna4: a peer did not arrive within the time-out of the direct "
                "xGMI path (LSBENCH_HIP_P2P_TIMEOUT_MS); iteration %d (rank %d of %d)", hst[0].iters,
                lsb_hip_comm_rank(), lsb_hip_comm_size());
  /* (single-reduction form: r.r of the maxit-th update and the final status --
   * MAXIT, or CONVERGED exactly at maxit -- are settled on the device by the
   * launch after it, k_cg1_update's `pend` branch) */
  double t1 = wall_seconds();
  struct lsb_hip_result r;
  memset(&r, 0, sizeof r);
  result_from_state(&r, &hst[0]);
  r.seconds = t1 - t0;
  const int nsamp = enq.nsamp;
  if (nsamp > 0) {
    double tot = 0.0;
    int used = 0;
    for (int k = 0; k < nsamp; k++) {
      float ms = 0.f;
      /* samples enqueued after convergence time a no-op launch: skip them */
      if ((unsigned)k * (unsigned)sv->o.sample_spmv >= r.iters)
        break;
      if (sv->samp_skip[k])
        continue;
      float pair = 0.f;
      LSB_CHK_HIP(hipEventElapsedTime(&ms, sv->ev[4 * k], sv->ev[4 * k + 1]));
      LSB_CHK_HIP(hipEventElapsedTime(&pair, sv->ev[4 * k + 2], sv->ev[4 * k + 3]));
      /* (a host hiccup between the two bare markers can make their distance exceed the bracketed
       * launch's on a launch of a few microseconds: such a sample says nothing) */
      if (ms > pair)
        tot += ms - pair, used++;
    }
    r.spmv_ms = used ? tot / used : 0.0;
    r.spmv_samples = (unsigned)used;
  }
  check_aux_status(sv, "solve");
  r.true_relres = -1.0;
  if (res)
    *res = r;
  return 0;
}

/* products with the operator of a PCG solve and its correction runs, from the counts in *r */
unsigned pcg_spmvs(const lsb_hip_solver *sv, const struct lsb_hip_result *r) {
  const unsigned m = sv->o.precond == LSB_PRECOND_CHEBYSHEV ? (unsigned)sv->cheb_m : 0u;
  return r->iters * (1u + m) + (1u + r->corrections) * (m + (sv->form == PCG_CG1 || sv->ps.use ? 1u : 0u)) +
         (r->true_relres >= 0.0 ? 1u + r->corrections : 0u);
}

/* One PCG solve from x0 = 0 as the caller sees it (the driver's entry point, hip_solve.c): the run, then -- opts.verify,
 * or always when the direct xGMI path carried the run -- the recomputed residual and the correction runs of
 * verify_correct. */
int pcg_solve_dev(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res) {
  const double t0 = wall_seconds();
  struct lsb_hip_result r;
  /* Mixed precision: the CG runs see S~ = fp32(S) (fp64 vectors and sums) and
   * are the inner solves of an iterative refinement on the fp64 operator,
   * x += S~^-1 (b - S x); each is asked for no more than the rounding of the
   * values lets it deliver (where rounding changed no value -- the Laplacians --
   * S~ = S and the first run is the whole solve). */
  sv->tol_run = fmax(sv->o.tol, mixed_floor_tol(sv));
  pcg_run(sv, d_b, d_x, &r, 0);
  const double bb = sv->h_st->bb;
  if (sv->p2p_on && !direct_path_agrees(sv, d_b, d_x, bb, &r, "solving again"))
    return pcg_solve_dev(sv, d_b, d_x, res); /* from zero, over RCCL */
  verify_correct(sv, d_b, d_x, &r, bb, 0);
  r.seconds = wall_seconds() - t0;
  r.spmvs = pcg_spmvs(sv, &r);
  if (res)
    *res = r;
  g_last = r;
  return 0;
}
