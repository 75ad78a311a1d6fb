/*
 * Internal header of liblsbench_hip.so: the role src/lsbench-impl.h plays in
 * the reference (struct layouts + backend prototypes), plus the launcher
 * prototypes of the HIP shim (hip_kernels.hip, hip_sweeps.hip) that hip_cdna4.c calls.
 */
#ifndef LSB_IMPL_H
#define LSB_IMPL_H

#include "lsbench_hip.h"
#include <err.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#ifdef __cplusplus
extern "C" {
#endif

#define lsb_calloc(T, n) ((T *)calloc((size_t)(n) > 0 ? (size_t)(n) : 1, sizeof(T)))

/* ---- device-side PCG scalars (one per shard, lives in HBM) -------------- */
struct lsb_pcg_state {
  double rz[2];    /* r.z, double-buffered by iteration parity              */
  double bb;       /* b.b                                                    */
  double thresh2;  /* tol^2 * b.b                                            */
  double rr;       /* r.r after the last completed iteration                 */
  double pq;       /* p.q of the last completed iteration (diagnostic)       */
  double alpha[2]; /* single-reduction CG: step length, parity-buffered      */
  int iters;       /* completed iterations                                   */
  int status;      /* LSB_STATUS_*; != 0 makes every later kernel a no-op    */
  int maxit;
  int pad;       /* single-reduction CG and the column form's two-launch iteration:
                    1 = the maxit-th update has run, the next launch turns it into
                    the final status (never set and tested in the same launch) */
  int xpend;     /* two-launch iteration on a z-column plan (k_pcg_col_px): 1, 2 = x is one
                    update behind -- x += alpha[0] p with p in direction buffer
                    xpend - 1; 3, 4 = two behind -- x += alpha[1] p'' + alpha[0] p, p in
                    buffer xpend - 3, p'' in the other; 0 = x is up to date      */
  int pad2_;
};

/* ---- the direct-xGMI all-reduce folded into neighbouring launches (hip_ar.h) ---
 * lsb_ar_tail: handed BY VALUE to the SpMV launch that writes the last dot
 * partials of an iteration; counter == NULL: no tail.  lsb_ar_collect: handed
 * to k_cg1_update, which then takes w.u, r.u, r.r from the mailbox instead of
 * from reduced scalars; mbox == NULL: off.  Filled by lsb_p2p_fold_*. */
struct lsb_ar_tail {
  unsigned *counter;          /* workgroups of the launch that have handed in */
  const double *parts;        /* ALL dot partials of this SpMV: the earlier launches' of a
                                 split SpMV first, then this launch's (one per workgroup) */
  const double *parts2;       /* the sweep's records: nparts2 of width2 */
  char *const *peer;          /* mailboxes of all ranks (device array) */
  unsigned long long epoch;
  unsigned nparts_before, nparts2, width2;
  int R, me;
};
/* A Chebyshev step riding in the epilogue of the 16-bit sliced-ELL SpMV (one shard):
 * with w = (S z)_row just formed, d = a d + b D^-1 (r - w) and z' = z + d for the lane's
 * own rows; z' goes to ANOTHER gather vector (other rows are still gathering z).
 * zout == NULL: off.  The same expression as k_cheb_step, bit for bit. */
struct lsb_cheb_epi {
  const double *r, *dinv; /* dinv == NULL: the constant dc */
  double *d, *zout;       /* local row indices */
  double dc, a, b;
};
struct lsb_ar_collect {
  char *mbox; /* the own mailbox */
  unsigned long long epoch;
  long long timeout; /* wall_clock64 ticks */
  int R;
};

/* ---- device-side GMRES(m) scalars ----------------------------------------- */
#define LSB_GMRES_MAX_RESTART 32
#define LSB_GMRES_PARTIALS 512
struct lsb_gmres_state {
  double bnorm, thresh, beta, resid, hnorm;
  double g[LSB_GMRES_MAX_RESTART + 1];
  double cs[LSB_GMRES_MAX_RESTART], sn[LSB_GMRES_MAX_RESTART], y[LSB_GMRES_MAX_RESTART];
  double R[LSB_GMRES_MAX_RESTART * LSB_GMRES_MAX_RESTART]; /* R[i*MAX + j] */
  int iters, status, maxit, restart, jlast, cycle_open;
};

/* ---- device-side BiCGSTAB scalars (hip_bicgstab.hip) -------------------------
 * c: the words the SpMV launchers and the reduction helpers gate on and the host polls -- status,
 * iters, maxit, bb, thresh2 = tol^2 bb, rr (the last residual norm formed, squared); its other
 * fields are not used.  alpha, omega and beta never leave the device. */
struct lsb_bcg_state {
  struct lsb_pcg_state c;
  double rho[2];  /* r^.r, double-buffered by iteration parity */
  double alpha, omega;
  int half;       /* 1: k_bcg_xr took the half step; k_bcg_p behind it sets CONVERGED */
  int nspmv;      /* products with Op of the iterations run: 2 per full one, 1 for a half step, the
                     one or two of an iteration that ended in a breakdown */
};

/* ---- device-side state of a batch of right-hand sides (hip_mrhs.hip) -----------
 * One lsb_pcg_state per column (status, iters, maxit, bb, thresh2, rr, rz[2], pq are used; under FSAI also
 * alpha[parity], the step length on its way from one row kernel to the next) and the words
 * of the batch.  A column whose status != 0 is frozen; running = some column's status is 0. */
#define LSB_MRHS_MAX 8
struct lsb_mrhs_state {
  struct lsb_pcg_state c[LSB_MRHS_MAX];
  double true_relres[LSB_MRHS_MAX]; /* opts.verify: ||b_c - S x_c|| / ||b_c|| of the last round, -1: none */
  double tol;
  int corrections[LSB_MRHS_MAX];    /* in-place restarts of the column */
  int running;                      /* the SpMM's gate: cleared by the sweep that sees the last column stop */
  int nspmm;                        /* SpMM launches of the iterations that did work */
  double start_relres[LSB_MRHS_MAX]; /* a batch from an initial guess: ||b_c - S x0_c|| / ||b_c||, 0 where b_c = 0 */
};

/* Upper bound on per-launch partial sums any reduction kernel writes; the
 * consumer kernels re-reduce them in fixed order (deterministic). */
#define LSB_MAX_PARTIALS 2048
/* Workgroups of a launch that only streams vectors: three per CU.  More of them stream SLOWER once
 * the vectors come out of HBM (lsb_k_blas1_grid, profiles/r03_sweep_grid.txt). */
#define LSB_STREAM_GRID_CAP 768
/* Non-zeros staged in LDS per row block of the adaptive SpMV (16 KiB). */
#define LSB_BLOCK_NNZ 2048

/* ---- HIP shim: kernel launchers (hip_kernels.hip, hip_sweeps.hip) ---------
 * All take raw device pointers and a hipStream_t as void*.  `st` may be NULL
 * for the stand-alone (non-PCG) use of a kernel; when given, a non-zero
 * st->status turns the launch into a no-op on the device. */
void lsb_k_spmv(int variant, unsigned n, const int *offs, const int *cols,
                const double *vals, const int *rowblk,
                const unsigned char *blklanes, unsigned nblk,
                unsigned lanes_per_row, unsigned flags, unsigned grid_cap,
                const double *x, double *y, const double *xdot,
                double *partials, unsigned *npartials,
                const struct lsb_pcg_state *st, const int *rowmap,
                const struct lsb_ar_tail *tail, void *stream);
int lsb_k_spmv_has_tail(int variant); /* the variant's kernel can carry an lsb_ar_tail */
unsigned lsb_k_spmv_grid(int variant, unsigned n, unsigned nblk,
                         unsigned lanes_per_row, unsigned grid_cap);
/* flags of the adaptive SpMV (picked by the timing pass at solver creation) */
#define LSB_SP_PREFETCH 1u
#define LSB_SP_NT 2u
#define LSB_SP_C16 4u /* sliced-ELL only: 16-bit column codes */
#define LSB_SP_F32 32u /* the values pointer holds fp32 (opts.precision = LSB_PREC_MIXED) */
void lsb_k_spmv_sell(unsigned flags, unsigned grid_cap, unsigned period, const unsigned *sptr,
                     unsigned s0, unsigned ns, unsigned n, unsigned row_begin, unsigned xlen,
                     const void *cols,
                     const int *sbase, const double *vals, const double *vconst, unsigned ulen,
                     const double *x, double *y, const double *xdot, double *partials,
                     unsigned *npartials,
                     const struct lsb_pcg_state *st, const struct lsb_ar_tail *tail,
                     const struct lsb_cheb_epi *epi, void *stream);
#define LSB_SP_TMPL 64u /* 16-bit sliced-ELL with constant slots: slice templates (k_spmv_tmpl) */
#define LSB_SP_DEFER 128u /* k_spmv_tmpl: a turn's y is parked in LDS and stored by the wave's next turn */
/* A shard's 16-bit sliced-ELL copy on the device (lsb_csr_sellize16) with its constant slots
 * (lsb_sell16_value_slots) and slice templates (lsb_sell16_templates): the operands the template
 * launchers below unpack */
struct lsb_sell16_dev {
  unsigned *sptr;
  short *codes;
  int *sbase;
  double *vals;   /* the kept value slots (floats under LSB_SP_F32) */
  double *vconst; /* != NULL: the constant-slot layout -- sbase holds 4 ints per slot, vals only the
                     vslots slots that keep their values */
  unsigned vslots, slots, ulen; /* ulen != 0: every slice has this many slots */
  unsigned long long bytes; /* matrix-side bytes one launch streams */
  struct lsb_tmpl_dev { /* srec != NULL: the templates (LSB_SP_TMPL) */
    unsigned *srec; /* per slice {template id (255: none), first kept value slot, first mask, 0} */
    unsigned long long *mask;
    struct lsb_sell_tmpl *td;
    unsigned nfar;
    unsigned long long bytes;
  } tmpl;
};
void lsb_k_spmv_tmpl(unsigned flags, unsigned grid_cap, unsigned period, const struct lsb_sell16_dev *c, unsigned s0,
                     unsigned ns, unsigned n, unsigned row_begin, unsigned xlen, const double *x, double *y,
                     const double *xdot, double *partials, unsigned *npartials, const struct lsb_pcg_state *st,
                     const struct lsb_ar_tail *tail, const struct lsb_cheb_epi *epi, void *stream);
/* the classic PCG iteration in two launches on a z-column plan (hip_kernels.hip: k_pcg_col_px) */
void lsb_k_pcg_col_px(unsigned grid_cap, unsigned period, const unsigned *plan, unsigned nitem, unsigned n,
                      const struct lsb_sell16_dev *c, const double *r, const double *pold, double *pnew, double *x,
                      int xupd, double dc, double *partials, unsigned *npartials, struct lsb_pcg_state *st, int parity,
                      const double *parts2, unsigned nparts2, void *stream);
/* the r half: alpha, r -= alpha S p with S p formed again out of p (q is never stored), partials of (r.z', r.r);
 * rev: the turns take each XCD band's groups of four items in descending order */
void lsb_k_pcg_col_r(unsigned grid_cap, unsigned period, const unsigned *plan, unsigned nitem, unsigned n,
                     const struct lsb_sell16_dev *c, const double *p, double *r, double dc, struct lsb_pcg_state *st,
                     int parity, int pbuf, int xtwo, int rev, const double *pq_parts, unsigned npq, double *partials2,
                     unsigned *npartials, void *stream);
void lsb_k_pcg_xfix(unsigned n, const double *p0, const double *p1, double *x, const struct lsb_pcg_state *st,
                    void *stream);
#define LSB_SP_COL 256u /* k_spmv_tmpl_col: the template layout walked in z-columns (whole launches of a
                           shard that has a column plan; implies LSB_SP_TMPL) */
void lsb_k_spmv_tmpl_col(unsigned flags, unsigned grid_cap, unsigned period, const unsigned *plan, unsigned nitem,
                         int centre0, unsigned n, unsigned row_begin, unsigned xlen, const struct lsb_sell16_dev *c,
                         const double *x, double *y, const double *xdot, double *partials, unsigned *npartials,
                         const struct lsb_pcg_state *st, const struct lsb_ar_tail *tail, void *stream);
void lsb_k_spmv_binned(unsigned flags, unsigned chunk_cap, const unsigned *chunk_begin, unsigned c0,
                       unsigned nchunk, const unsigned *rows, const unsigned *cols, const double *vals,
                       const double *x, double *y, const struct lsb_pcg_state *st, void *stream);
void lsb_k_spmv_twophase(unsigned nitems, const unsigned *item, const double *vals,
                         const unsigned short *colw, const unsigned *grp_first,
                         const unsigned long long *grp_mask, const unsigned *delta,
                         const unsigned short *roww, unsigned col_lo, unsigned cols, unsigned rows,
                         unsigned nbins, const unsigned *bin_ptr, double *prod, unsigned n,
                         const double *x, unsigned xlen, double *y, const double *xdot,
                         double *partials, unsigned *npartials, double *binparts,
                         const struct lsb_pcg_state *st, void *stream);
unsigned lsb_k_twophase_groups(unsigned nbins);
void lsb_k_reduce_final(const double *partials, unsigned nparts, unsigned width,
                        double *out, int take_sqrt,
                        const struct lsb_pcg_state *st, void *stream);
void lsb_k_reduce_final2(const double *pa, unsigned na, unsigned wa, double *outa,
                         const double *pb, unsigned nb, unsigned wb, double *outb,
                         const struct lsb_pcg_state *st, void *stream);
void lsb_k_dot(unsigned n, const double *a, const double *b, double *partials,
               unsigned *npartials, void *stream);
void lsb_k_axpy(unsigned n, const double *alpha, const double *x, double *y,
                void *stream);
void lsb_k_xpay(unsigned n, const double *beta, const double *x, double *y,
                void *stream);
void lsb_k_jacobi_setup(unsigned n, unsigned row_begin, const int *offs,
                        const int *cols, const double *vals, double *dinv,
                        int *nzero, void *stream);
void lsb_k_l1_setup(unsigned n, const int *offs, const double *vals, double *dinv, int *nzero,
                    void *stream);
void lsb_k_jacobi_apply(unsigned n, const double *dinv, const double *r,
                        double *z, void *stream);
void lsb_k_jacobi_sweep(unsigned n, double w, const double *dinv,
                        const double *b, const double *ax, double *x,
                        void *stream);
/* PCG fused sweeps */
/* dinv == NULL: the Jacobi diagonal is the constant dc (not read from memory).  nt: which operands
 * the sweeps load nontemporal -- bit 0 x, 1 p and q, 2 r (update_xr); 3 r, 4 p (update_p); 5 cg1_update */
void lsb_k_pcg_init(unsigned n, const double *b, const double *dinv, double dc, double *x,
                    double *r, double *p, double *partials2,
                    unsigned *npartials, void *stream);
void lsb_k_pcg_init_state(struct lsb_pcg_state *st, const double *partials2,
                          unsigned nparts, double tol, int maxit,
                          void *stream);
/* q = S x - b off a CSR with global column ids into xfull, formed as in twice the working precision and rounded;
 * one partial of q.q per workgroup (<= LSB_MAX_PARTIALS) */
void lsb_k_resid_csr2(unsigned n, const int *offs, const int *cols, const double *vals, unsigned lanes,
                      const double *xfull, const double *b, double *q, double *partials, unsigned *npartials,
                      void *stream);
/* a solve from an initial guess: r0 = b - q (q = S x0), one record (r0.r0, b.b) per workgroup */
void lsb_k_x0_start(unsigned n, const double *b, const double *q, double *r0, double *partials2,
                    unsigned *npartials, void *stream);
void lsb_k_pcg_update_xr(unsigned n, const double *p, const double *q,
                         const double *dinv, double dc, double *x, double *r,
                         struct lsb_pcg_state *st, int parity,
                         const double *pq_parts, unsigned npq,
                         double *partials2, unsigned *npartials, unsigned nt, void *stream);
void lsb_k_spmv_subwave_p(unsigned n, const int *offs, const int *cols, const double *vals,
                          unsigned lanes_per_row, const double *r, const double *dinv, double dc,
                          const double *pold, double *pnew, double *y, double *partials,
                          unsigned *npartials, struct lsb_pcg_state *st, int parity,
                          const double *parts2, unsigned nparts2, void *stream);
void lsb_k_pcg_update_p(unsigned n, const double *r, const double *dinv, double dc,
                        const double *pin, double *p, struct lsb_pcg_state *st, int parity,
                        const double *parts2, unsigned nparts2, unsigned nt, void *stream);
void lsb_k_cg1_update(unsigned n, double *u, const double *w, const double *dinv, double dc,
                      double *p,
                      double *s, double *x, double *r, struct lsb_pcg_state *st, int parity,
                      const double *parts_gr, unsigned ngr, const double *parts_d, unsigned nd,
                      const struct lsb_ar_collect *collect, double *partials2, unsigned *npartials,
                      unsigned nt, void *stream);
unsigned lsb_k_blas1_grid(unsigned n);
void lsb_k_fill_index(unsigned n, unsigned first, double *v, void *stream);
void lsb_k_perm_gather(unsigned n, const int *perm, const double *src, double *dst,
                       void *stream);
void lsb_k_perm_scatter(unsigned n, const int *perm, const double *src, double *dst,
                        void *stream);
void lsb_k_vreduce(double *base, unsigned stride, unsigned nshard, unsigned off,
                   unsigned cnt, void *stream);

/* GMRES launchers (hip_gmres.hip) */
unsigned lsb_k_gm_grid(unsigned n);
void lsb_k_gm_resid(unsigned n, const double *b, const double *ax, double *v0,
                    double *partials, const struct lsb_gmres_state *st, void *stream);
void lsb_k_gm_begin(struct lsb_gmres_state *st, const double *partials, unsigned nparts,
                    double tol, int maxit, int restart, int first, void *stream);
void lsb_k_gm_scale_prec(unsigned n, const double *w, double *v, const double *dinv, double *z,
                         const struct lsb_gmres_state *st, void *stream);
void lsb_k_gm_multidot(unsigned n, const double *V, size_t ld, int cnt, const double *w,
                       double *partials, double *h, int accumulate,
                       const struct lsb_gmres_state *st, void *stream);
void lsb_k_gm_update_w(unsigned n, const double *V, size_t ld, int cnt, const double *h,
                       double *w, double *partials, const struct lsb_gmres_state *st,
                       void *stream);
void lsb_k_gm_hess(struct lsb_gmres_state *st, int j, const double *h, const double *h2,
                   const double *partials, unsigned nparts, void *stream);
void lsb_k_gm_finish_cycle(unsigned n, const double *V, size_t ld, const double *dinv, double *x,
                           struct lsb_gmres_state *st, void *stream);

/* Successive right-hand sides (hip_seq.hip): the projection onto m = 1 .. LSB_SEQ_MAX_DEPTH earlier solutions.  X, SX:
 * the pairs (x~_k, S x~_k), vector-major, column k at k ld with ld even.  partials: room for lsb_k_seq_grid(n) records
 * of m + 2 doubles.  A lane takes two neighbouring rows per turn and all of a turn's loads are issued before the first
 * is waited for; the operands need 8-byte alignment only, and the bits do not depend on it; the scalars are read from
 * device memory.
 * dots: alpha_k = sum_i X[k][i] v[i], reduced on the device.  combine: x0_i = sum_k alpha_k X[k][i], an fma chain in
 * ascending k from 0.0.  orth: d -= sum_k beta_k X[k], w -= sum_k beta_k SX[k] in place; out[0 .. m) = X[k] . w',
 * out[m] = d' . w', out[m + 1] = d . w from before the update -- dots' sums on the vectors just written, bit for bit.
 * store: xs = d / sqrt(*nu), sxs = w / sqrt(*nu) and rec = (*nu0, *nu, 1); *nu not finite or not > 0: rec = (*nu0, *nu,
 * 0) and nothing else. */
unsigned lsb_k_seq_grid(unsigned n);
void lsb_k_seq_dots(unsigned n, unsigned m, const double *X, size_t ld, const double *v, double *partials,
                    double *alpha, void *stream);
void lsb_k_seq_combine(unsigned n, unsigned m, const double *X, size_t ld, const double *alpha, double *x0,
                       void *stream);
void lsb_k_seq_orth(unsigned n, unsigned m, const double *X, const double *SX, size_t ld, const double *beta,
                    double *d, double *w, double *partials, double *out, void *stream);
void lsb_k_seq_store(unsigned n, const double *d, const double *w, double *xs, double *sxs, const double *nu,
                     const double *nu0, double *rec, void *stream);

/* BiCGSTAB launchers (hip_bicgstab.hip); dinv == NULL: the constant dc */
void lsb_k_bcg_init(unsigned n, const double *b, const double *dinv, double dc, double *x, double *r,
                    double *rhat, double *p, double *phat, double *partials, unsigned *npartials,
                    void *stream);
void lsb_k_bcg_init_state(struct lsb_bcg_state *st, const double *parts, unsigned nparts, double tol,
                          int maxit, void *stream);
void lsb_k_bcg_restart(unsigned n, const double *b, const double *ax, const double *dinv, double dc,
                       double *r, double *rhat, double *p, double *phat, double *partials,
                       unsigned *npartials, void *stream);
void lsb_k_bcg_restart_state(struct lsb_bcg_state *st, const double *parts, unsigned nparts, int more,
                             void *stream);
void lsb_k_bcg_s(unsigned n, double *r, const double *v, const double *dinv, double dc, double *shat,
                 struct lsb_bcg_state *st, int parity, const double *sig_parts, unsigned nsig,
                 double *partials, unsigned *npartials, void *stream);
void lsb_k_bcg_tt(unsigned n, const double *t, const struct lsb_bcg_state *st, double *partials,
                  unsigned *npartials, void *stream);
void lsb_k_bcg_xr(unsigned n, double *x, const double *phat, const double *shat, double *r, const double *t,
                  const double *rhat, struct lsb_bcg_state *st, const double *ss_parts, unsigned nss,
                  const double *ts_parts, unsigned nts, const double *tt_parts, unsigned ntt,
                  double *partials2, unsigned *npartials, void *stream);
void lsb_k_bcg_p(unsigned n, const double *r, double *p, const double *v, const double *dinv, double dc,
                 double *phat, struct lsb_bcg_state *st, int parity, const double *parts2, unsigned nparts2,
                 void *stream);

/* Several right-hand sides (hip_mrhs.hip): kp = 2, 4 or 8 columns, block vectors interleaved (element
 * (i, c) at i kp + c, 16-byte aligned); dinv == NULL: the constant dc.
 * pack / unpack: the caller's column-major block (leading dimension ld) <-> interleaved; perm[internal row]
 * = the caller's row, -1 on a pad row, NULL: the same numbering; columns >= nrhs are packed as zeros. */
void lsb_k_mrhs_pack(unsigned n, unsigned kp, unsigned nrhs, const int *perm, const double *src, size_t ld,
                     double *dst, void *stream);
void lsb_k_mrhs_unpack(unsigned n, unsigned kp, unsigned nrhs, const int *perm, const double *src, double *dst,
                       size_t ld, void *stream);
/* Y = S X off any CSR (n rows, `lanes` per row), one record of kp partials per workgroup: x_c . y_c, or --
 * bres != NULL -- y = bres - S x and y_c . y_c.  st != NULL: a no-op once st->running == 0. */
unsigned lsb_k_spmm_grid(unsigned n, unsigned lanes);
void lsb_k_spmm_csr(unsigned kp, unsigned n, const int *offs, const int *cols, const double *vals, unsigned lanes,
                    const double *x, double *y, const double *bres, double *partials, unsigned *npartials,
                    const struct lsb_mrhs_state *st, void *stream);
void lsb_k_mrhs_init(unsigned kp, unsigned n, const double *b, const double *dinv, double dc, double *x, double *r,
                     double *p, double *partials2, unsigned *npartials, void *stream);
/* bb_parts == NULL: the state of a batch from x0 = 0, b.b from the records of lsb_k_mrhs_init.  Else the state of a
 * batch from an initial guess: partials2 holds (r.z, r.r) of r = b - S x0 and bb_parts the records of
 * lsb_k_mrhs_x0_bb; a column with r.r <= tol^2 b.b is CONVERGED from the start */
void lsb_k_mrhs_init_state(unsigned kp, struct lsb_mrhs_state *st, const double *partials2, unsigned nparts,
                           const double *bb_parts, unsigned nbb, double tol, int maxit, void *stream);
/* A batch from an initial guess X0 (hip_mrhs_x0.hip), in three steps around the SpMM r = b - S x0 (bres = b):
 * x0_bb, before it: one record (0, then b.b per column) per workgroup, in lsb_k_mrhs_init's format and order.
 * x0_start, behind it: x_c = 0 for the columns with b_c = 0, p = dinv .* r and one record (r.z, r.r) per workgroup
 * by lsb_k_mrhs_init's expressions -- a column with x0 = 0 gets the bits of a batch from zero.
 * amg_mrhs_x0_start: the zeroing alone; the cycle on r and lsb_k_amg_mrhs_init_p (on r) follow. */
void lsb_k_mrhs_x0_bb(unsigned kp, unsigned n, const double *b, double *bb_parts, unsigned *nbb, void *stream);
void lsb_k_mrhs_x0_start(unsigned kp, unsigned n, const double *r, const double *dinv, double dc, double *x,
                         double *p, const double *bb_parts, unsigned nbb, double *partials2, unsigned *npartials,
                         void *stream);
void lsb_k_amg_mrhs_x0_start(unsigned kp, unsigned n, double *x, const double *bb_parts, unsigned nbb, void *stream);
void lsb_k_mrhs_update_xr(unsigned kp, unsigned n, const double *p, const double *q, const double *dinv, double dc,
                          double *x, double *r, struct lsb_mrhs_state *st, int parity, const double *pq_parts,
                          unsigned npq, double *partials2, unsigned *npartials, void *stream);
void lsb_k_mrhs_update_p(unsigned kp, unsigned n, const double *r, const double *dinv, double dc, double *p,
                         struct lsb_mrhs_state *st, int parity, const double *parts2, unsigned nparts2,
                         void *stream);
/* opts.verify, behind the SpMM with bres = b: the in-place restart of the columns whose recomputed residual
 * misses the tolerance (more == 0: they become MAXIT instead) */
void lsb_k_mrhs_restart(unsigned kp, unsigned n, const double *q, const double *dinv, double dc, double *r,
                        double *p, const struct lsb_mrhs_state *st, const double *rr_parts, unsigned nrr, int more,
                        double *partials, unsigned *npartials, void *stream);
void lsb_k_mrhs_restart_state(unsigned kp, struct lsb_mrhs_state *st, const double *rr_parts, unsigned nrr,
                              const double *rz_parts, unsigned nrz, int more, void *stream);
/* The same sweeps with z as a block of its own, written by a V-cycle on blocks (hip_mrhs_amg.hip) between them.
 * records (r_c . z_c, then r_c . r_c) of a one-level hierarchy, which has no sweep to leave them; st: a no-op
 * once st->running == 0 (NULL: always run) */
void lsb_k_amg_dot2_m(unsigned kp, unsigned n, const double *r, const double *z, double *records,
                      unsigned *nrecords, const struct lsb_mrhs_state *st, void *stream);
/* x = 0, r = b ; behind the cycle on r: p = z and the records (b.z, b.b) for lsb_k_mrhs_init_state */
void lsb_k_amg_mrhs_init(unsigned kp, unsigned n, const double *b, double *x, double *r, void *stream);
void lsb_k_amg_mrhs_init_p(unsigned kp, unsigned n, const double *b, const double *z, double *p, double *partials2,
                           unsigned *npartials, void *stream);
/* lsb_k_mrhs_update_xr without dot products of its own ; p = z + beta p with the stop test on the cycle's records */
void lsb_k_amg_mrhs_update_xr(unsigned kp, unsigned n, const double *p, const double *q, double *x, double *r,
                              struct lsb_mrhs_state *st, int parity, const double *pq_parts, unsigned npq,
                              void *stream);
void lsb_k_amg_mrhs_update_p(unsigned kp, unsigned n, const double *z, double *p, struct lsb_mrhs_state *st,
                             int parity, const double *parts2, unsigned nparts2, void *stream);
/* opts.verify: r = q, then (behind the cycle) p = z and the records of r.z, for the restarting columns only */
void lsb_k_amg_mrhs_restart_r(unsigned kp, unsigned n, const double *q, double *r, const struct lsb_mrhs_state *st,
                              const double *rr_parts, unsigned nrr, int more, void *stream);
void lsb_k_amg_mrhs_restart_p(unsigned kp, unsigned n, const double *r, const double *z, double *p,
                              const struct lsb_mrhs_state *st, const double *rr_parts, unsigned nrr, int more,
                              double *partials, unsigned *npartials, void *stream);
/* FSAI on blocks (hip_mrhs_fsai.hip), between lsb_k_spmm_csr and lsb_k_amg_mrhs_update_p: G and G^T as CSR, `lanes`
 * per row.  xr_gr: alpha_c from the SpMM's records (lsb_k_mrhs_update_xr's decisions; alpha_c left in the column's
 * alpha[parity]), x += alpha p, t = G (r - alpha q) -- r is only read.  gt_dots: z = G^T t, r -= alpha q in place on
 * the own rows, one record per workgroup of (r_c . z_c, then r_c . r_c); a no-op once st->running == 0. */
void lsb_k_mrhs_fsai_xr_gr(unsigned kp, unsigned n, const int *goffs, const int *gcols, const double *gvals,
                           unsigned lanes, const double *p, const double *q, double *x, const double *r, double *t,
                           struct lsb_mrhs_state *st, int parity, const double *pq_parts, unsigned npq, void *stream);
void lsb_k_mrhs_fsai_gt_dots(unsigned kp, unsigned n, const int *offs, const int *cols, const double *vals,
                             unsigned lanes, const double *t, const double *q, double *r, double *z, double *records,
                             unsigned *nrecords, const struct lsb_mrhs_state *st, int parity, void *stream);

/* ---- block-CG proper (hip_bcg.hip; driver: hip_bcg_drv.c) ----------------------------------------------------
 * One Krylov space for the kp = 2, 4 or 8 columns of an interleaved block (layout, pack / unpack: hip_mrhs.hip's).
 * The device state is lsb_blockcg_state (lsb_bcg_state is BiCGSTAB's): the small matrices are row-major with stride
 * LSB_MRHS_MAX whatever kp, the identity on the rows and columns >= nrhs.  Only the single-workgroup launches
 * (lsb_k_blockcg_small) write it; the SpMM gates on `running`, the two passes return at once where it is 0. */
struct lsb_blockcg_state {
  double xi[LSB_MRHS_MAX * LSB_MRHS_MAX];    /* Gamma^-1, Gamma = P^T S P */
  double xs[LSB_MRHS_MAX * LSB_MRHS_MAX];    /* xi sigma: X += P xs */
  double zeta[LSB_MRHS_MAX * LSB_MRHS_MAX];  /* L^T of G = W~^T D^-1 W~ = L L^T (upper triangular) */
  double zinv[LSB_MRHS_MAX * LSB_MRHS_MAX];  /* zeta^-1 (upper triangular); at the start: sigma^-1 */
  double sigma[LSB_MRHS_MAX * LSB_MRHS_MAX]; /* R = W sigma (upper triangular) */
  double rr[LSB_MRHS_MAX], bb[LSB_MRHS_MAX], thresh2[LSB_MRHS_MAX]; /* ||r_c||^2, ||b_c||^2, tol^2 ||b_c||^2 */
  double true_relres[LSB_MRHS_MAX];          /* opts.verify: ||b_c - S x_c|| / ||b_c||, -1: none */
  double tol;
  double min_pivot;                          /* smallest pivot of the unit-diagonal Gram matrix of the start */
  int status[LSB_MRHS_MAX];                  /* LSB_STATUS_*, per column; columns >= nrhs: CONVERGED */
  int iters, maxit, nrhs;
  int running;                               /* the SpMM's gate */
  int nspmm;                                 /* SpMM launches that did work */
  int rank_bad;                              /* the start found the block rank-deficient */
};
enum { LSB_BLOCKCG_START, LSB_BLOCKCG_GAMMA, LSB_BLOCKCG_G, LSB_BLOCKCG_VERIFY }; /* lsb_k_blockcg_small's phase */
/* records a launch leaves, one per workgroup: the upper triangle row by row, kp (kp + 1) / 2 doubles */
unsigned lsb_k_blockcg_tri(unsigned kp);
/* records of (B^T D^-1 B, then b_c . b_c per column): tri + kp doubles each */
void lsb_k_blockcg_init(unsigned kp, unsigned n, const double *b, const double *dinv, double dc, double *records,
                        unsigned *nrecords, void *stream);
/* one workgroup: re-reduces the records of the launch in front of it in a fixed order, does the kp x kp algebra of
 * its phase and the stop / breakdown / maxit decision, writes the state.  START: records of lsb_k_blockcg_init (tol,
 * maxit, nrhs are read in this phase only); GAMMA: of the SpMM; G: of pass A (G then H); VERIFY: of the residual
 * SpMM (lsb_k_spmm_csr, kp doubles each) */
void lsb_k_blockcg_small(unsigned kp, int phase, struct lsb_blockcg_state *st, const double *records,
                         unsigned nrecords, unsigned nrhs, double tol, int maxit, void *stream);
/* W = B sigma^-1, P = D^-1 W, X = 0 (not gated) */
void lsb_k_blockcg_start(unsigned kp, unsigned n, const double *b, const double *dinv, double dc, double *w, double *p,
                         double *x, const struct lsb_blockcg_state *st, void *stream);
/* Q = S P with lsb_k_spmm_csr's row and rounding rule, and the records of the upper triangle of P^T Q */
void lsb_k_blockcg_spmm(unsigned kp, unsigned n, const int *offs, const int *cols, const double *vals, unsigned lanes,
                        const double *p, double *q, double *records, unsigned *nrecords,
                        const struct lsb_blockcg_state *st, void *stream);
/* X += P xs ; W~ = W - Q xi in place ; records of the upper triangles of W~^T D^-1 W~ and of W~^T W~ */
void lsb_k_blockcg_pass_a(unsigned kp, unsigned n, double *w, const double *q, const double *p, double *x,
                          const double *dinv, double dc, const struct lsb_blockcg_state *st, double *records,
                          unsigned *nrecords, void *stream);
/* W = W~ zeta^-1 ; P = D^-1 W + P zeta^T */
void lsb_k_blockcg_pass_b(unsigned kp, unsigned n, double *w, double *p, const double *dinv, double dc,
                          const struct lsb_blockcg_state *st, void *stream);
/* ... under a preconditioner that is an operator (hip_bcg_m.hip): Z = M^-1 (.) is a block of its own.  The state, the
 * SpMM and lsb_k_blockcg_small are the ones above; zeta is then L^T of G = W~^T M^-1 W~.
 * X += P xs ; W~ = W - Q xi in place ; no records */
void lsb_k_blockcg_m_pass_a(unsigned kp, unsigned n, double *w, const double *q, const double *p, double *x,
                            const struct lsb_blockcg_state *st, void *stream);
/* records of two blocks of the same rows, <= LSB_STREAM_GRID_CAP of them.  start: the upper triangle of A^T Z, then
 * a_c . a_c (lsb_k_blockcg_init's layout, tri + kp doubles; not gated, st is not read); else the upper triangles of
 * A^T Z and of A^T A (pass A's layout, 2 tri doubles) */
void lsb_k_blockcg_m_gram(unsigned kp, int start, unsigned n, const double *a, const double *z, double *records,
                          unsigned *nrecords, const struct lsb_blockcg_state *st, void *stream);
/* Z = G^T T with lsb_k_spmm_csr's row and rounding rule (offs, cols, vals: the CSR of G^T) and the records of the
 * upper triangles of W~^T Z and of W~^T W~ in pass A's layout, one per workgroup of the SpMM's grid
 * (<= LSB_MAX_PARTIALS) */
void lsb_k_blockcg_m_gt_gram(unsigned kp, unsigned n, const int *offs, const int *cols, const double *vals,
                             unsigned lanes, const double *t, const double *wt, double *z, double *records,
                             unsigned *nrecords, const struct lsb_blockcg_state *st, void *stream);
/* W = B sigma^-1, P = Z sigma^-1, X = 0 (not gated) */
void lsb_k_blockcg_m_start(unsigned kp, unsigned n, const double *b, const double *z, double *w, double *p, double *x,
                           const struct lsb_blockcg_state *st, void *stream);
/* W = W~ zeta^-1 ; P = Z~ zeta^-1 + P zeta^T */
void lsb_k_blockcg_m_pass_b(unsigned kp, unsigned n, double *w, const double *z, double *p,
                            const struct lsb_blockcg_state *st, void *stream);

/* ---- the direct solver's factor on the device (hip_direct_t.hip, hip_direct_tm.hip; launchers in hip_solver.h) ----
 * struct lsb_tierinv on the device; one tier is the single skyline, and the coupling's pointers are then NULL.  How
 * k_dirt_rows deals the skyline rows: grp[2 g] = first row of group g, grp[2 g + 1] = rows << 8 | lanes per row;
 * blk[w] .. blk[w + 1]: the groups of workgroup w; bwin[2 w], bwin[2 w + 1]: first column and width of the window
 * of its operand its rows read.  Dealt tier by tier: tier t's workgroups are blk0 .. blk0 + nblk - 1 and stage
 * lds_doubles at the most.  cgrp / tgrp: the rows of C and of C^T in
 * groups of the same shape (first row, rows << 8 | lanes per row), tier t's at cg0 .. cg1 - 1 and tg0 .. tg1 - 1;
 * tbase: where tier t's offsets begin in toffs.  lds_m: the widest window, in rows, that the tier's launch on a block
 * of 2, 4, 8 right-hand sides stages (hip_direct_tm.hip). */
struct lsb_dirt_tier {
  unsigned lo, hi, blk0, nblk, lds_doubles, cg0, cg1, tg0, tg1, tbase, lds_m[3];
};
struct lsb_dirt_dev {
  unsigned n, ntier;
  const double *vals, *cvals, *tvals;
  const unsigned long long *woff;
  const unsigned *first, *perm, *parent, *run_end, *grp, *blk, *bwin;
  const unsigned *coffs, *ccols, *toffs, *tcols, *cgrp, *tgrp;
  struct lsb_dirt_tier t[LSB_DIRECT_MAX_TIERS];
};

/* ---- preconditioners with z as a vector (hip_precond_k.hip) -------------------- */
void lsb_k_dot2(unsigned n, const double *r, const double *z, double *partials2,
                unsigned *npartials, const struct lsb_pcg_state *st, void *stream);
void lsb_k_cheb_first(unsigned n, const double *r, const double *dinv, double dc, double c0,
                      double *d, double *z, const struct lsb_pcg_state *st, void *stream);
void lsb_k_cheb_step(unsigned n, const double *r, const double *w, const double *dinv, double dc,
                     double a, double b, double *d, double *z, const struct lsb_pcg_state *st,
                     void *stream);
void lsb_k_scale_dinv(unsigned n, double c, const double *dinv, const double *w, double *v,
                      void *stream);
void lsb_k_scale_vec(unsigned n, double c, double *v, void *stream);
void lsb_k_power_start(unsigned n, unsigned first, double *v, void *stream);
void lsb_k_bj_invert(unsigned n, unsigned bs, double *binv, double *scratch, void *stream);
void lsb_k_bj_apply(unsigned n, unsigned bs, const double *binv, const double *r, double *z,
                    double *part, const struct lsb_pcg_state *st, const double *skip2,
                    unsigned nskip, void *stream);
unsigned lsb_k_bj_chunks(unsigned bs);

/* ---- one-launch solve of launch-bound operators (hip_persist.hip) ------------ */
size_t lsb_k_persist_shared_bytes(void);
unsigned lsb_k_persist_limits(unsigned *nzmax, unsigned *rmax, unsigned *gmax);
int lsb_k_pcg_persist(unsigned n, unsigned G, unsigned stride, const unsigned *wg_row,
                      const int *offs, const int *cols, const double *vals, const double *dinv,
                      const double *b, double *x, double *ug, void *shared,
                      struct lsb_pcg_state *st, double tol, int maxit, unsigned lanes,
                      long long timeout_ticks, void *stream);

/* ---- direct xGMI path (hip_p2p.hip) ---------------------------------------- */
struct lsb_p2p;
struct lsb_p2p *lsb_p2p_create_dist(const struct lsb_xfer *recv, int nrecv,
                                    const struct lsb_xfer *send, int nsend);
int lsb_p2p_create_virtual(struct lsb_p2p **out, int n, struct lsb_xfer *const *recv,
                           const int *nrecv, struct lsb_xfer *const *send, const int *nsend);
void lsb_p2p_destroy(struct lsb_p2p *p);
int lsb_p2p_has_halo(const struct lsb_p2p *p);
void lsb_p2p_send(struct lsb_p2p *p, const double *d_full, const struct lsb_pcg_state *st,
                  void *stream);
void lsb_p2p_recv(struct lsb_p2p *p, double *d_full, struct lsb_pcg_state *st, void *stream);
void lsb_p2p_sendrecv(struct lsb_p2p *p, double *d_full, struct lsb_pcg_state *st, void *stream);
void lsb_p2p_allreduce(struct lsb_p2p *p, const double *parts, unsigned nparts, unsigned width,
                       const double *parts2, unsigned nparts2, unsigned width2,
                       const double *extra, unsigned nextra, double *out,
                       struct lsb_pcg_state *st, int phases, void *stream);
void lsb_p2p_fold_contribute(struct lsb_p2p *p, struct lsb_ar_tail *t);
void lsb_p2p_fold_collect(const struct lsb_p2p *p, struct lsb_ar_collect *c);
void lsb_p2p_test_collect_check(struct lsb_p2p *p, unsigned round, unsigned *d_bad,
                                struct lsb_pcg_state *st, void *stream);
void lsb_p2p_test_pattern(double *d_full, size_t goff, size_t n, unsigned round, void *stream);
void lsb_p2p_test_check_range(const double *d_full, size_t goff, size_t n, unsigned round,
                              unsigned *d_bad, void *stream);
void lsb_p2p_test_setvals(double *d_v, int me, unsigned round, void *stream);
void lsb_p2p_test_checkvals(const double *d_v, int R, unsigned round, unsigned *d_bad,
                            void *stream);

/* ---- smoothed-aggregation AMG V-cycle (hip_amg.hip; set-up lsb_amg.c, hip_amg_drv.c) ----
 * One level as the kernels see it.  A CSR of the level: int offsets and columns (all < 2^31),
 * `lanes` per row (2..64, from the mean row length), `rows` of them. */
struct lsb_amg_mat {
  const int *offs, *cols;
  const double *vals;
  unsigned rows, lanes;
};
/* its sibling in the fp32 hierarchy (hip_amg_f32.hip): one packed {column, float} word per stored entry
 * (lsb_csr_pack_f32).  A struct of its own: k_amg_tail reads lsb_amg_mat's layout from the device. */
struct amg_mat32 {
  const int *offs;
  const unsigned long long *ent;
  unsigned rows, lanes;
};
/* a level as k_amg_tail reads it from the device, and nothing more (the host's description: hip_solver.h) */
struct lsb_amg_lvdev {
  unsigned n, pad_;
  struct lsb_amg_mat A, P, R; /* P: n rows, R: the next level's n rows (none on the coarsest) */
  const double *minv;         /* 1 / sum_j |a_ij|: the l1-Jacobi smoother (the Chebyshev smoother: 1 / a_ii) */
  double *b, *out;            /* the level's right-hand side and correction (level 0: the caller's) */
  double *tmp, *r;            /* the other smoothing buffer, the residual */
};
enum { LSB_AMG_SWEEP = 1, /* y = x + M^-1 (b - A x), out of place                 */
       LSB_AMG_RESID = 2, /* r = b - A x                                           */
       LSB_AMG_SPMV = 3,  /* y = M x for a rectangular M (the restriction R r)      */
       LSB_AMG_ADDP = 4 };/* x += P e, in place (row i reads x_i only)              */
void lsb_k_amg_first(unsigned n, const double *b, const double *minv, double *x,
                     const struct lsb_pcg_state *st, void *stream);
void lsb_k_amg_csr(int mode, const struct lsb_amg_mat *m, const double *xin, const double *b, const double *minv,
                   double *y, const struct lsb_pcg_state *st, void *stream);
void lsb_k_amg_dense(unsigned nc, unsigned lanes, const double *cinv, const double *b, double *out,
                     const struct lsb_pcg_state *st, void *stream);
/* the Chebyshev smoother (LSB_AMG_SMOOTH_CHEB): step 0 from the zero guess, d = (c2 dinv) b, x = d ; a step
 * with the matrix, d <- c1 d + c2 dinv (b - A xin) in place (not read when c1 == 0), y = xin + d */
void lsb_k_amg_cheb_first(unsigned n, const double *b, const double *dinv, double c2, double *d, double *x,
                          const struct lsb_pcg_state *st, void *stream);
void lsb_k_amg_cheb(const struct lsb_amg_mat *m, const double *xin, const double *b, const double *dinv, double c1,
                    double c2, double *d, double *y, const struct lsb_pcg_state *st, void *stream);
/* levels t .. nlev - 1 of the V-cycle and the coarse solve in one launch of one 1024-thread
 * workgroup; lv = the device copy of all levels' descriptors; b0 / out0 stand in for level 0's */
void lsb_k_amg_tail(const struct lsb_amg_lvdev *lv, unsigned t, unsigned nlev, unsigned nu, const double *cinv,
                    unsigned nc, unsigned clanes, const double *b0, double *out0, const struct lsb_pcg_state *st,
                    void *stream);

/* ---- the V-cycle on blocks of kp = 2, 4 or 8 columns (hip_mrhs_amg.hip; the PCG sweeps around it: hip_mrhs.hip) ----
 * Interleaved blocks as hip_mrhs.hip's on every level; each column's arithmetic is the single-column kernels'
 * (lsb_k_amg_first / _csr / _dense), so a column has their bits.  st: a no-op once st->running == 0 (NULL:
 * always run); never written.  records (LSB_AMG_SWEEP only, may be NULL): one record per workgroup of
 * 2 kp doubles, b_c . y_c per column then b_c . b_c per column; *nrecords of them (<= LSB_MAX_PARTIALS). */
void lsb_k_amg_first_m(unsigned kp, unsigned n, const double *b, const double *minv, double *x,
                       const struct lsb_mrhs_state *st, void *stream);
void lsb_k_amg_csr_m(unsigned kp, int mode, const struct lsb_amg_mat *m, const double *xin, const double *b,
                     const double *minv, double *y, double *records, unsigned *nrecords,
                     const struct lsb_mrhs_state *st, void *stream);
void lsb_k_amg_dense_m(unsigned kp, unsigned nc, unsigned lanes, const double *cinv, const double *b, double *out,
                       const struct lsb_mrhs_state *st, void *stream);

/* ---- the Chebyshev smoother on blocks of kp columns (hip_amg_cheb.hip): lsb_k_amg_cheb_first / lsb_k_amg_cheb
 * per column, bit for bit; d is a block as x is.  records / nrecords as lsb_k_amg_csr_m's sweep leaves them. */
void lsb_k_amg_cheb_first_m(unsigned kp, unsigned n, const double *b, const double *dinv, double c2, double *d,
                            double *x, const struct lsb_mrhs_state *st, void *stream);
void lsb_k_amg_cheb_m(unsigned kp, const struct lsb_amg_mat *m, const double *xin, const double *b,
                      const double *dinv, double c1, double c2, double *d, double *y, double *records,
                      unsigned *nrecords, const struct lsb_mrhs_state *st, void *stream);

/* ---- the fp32 V-cycle (hip_amg_f32.hip).  Modes, lanes, grids and the gate `st` as hip_amg.hip's launchers.
 * in64: b is the caller's fp64 r, rounded once, the copy stored in b32 (else b is float and b32 unused);
 * y64 != NULL: the result goes there widened to double instead of to y (sweeps and Chebyshev steps only);
 * ends64: a one-level hierarchy's coarse solve, fp64 r to fp64 z. */
void lsb_k_amg32_first(unsigned n, int in64, const void *b, const float *minv, float *x, float *b32,
                       const struct lsb_pcg_state *st, void *stream);
void lsb_k_amg32_csr(int mode, const struct amg_mat32 *m, const float *xin, const float *b, const float *minv,
                     float *y, double *y64, const struct lsb_pcg_state *st, void *stream);
void lsb_k_amg32_cheb_first(unsigned n, int in64, const void *b, const float *dinv, float c2, float *d, float *x,
                            float *b32, const struct lsb_pcg_state *st, void *stream);
void lsb_k_amg32_cheb(const struct amg_mat32 *m, const float *xin, const float *b, const float *dinv, float c1,
                      float c2, float *d, float *y, double *y64, const struct lsb_pcg_state *st, void *stream);
void lsb_k_amg32_dense(unsigned nc, unsigned lanes, int ends64, const float *cinv, const void *b, void *out,
                       const struct lsb_pcg_state *st, void *stream);

/* ---- multicolour Gauss-Seidel smoothing (hip_amg_mcgs.hip; LSB_AMG_SMOOTH_MCGS).  m: the colour-sorted copy of the
 * level's matrix (lsb_csr_mcgs; its lanes are the level's), rowid: position -> row, [p0, p1): one colour's range of
 * positions.  One launch is one colour step in place: x_i <- fma(dinv_i, b_i - (row i) . x, x_i) on the rows of that
 * colour.  _first: the first launch from the zero guess, over all n rows -- x_i = fma(dinv_i, b_i, 0) where
 * colour[i] == 0, else 0; in64 / b32 as lsb_k_amg32_first.  z64 != NULL: the float result goes to x AND, widened, to
 * z64.  The gate `st` as hip_amg.hip's launchers. */
void lsb_k_amg_mcgs_first(unsigned n, const unsigned char *colour, const double *b, const double *dinv, double *x,
                          const struct lsb_pcg_state *st, void *stream);
void lsb_k_amg_mcgs(const struct lsb_amg_mat *m, const int *rowid, unsigned p0, unsigned p1, double *x,
                    const double *b, const double *dinv, const struct lsb_pcg_state *st, void *stream);
void lsb_k_amg32_mcgs_first(unsigned n, int in64, const unsigned char *colour, const void *b, const float *dinv,
                            float *x, float *b32, const struct lsb_pcg_state *st, void *stream);
void lsb_k_amg32_mcgs(const struct amg_mat32 *m, const int *rowid, unsigned p0, unsigned p1, float *x, const float *b,
                      const float *dinv, double *z64, const struct lsb_pcg_state *st, void *stream);

/* ---- geometric multigrid on grids (lsb_gmg.c, hip_gmg.hip; LSB_PRECOND_GMG) ----
 * the rest of the host logic: why lsb_gmg_detect refused; the 2^dim diagonals D and smoothing weights w = omega / D of
 * a level, indexed by the mask of far faces a point lies on (bit d: i_d == n_d - 1); the level's operator as a CSR;
 * AMG's dense inverse of a coarsest operator (lsb_amg.c), who = the option its messages name, what = the inverse
 * as its out-of-memory message calls it */
const char *lsb_gmg_why(int rc);
void lsb_gmg_diagonals(unsigned dim, double c, const double delta[3], double D[8], double w[8]);
struct csr *lsb_gmg_level_csr(unsigned dim, double c, const struct lsb_gmg_level *lv);
double *lsb_amg_coarse_inverse(const struct csr *A, const char *who, const char *what);
/* A level as the kernels take it, by value: its points n and the next level's nc per dimension (1 beyond the grid's),
 * the doubles between grid lines (n[0], or more on a line-padded fine level: the lanes i >= n[0] of a line write 0),
 * c, sigma, per dimension what the last fine point of an odd n takes of the last coarse one, delta / (1 + delta), and
 * the diagonals and weights by far-face mask.  Point (i, j, k) is element (k n[1] + j) pitch + i. */
struct lsb_gmg_lv {
  unsigned n[3], pitch;
  unsigned nc[3], pad_;
  double c, sigma, wlast[3];
  double D[8], w[8];
};
/* The steps of the cycle on one level, dim = 2 or 3.  first: x = w b.  sweep: y = x + w (b - A x), out of place.
 * restrict: bc = sigma P^T (b - A x), a coarse point forms the 3^dim fine residuals it needs.  prolong: x += P xc.
 * down = first and restrict in one launch (the residual of x = w b needs only b): writes x and bc.  up = prolong and
 * one sweep: y = u + w (b - A u), u = x + P xc on a tile with a one-point halo in LDS.  Each step's arithmetic is one
 * device function shared by the plain and the fused kernel: the two paths give the same bits.  The gate `st` as
 * hip_amg.hip's launchers. */
void lsb_k_gmg_first(unsigned dim, const struct lsb_gmg_lv *lv, const double *b, double *x,
                     const struct lsb_pcg_state *st, void *stream);
void lsb_k_gmg_sweep(unsigned dim, const struct lsb_gmg_lv *lv, const double *xin, const double *b, double *y,
                     const struct lsb_pcg_state *st, void *stream);
void lsb_k_gmg_restrict(unsigned dim, const struct lsb_gmg_lv *lv, const double *x, const double *b, double *bc,
                        const struct lsb_pcg_state *st, void *stream);
void lsb_k_gmg_prolong(unsigned dim, const struct lsb_gmg_lv *lv, double *x, const double *xc,
                       const struct lsb_pcg_state *st, void *stream);
void lsb_k_gmg_down(unsigned dim, const struct lsb_gmg_lv *lv, const double *b, double *x, double *bc,
                    const struct lsb_pcg_state *st, void *stream);
void lsb_k_gmg_up(unsigned dim, const struct lsb_gmg_lv *lv, const double *x, const double *b, const double *xc,
                  double *y, const struct lsb_pcg_state *st, void *stream);

/* ---- backend internals shared between hip_cdna4.c and hip_comm.c -------- */
void *lsb_hip_stream(void);
int lsb_hip_is_initialized(void);
/* grouped point-to-point exchange of contiguous ranges of a device vector */
int lsb_hip_comm_exchange(double *d_full, const struct lsb_xfer *sends,
                          int nsend, const struct lsb_xfer *recvs, int nrecv,
                          void *stream);
int lsb_hip_comm_allgather_u32(const unsigned *mine, unsigned count,
                               unsigned *all);
int lsb_hip_comm_allreduce_stream(double *d_buf, int count, void *stream);

#define LSB_CHK_HIP(call)                                                      \
  do {                                                                         \
    hipError_t e_ = (call);                                                    \
    if (e_ != hipSuccess)                                                      \
      errx(EXIT_FAILURE, "%s:%d hip error: %s", __FILE__, __LINE__,            \
           hipGetErrorString(e_));                                             \
  } while (0)

#ifdef __cplusplus
}
#endif
#endif
