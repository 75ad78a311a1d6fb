/*
 * Internals of the solver object shared by the host-side C files of the HIP
 * backend:
 *   hip_cdna4.c      backend entry points (init / finalize / bench), options,
 *                    device memory helpers, kernel-level C-ABI
 *   hip_solver.c     shards: one builder and one free per SpMV layout, upload, kernel forms,
 *                    timing pass, create / destroy
 *   hip_dist.c       what sharded solves add: exchange, all-reduce, overlap,
 *                    the direct xGMI path's set-up
 *   hip_run.c        what the iteration drivers share: the host loop, the cache of captured graphs, the chunk rule
 *   hip_pcg.c        the PCG driver: its iteration forms (one chosen per solver), one run, the persistent launch
 *   hip_solve.c      what a caller's solve is, whichever driver runs it (one chosen per solver): cold and from an
 *                    initial guess, recomputed residuals and what follows from them, the single-column entry points
 *   hip_seq_drv.c    successive right-hand sides: the basis of earlier solutions a solver keeps when asked, the
 *                    projection in front of a solve and the update behind it
 *   hip_precond.c    FSAI, block-Jacobi and the Chebyshev preconditioner: set-up and z = M^-1 r
 *   hip_amg_drv.c    AMG: upload of the hierarchy, the V-cycle's one schedule (amg_cycle), its accessors
 *   hip_gmres_drv.c  GMRES(m) driver
 *   hip_bicgstab_drv.c  BiCGSTAB driver
 *   hip_rich_drv.c   AMG as the solver: stationary V-cycle iterations (Richardson)
 *   hip_direct_drv.c the direct solver: factor at creation, rounds of x (+)= L^-T L^-1 r on an inverse factor in tiers
 *                    (one tier: the single skyline W = L^-1; more for operators whose single skyline is over the budget)
 *   hip_direct_m_drv.c  ... on blocks of right-hand sides: the factor streamed once per product for a block of columns
 *   hip_rich_m_drv.c ... AMG as the solver on blocks of right-hand sides: the hierarchy streamed once per cycle
 *   hip_block.c      interleaved blocks of right-hand sides, what their two drivers share: the service rules, the work
 *                    area (struct block_work), Z = M^-1 R on a block, the enqueue and host-buffer wrappers
 *   hip_mrhs_drv.c   several right-hand sides: independent PCG recurrences (Jacobi, AMG, FSAI) on a CSR SpMM
 *   hip_bcg_drv.c    block-CG proper: one Krylov space for a block of right-hand sides (second half: under FSAI and AMG)
 * Nothing here is part of the C-ABI (include/lsbench_hip.h).
 */
#ifndef HIP_SOLVER_H
#define HIP_SOLVER_H

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stddef.h>
#include <string.h>
#include <strings.h>
#include <time.h>

#include "lsb_impl.h"

#define LSB_INTERNAL __attribute__((visibility("hidden")))

/* backend globals (defined in hip_cdna4.c; reference style, src/cusparse.c:33-36) */
/* The streams, the communicator (hip_comm.c) and the last result are per host
 * THREAD: a rank is a thread -- the caller's own when there is one GPU or one
 * process per GPU, one of hip_multi.c's workers when hip_cdna4_bench drives
 * several GPUs from the one caller process. */
extern LSB_INTERNAL int lsb_initialized;
extern LSB_INTERNAL __thread hipStream_t g_stream; /* compute */
extern LSB_INTERNAL __thread struct lsb_hip_result g_last;
LSB_INTERNAL hipStream_t comm_stream(void); /* halo exchange behind interior rows; made on first use */
LSB_INTERNAL void rank_thread_attach(int device);
LSB_INTERNAL void rank_thread_detach(void);
/* hip_multi.c */
LSB_INTERNAL int bench_multi(double *x, struct csr *A, const double *r, const struct lsbench *cb,
                             const struct lsb_hip_opts *o, int ngpus);

/* ------------------------------------------------------------------------ */
/* solver object                                                             */
/* ------------------------------------------------------------------------ */
#define SCAL_STRIDE 8 /* doubles per shard in the scalar slab */
#define MAX_SAMPLES 64
#define LSB_NGRAPH 4 /* cached hipGraphs: whole-solve + continuation chunk, solve proper + correction */

/* hipGraphs of `count` iterations each, found by (count, key) and replaced round-robin (hip_run.c: graph_launch,
 * graph_drop).  key: the caller's x where the launches hold it, NULL where they touch internal buffers only */
struct graph_cache {
  struct {
    hipGraphExec_t exec;
    int count;
    const void *key;
  } e[LSB_NGRAPH];
  int next;
};

/* What a work area on interleaved blocks of kp right-hand sides has in common, whichever driver owns it (hip_block.c:
 * block_work_slab, block_work_z, block_work_free; the owners: struct mrhs_work, struct blockcg_work) */
struct amg_vecs;
struct block_work {
  unsigned kp;           /* 0: not allocated */
  char *mem;             /* the slab: the five blocks, then z and t where it holds them, then the owner's records and
                            state */
  double *b, *x, *p, *q; /* n kp doubles each */
  union {
    double *r; /* the residual block of independent recurrences */
    double *w; /* block-CG: the factor W of R = W sigma */
  };
  /* z = M^-1 (.) as a block of its own, and what forming it needs.  FSAI: z and t = G (.) are two blocks, of the slab
   * or -- block_work_z -- of zmem.  AMG: z is the head of amg_mem, the cycle's vectors of every level at this width
   * (amg_block_vecs, av; level 0: b and out are the r and z of the call; the fp32 cycle: amg_block_vecs32, float
   * blocks on every level behind the fp64 z). */
  double *z, *t;
  char *zmem, *amg_mem;
  struct amg_vecs *av;
  struct graph_cache g; /* keyed on the count: the iteration touches these buffers only */
};

/* Rows that reference other shards' columns sit in units [0,first) and [last,count) of a layout (row
 * blocks, slices); the units in between can start before the halo has arrived (ok = 0: not separable) */
struct halo_split {
  unsigned first, last;
  int ok;
};
/* the sliced-ELL kernel a shard's SpMV runs (tune_spmv resolves it from the variant, the flags and the
 * copies that exist; sell_launch, the getters, the fused PCG and Chebyshev forms read it) */
enum { SELL_NONE, SELL_32, SELL_16, SELL_TMPL, SELL_COL };
/* the PCG iteration a solver runs (pcg_choose_form picks it once, at creation; hip_pcg.c) */
enum pcg_form {
  PCG_NONE,    /* GMRES, BiCGSTAB, Richardson, the direct solver: no PCG iteration */
  PCG_CLASSIC, /* SpMV, k_pcg_update_xr, k_pcg_update_p (one shard or many) */
  PCG_SUBWAVE, /* k_spmv_subwave_p + k_pcg_update_xr: the direction update rides in the next SpMV */
  PCG_COL,     /* k_pcg_col_px + k_pcg_col_r on the z-column plan (+ k_pcg_xfix at a run's end) */
  PCG_CG1,     /* single reduction: k_cg1_update + SpMV */
  PCG_GENERIC, /* the classic sweeps around precond_apply (z = M^-1 r as a vector) */
  PCG_FSAI3,   /* FSAI in three launches: k_spmv_subwave_p, k_fsai_xr_gr, k_fsai_gt_dots */
};

/* An iteration driver (solve_driver_for picks it once, at creation; hip_solve.c).  solve: one solve from x0 = 0 as the
 * caller sees it, to sv->tol_run and -- sv->verify_run -- checked against a recomputed residual.  run: one bare run
 * of the iteration, `round` = 0 for the solve proper, k for its k-th correction run; NULL: solve, with
 * sv->verify_run = 0, is that run */
typedef int solve_dev_fn(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res);
struct solve_driver {
  solve_dev_fn *solve;
  int (*run)(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res, int round);
};

/* The vectors of one level of the AMG V-cycle: right-hand side, result, the other smoothing buffer, the residual, the
 * Chebyshev smoother's direction (NULL under l1-Jacobi).  double in the fp64 cycle (one column: amg_dev.vec; blocks of
 * kp: block_work.av), float in the fp32 cycle.  Level 0 under fp64: b and out are NULL, the caller's r and z stand in.
 * A level smoothed by multicolour Gauss-Seidel keeps its iterate in out alone and does not touch tmp */
struct amg_vecs {
  void *b, *out, *tmp, *r, *d;
};

struct shard {
  /* ONE allocation for the vectors the iteration streams (r, q, the gather vector, the Jacobi
   * diagonal, the single-reduction form's p / s, the preconditioners' z vectors, the second direction
   * buffer of the fused-p forms and, for a padded or re-ordered one-shard solver, its x and b -- so
   * the two-launch form's r, p0, p1 and x are neighbours too; an unpadded solver's x is the caller's): their placement
   * relative to one another is then the same in every solver of every process -- which of their
   * lines compete for the same sets of the 256 MB Infinity Cache no longer depends on which
   * physical pages a dozen separate hipMallocs happened to get ("Where the
   * vectors land"); used where the vectors are of that cache's scale (<= 160 MB each: larger ones measured
   * slower out of one allocation).  shard_vec() carves 256-byte aligned pieces; what does not fit (or arrives with
   * LSBENCH_HIP_NO_SLAB=1) is a hipMalloc of its own; shard_vec_free() tells the two apart. */
  char *d_slab;
  size_t slab_cap, slab_used;
  int slab_bx; /* the slab also holds the solver's permuted x and b (one shard, padded or re-ordered): set by the
                  creator before shard_upload, which counts them; carved behind the shard's own vectors */
  unsigned row_begin, n;
  unsigned long long nnz;
  unsigned n_glob; /* columns of the operator = length of the gather vector */
  unsigned col_lo, col_hi; /* column hull referenced by the shard's rows */
  int variant, sell_form; /* LSB_SPMV_*; the sliced-ELL kernel it resolves to (SELL_*) */
  unsigned lanes;
  /* SpMV flavour, grid and (sliced-ELL) slices per plane the XCD dealing follows (0 = contiguous eighths),
   * picked by tune_spmv() */
  unsigned sp_flags, sp_grid, sp_period;
  /* opts.precision = LSB_PREC_MIXED: the SpMV forms stream fp32 values (the sliced-ELL value arrays then
   * HOLD floats; csr.vals32 is the CSR's copy); csr.vals stays fp64 for the residual of the refinement.
   * exact32: rounding changed nothing */
  int mixed, exact32;
  /* The SpMV layouts: one struct, one builder and one free each (hip_solver.c).  The CSR is always
   * there; the others are built where the operator qualifies, and tune_spmv() frees the ones that lose. */
  struct shard_csr { /* CSR + the row blocks of the adaptive kernel */
    int *offs, *cols, *rowblk;
    unsigned char *blklanes;
    double *vals;
    float *vals32;
    unsigned nblk;
    struct halo_split split; /* in row blocks */
  } csr;
  struct shard_panel { /* column-panel form (LSB_SPMV_PANEL), built when asked for */
    unsigned n;     /* panels, 0 = not built */
    unsigned *blk;  /* host, n+1: first row block of each panel */
    int *offs, *cols, *rowmap, *rowblk;
    unsigned char *blklanes;
    double *vals;
  } panel;
  struct shard_bins { /* binned form (LSB_SPMV_BINNED), built for scattered operators only */
    unsigned n, cap; /* bins (0 = not built), entries per chunk */
    unsigned *chunk_h; /* host, n+1: first chunk of each bin */
    unsigned *chunk, *rows, *cols;
    double *vals;
  } bins;
  struct shard_tp { /* two-phase form (LSB_SPMV_TWOPHASE), built for scattered operators only */
    unsigned items, bins, col_lo, xlen, cols, rows; /* bins = 0: not built */
    unsigned *item, *binptr, *first, *delta;
    unsigned long long *mask;
    unsigned short *colw, *roww;
    double *vals, *prod, *binparts;
  } tp;
  /* sliced-ELL (LSB_SPMV_SELL), built when padding stays under 1/8: the slice geometry every copy shares
   * and the 32-bit copy */
  struct shard_sell {
    unsigned nslice;
    unsigned period;         /* candidate period of the XCD dealing, found at upload (0: none) */
    struct halo_split split; /* in slices */
    unsigned *sptr;
    int *cols;
    double *vals;
    unsigned long long bytes; /* matrix-side bytes one launch streams */
  } sell;
  struct lsb_sell16_dev c16; /* its 16-bit-code form (LSB_SP_C16) and the templates (LSB_SP_TMPL) */
  /* z-column plan of the template layout (lsb_sell_tmpl_columns; LSB_SP_COL): xbeg[9], padding to 16
   * unsigneds, 16-byte items */
  struct shard_col {
    unsigned period;           /* slices per plane (a period of at least 8 slices; 0: no plan) */
    unsigned *plan, *plan_in;  /* all slices; the interior range of the split SpMV */
    unsigned items, items_in;
    int centre0;
    unsigned long long slices; /* slices inside columns */
    unsigned long long bytes;  /* matrix-side bytes one launch of the walk streams */
  } col;
  double *d_dinv, *d_r, *d_q, *d_pfull;
  /* the forms' own vectors (form_vecs): the second direction buffer of the fused and FSAI-3 forms, or the
   * single-reduction form's p (pfull then holds u); its s = S p */
  double *d_p1, *d_s1;
  unsigned npq, np2;   /* partial counts of the SpMV / sweep launches */
  const double *ar2_parts; /* sweep partials the next all-reduce folds in */
  unsigned ar2_n, ar2_width;
  struct lsb_cheb_epi epi; /* zout != NULL: the next 16-bit sliced-ELL launch of this shard carries a
                              Chebyshev step in its epilogue (precond_apply arms and clears it) */
  double *d_zfull2;        /* its second gather vector: z' of step k is step k+1's z */
  struct lsb_ar_tail tail; /* counter != NULL: the next SpMV launch of this shard carries the
                              all-reduce's contribute phase (exchange_and_spmv arms and clears it) */
  int dinv_uniform;   /* all entries of dinv equal dinv_const */
  double dinv_const;
  double *d_parts_pq, *d_parts2;
  double *d_scal; /* [0] p.q   [1] r.z'  [2] r.r   (multi-shard path) */
  struct lsb_pcg_state *d_st;
  /* status word for communication steps that belong to no running solve (the
   * SpMV entry point, the first all-reduce of a solve): a time-out of the direct
   * xGMI path is recorded here and reported by the host (check_aux_status) */
  struct lsb_pcg_state *d_st_aux;
  /* preconditioners that produce z = M^-1 r as a vector (hip_precond.c) */
  double *d_zfull, *d_z; /* z: a gather vector of its own (Chebyshev), or n doubles */
  double *d_chd;         /* Chebyshev: the recurrence's direction vector */
  double *d_binv, *d_bjpart; /* block-Jacobi: inverted diagonal blocks; chunk partial sums */
  unsigned bj_bs;
  /* FSAI (LSB_PRECOND_FSAI): G and G^T as CSR of their own, z = G^T (G r) through the row kernels */
  struct fsai_csr {
    int *offs, *cols, *rowblk;
    unsigned char *blklanes;
    double *vals;
    unsigned nblk, lanes;
    int variant;
    unsigned long long nnz;
  } fs_g, fs_gt;
  double *d_fst;     /* t = G r */
  double *d_r1;      /* the three-launch iteration's second residual buffer (form_vecs) */
  unsigned fs_maxrow; /* longest row of the pattern */
  /* AMG (PRECOND_AMG): the hierarchy on the device, z = one V-cycle (hip_amg_drv.c; hip_amg.hip, hip_amg_f32.hip) */
  struct amg_dev {
    unsigned nlev, tail, nu, nc, clanes; /* tail: first level of the one-launch tail (nlev: none) */
    int prec, cheb, mcgs;                /* LSB_AMG_PREC_*; opts.amg_smoother == LSB_AMG_SMOOTH_CHEB, == _MCGS */
    unsigned mcgs_cap;                   /* mcgs: a level of more colours keeps l1-Jacobi */
    unsigned long long mcgs_bytes;       /* mcgs: device bytes of the colour-sorted copies */
    /* a level, in the solver's precision: its matrices (.d fp64, .f fp32: packed entries), minv (double or float;
     * the Chebyshev smoother: 1 / a_ii) and, per smoothed level under that smoother, the interval of D^-1 A and
     * the coefficients of its nu steps (lsb_amg_cheb_coeffs; the fp32 launches round them) */
    struct amg_lv {
      unsigned n;
      union amg_mat {
        struct lsb_amg_mat d;
        struct amg_mat32 f;
      } A, P, R;
      const void *minv;
      double lo, hi, c1[16], c2[16];
      /* multicolour Gauss-Seidel (hip_amg_mcgs.hip): ncol > 0 on a level it smooths -- then minv holds 1 / a_ii, C is
       * the colour-sorted copy of A (lsb_csr_mcgs), rowid its position -> row, colour8 the colour of every row and
       * cbeg (host, ncol + 1) the colours' ranges of positions.  ncol_found: what the colouring gave, cap or not */
      unsigned ncol, ncol_found, *cbeg;
      union amg_mat C;
      const int *rowid;
      const unsigned char *colour8;
    } *lv;
    /* the single-column cycle's vectors.  Level 0's come out of the vector slab: under fp64 tmp and r; under fp32
     * the same two slab vectors split in halves -- tmp | out, and b (the fp32 copy of the caller's r) | r */
    struct amg_vecs *vec;
    struct lsb_amg_lvdev *d_lv;          /* fp64: the levels as k_amg_tail reads them */
    void *d_cinv;                        /* nc x nc coarse inverse, double or float */
    void **mem;                          /* every allocation of the hierarchy */
    unsigned nmem;
    double setup_s;
    /* what one cycle streams, for the poll interval of a batch of right-hand sides: the bytes of its matrices
     * and its vector passes in rows (summed over the levels) */
    unsigned long long cycle_mat_bytes, cycle_vec_rows;
    unsigned long long cycle_bytes32; /* what lsb_hip_solver_amg_cycle_bytes answers under fp32 */
  } *amg;
  /* Geometric multigrid (PRECOND_GMG; hip_gmg_drv.c, hip_gmg.hip).  gmg_grid / gmg_pitch: what the creator detected on
   * the operator before line padding and the pitch of its lines after it, handed over before shard_upload (dim = 0:
   * nothing was handed over -- a shard of a sharded solver).  gmg: the levels as the kernels take them, their vectors
   * (level 0: b and buf[1] are the caller's r and z, buf[0] comes out of the slab; below it one allocation, mem), the
   * coarsest level's dense inverse, and what a cycle streams */
  struct lsb_gmg_grid gmg_grid;
  unsigned gmg_pitch;
  struct gmg_dev {
    unsigned dim, nlev, nu, nc, clanes;
    int fused; /* nu == 1 and not LSBENCH_HIP_GMG_FUSE=0: k_gmg_down / k_gmg_up in the place of the plain steps */
    struct lsb_gmg_level plan[LSB_GMG_MAX_LEVELS];
    struct lsb_gmg_lv lv[LSB_GMG_MAX_LEVELS];
    double *b[LSB_GMG_MAX_LEVELS], *buf[LSB_GMG_MAX_LEVELS][2];
    double *mem, *d_cinv;
    unsigned long long cycle_bytes;
    double setup_s;
  } *gmg;
  struct lsb_xfer *recv, *send;
  int nrecv, nsend;
};

struct lsb_hip_solver {
  unsigned n_glob;   /* rows of the whole operator                         */
  unsigned n_here;   /* rows held by this process (sum over its shards)     */
  unsigned n_user;   /* ... as the caller counts them: n_here less the pad rows of a line-padded grid */
  int padded;        /* the operator was line-padded (lsb_csr_pad_lines): d_perm maps internal rows to the
                        caller's, -1 on pad rows */
  unsigned row_first; /* first row held by this process                     */
  int nshard;        /* shards in this process (1, or nvirt)                */
  int dist;          /* 1: shards of other processes exist (RCCL)           */
  int multi;         /* nshard > 1 || dist: scalars go through all-reduce   */
  struct shard *sh;
  double *d_scal_all; /* nshard * SCAL_STRIDE doubles                        */
  struct lsb_hip_opts o;
  struct lsb_pcg_state *h_st; /* pinned, 2 slots */
  struct graph_cache graphs; /* PCG's, keyed on the count and on x: the form a run takes depends on the solver and
                                x alone */
#define LSB_MAX_CORRECTIONS 6
#define LSB_MIXED_INNER_TOL 1e-5 /* what an inner solve on fp32-rounded values is asked for */
  unsigned hint_iters[LSB_MAX_CORRECTIONS + 1]; /* iterations of the previous solve and of each of
                                                   its correction runs, 0 = none yet */
  double tol_run;    /* tolerance of the run being enqueued, whichever the driver (opts.tol, a correction's, or a
                        warm start's tol ||b|| / ||b - S x0||) */
  int verify_run;    /* GMRES, BiCGSTAB, Richardson: the run restarts on its own recomputed residual (opts.verify;
                        0 in a correction run and in the run of a warm start, whose caller recomputes) */
  double *d_vr, *d_ve; /* opts.verify: right-hand side and solution of a correction run */
  /* a solve from an initial guess (solve_x0_core): r0 = b - S x0 and the correction e, n_here doubles each, taken
   * on the first such call; ||b_c - S x0_c|| / ||b_c|| of the last one (start_n columns; 0: the last solve was cold) */
  double *d_x0r, *d_x0e;
  double *start_rr;
  unsigned start_n, start_cap;
  /* Successive right-hand sides (hip_seq_drv.c), NULL until lsb_hip_solver_seq_begin: ONE allocation of `bytes` -- the
   * pairs x~_k (X) and S x~_k (SX), depth columns of ld doubles each (ld even, the rows behind n_here zero), the
   * records of the sweeps (parts) and the scalars (scal: the coefficients of the projection and of the two
   * Gram-Schmidt passes, the record of the store) -- in the solver's internal numbering; events around the last
   * projection and the last update, made and recorded only once asked for */
  struct seq_basis {
    unsigned depth, held, restarts;
    size_t ld;
    double *X, *SX, *parts, *scal;
    unsigned long long bytes;
    hipEvent_t ev[4];
    int timing, timed_project, timed_update; /* timing: lsb_hip_solver_seq_last_us was called, the events exist */
  } *seq;
  unsigned agree_nnz, agree_n; /* distributed: largest shard, identical on all ranks */
  unsigned agree_halo;         /* largest halo (doubles) any shard receives from one peer */
  /* opts.overlap = -1: the split SpMV (interior rows while the halo travels) against the plain one,
   * timed on the real communicator at creation (overlap_setup): -1 undecided, else the choice; the
   * two timings in us per iteration (max over ranks), 0 where the pass did not run */
  int overlap_on;
  double overlap_us[2];
  /* reordering: d_perm[new] = old; b and x are permuted through d_bp / d_xp */
  int *d_perm;
  double *d_bp, *d_xp;
  /* GMRES workspace (allocated on first use) */
  struct gm_work { /* per shard */
    double *V, *parts, *ax;
    struct lsb_gmres_state *st;
    size_t ld;
  } *gm;
  double *gm_red; /* nshard x GM_RED doubles: [0] a norm, [8..) h, [48..) h2 -- all-reduced */
  struct lsb_gmres_state *gm_hst;
  int gm_m;
  /* BiCGSTAB workspace (allocated on first use; hip_bicgstab_drv.c) */
  struct bcg_work { /* per shard */
    double *t, *p, *rhat, *sfull; /* t = Op s^, the direction, the shadow residual, the gather vector of s^ */
    struct lsb_bcg_state *st;
    unsigned nss, ntt, np2; /* partial counts of the sweeps */
  } *bcg;
  double *bcg_red; /* nshard x BCG_RED doubles: the all-reduced dot products */
  struct lsb_bcg_state *bcg_hst; /* pinned, 2 slots */
  /* Richardson (hip_rich_drv.c): its vectors are the shard's own (r, q, the gather vector for z) and its state the
   * shard's d_st, polled through h_st; what it owns is its cache of captured graphs, keyed on the count and on x,
   * and the partial count of its update sweep */
  struct graph_cache rich_graphs;
  unsigned rich_nrr;
  /* The direct solver (hip_direct_drv.c), NULL on every other solver: the inverse factor in tiers on the device and
   * the dealing of its rows (k; one tier: the single skyline), y (d_t; at one tier t = W P r) and z (NULL at one tier),
   * what the factor is (entries of the W_tt, of the coupling, tree height, set-up seconds), the record count of the
   * residual launch, and its cache of captured graphs -- keyed on the count and on x; b is in them too, so they are
   * dropped when a solve brings another b (graph_b).  Blocks of right-hand sides (hip_direct_m_drv.c): a work area per
   * width, made when the solver first solves a block of that width (m: blk.kp != 0) -- interleaved B, X, R and Y
   * (blk.b, .x, .r, .p; at one tier Y is T = W P V), tiered a fifth block, Z (blk.q), behind them the records of the
   * residual launch and the state; its graphs are keyed on the count alone (blk.g), its hint is the rounds the previous
   * block of this width took */
  struct direct_dev {
    struct lsb_dirt_dev k;
    void *mem[17];
    double *d_t, *d_z;
    unsigned long long entries, coupling;
    unsigned height, nrec;
    double setup_s;
    struct graph_cache graphs;
    const double *graph_b;
    struct dirm_work {
      struct block_work blk;
      double *rec;
      struct lsb_mrhs_state *st;
      unsigned nrec, hint;
    } m[3];
  } *dir;
  /* Interleaved blocks of right-hand sides, per width kp = 2, 4, 8 and allocated on first use.  Two drivers run on
   * them -- independent recurrences (hip_mrhs_drv.c) and block-CG (hip_bcg_drv.c) -- and each keeps its OWN work
   * areas: their graph caches are keyed on the iteration count alone, and a caller may alternate the two on one
   * solver.  What an area of either has in common is struct block_work; its records, its state and its hints lie
   * beside it in the driver's struct. */
  struct mrhs_work {
    struct block_work blk;
    double *parts_pq, *parts2;   /* records of the SpMM (kp wide) and of the sweeps (2 kp wide) */
    double *parts_bb;            /* a batch from an initial guess: the records of b.b (2 kp wide), on first use */
    struct lsb_mrhs_state *st;
    unsigned hint[LSB_MAX_CORRECTIONS + 1]; /* launches the previous batch's solve and restarts took */
  } mr[3];
  struct lsb_mrhs_state *mr_hst; /* pinned, 2 slots */
  /* lanes per row of the SpMM on blocks (never 0 once read) and, FSAI on blocks, of G and of G^T (0 = each matrix's
   * own): read when the solver first runs a block, whichever driver that is (block_work_slab) */
  unsigned mr_lanes, mr_fs_lanes;
  struct blockcg_work {
    struct block_work blk;
    double *rec_spmm, *rec_pass; /* records of the SpMM (LSB_MAX_PARTIALS) and of the passes (LSB_STREAM_GRID_CAP) */
    double *rec_gram; /* solve_block_precond under FSAI: the records of the row kernel that forms the Gram sums
                         (LSB_MAX_PARTIALS), behind z and t in blk.zmem; under AMG they are a streaming pass's (rec_pass) */
    struct lsb_blockcg_state *st;
    unsigned hint;             /* SpMMs the previous block of this width took */
  } bk[3];
  struct lsb_blockcg_state *bk_hst; /* pinned, 2 slots; slot 0 keeps the last block's final state */
  /* AMG as the solver on blocks (hip_rich_m_drv.c): a work area per width, made when the solver first sees a block of
   * that width -- interleaved B, X, R and Q = S Z (blk.b, .x, .r, .p), Z at the head of the cycle's block vectors
   * (blk.z, blk.amg_mem, blk.av: fp64 or fp32 as the solver cycles); behind the four blocks the records of the SpMM,
   * which nobody reads, those of the sweeps, and the state, polled through mr_hst.  Its graphs are keyed on the count
   * alone (blk.g); hint: the cycles the previous block of this width and each of its restarts took */
  struct richm_work {
    struct block_work blk;
    double *rec_spmm, *rec;
    struct lsb_mrhs_state *st;
    unsigned nrec;
    unsigned hint[LSB_MAX_CORRECTIONS + 1];
  } rm[3];
  hipEvent_t ev_poll[2], ev_vec, ev_halo;
  hipEvent_t ev[4 * MAX_SAMPLES], ev_t0, ev_t1; /* per sample: e0 SpMV e1 e2 e3 */
  unsigned char samp_skip[MAX_SAMPLES];         /* the sample brackets nothing (a run's first iteration in the
                                                   two-launch form: a plain SpMV launch, not k_pcg_col_px) */
  int have_events;
  double *d_tmp; /* n_here doubles: scratch for spmv_dev / jacobi sweep */
  /* direct xGMI path (hip_p2p.hip), one context per shard; p2p_on: used for
   * the all-reduces, p2p_halo: also for the halo exchange */
  /* single-reduction PCG without the vector u = D^-1 r: every shard of every
   * rank has the same constant Jacobi diagonal (k_cg1_update<UI>) */
  int cg1_implicit;
  const struct solve_driver *driver; /* the iteration driver this solver runs (solve_driver_for) */
  enum pcg_form form; /* the PCG iteration this solver runs (pcg_choose_form) */
  int pcur, rcur; /* launch-bound fused paths: which direction / residual buffer is current */
  int nt_mask;    /* which operands of the BLAS-1 sweeps are loaded nontemporal (tune_blas1_nt) */
#define LSB_CHEB_MAX 32
  int cheb_m, cheb_fused; /* fused: the steps ride in the SpMV's epilogue (one shard, 16-bit sliced-ELL) */
  double cheb_lmin, cheb_lmax, cheb_c0, cheb_a[LSB_CHEB_MAX], cheb_b[LSB_CHEB_MAX];
  /* launch-bound operators: the whole solve as one persistent launch (hip_persist.hip) */
  struct {
    int ok, use;          /* qualifies / chosen */
    unsigned G, stride, lanes;
    unsigned *d_wgrow;    /* G+1 row bounds of the workgroups */
    double *d_ug;         /* the shared vector u */
    void *d_shared;       /* barrier counter + partial records */
    double us_persist, us_launches; /* creation-time timing of 40 iterations each way */
  } ps;
  struct lsb_p2p **p2p;
  int p2p_on, p2p_halo;
  /* single-reduction CG over the direct path: the all-reduce's collect phase rides at the
   * head of k_cg1_update (ar_fold = 1), its contribute phase in the SpMV's last launch too
   * (ar_fold = 2) -- hip_ar.h, can_fold_allreduce.  fold_next: the next exchange_and_spmv
   * arms the tails; ar_pending: a contribution is out, the next k_cg1_update collects it */
  int ar_fold, fold_next, ar_pending;
  double p2p_us, rccl_us; /* self-test: one exchange + all-reduce, each way */
};

/* the Jacobi diagonal as the fused sweeps take it: the vector, or (NULL, c) when
 * every entry is the same c -- then nobody reads 8 n bytes to learn it */
#define DINV(s) ((s)->dinv_uniform ? NULL : (s)->d_dinv), (s)->dinv_const

/* the iteration-count hint of the solve proper (round 0) or of its k-th correction run: each keeps its own, the
 * benchmark protocol repeats the same sequence trial after trial */
static inline unsigned *hint_slot(unsigned *hints, int round) {
  return &hints[round < LSB_MAX_CORRECTIONS ? round : LSB_MAX_CORRECTIONS];
}

/* lanes per row of the row kernels from a mean row length: the next power of two, 2 .. 64 */
static inline unsigned row_lanes(unsigned len) {
  unsigned L = 2;
  while (L < len && L < 64)
    L <<= 1;
  return L;
}

/* hip_fsai.hip */
void lsb_k_fsai_rows(const unsigned *rows, unsigned nrows, unsigned mcap, const int *offs, const int *cols,
                     const double *vals, unsigned row_begin, const unsigned *poffs, const unsigned *pcols,
                     double *gvals, int *bad, void *stream);
void lsb_k_fsai_xr_gr(unsigned n, const int *goffs, const int *gcols, const double *gvals, unsigned lanes,
                      const double *p, const double *q, double *x, const double *rold, double *rnew, double *t,
                      struct lsb_pcg_state *st, int parity, const double *pq_parts, unsigned npq, void *stream);
void lsb_k_fsai_gt_dots(unsigned n, const int *offs, const int *cols, const double *vals, unsigned lanes,
                        const double *t, double *z, const double *r, double *partials2, unsigned *npartials,
                        const struct lsb_pcg_state *st, void *stream);
/* hip_cdna4.c */
LSB_INTERNAL double wall_seconds(void);
/* Leave the process from a state in which a stream of this process may never drain (a hung
 * collective, a peer that never arrived): message, flush, _exit(EXIT_FAILURE).  Never exit():
 * exit() runs the HIP runtime's teardown, which waits for exactly that stream. */
LSB_INTERNAL void lsb_give_up(const char *fmt, ...) __attribute__((noreturn, format(printf, 1, 2)));
LSB_INTERNAL void *dev_upload(const void *h, size_t bytes);
/* hip_run.c */
/* hipStreamSynchronize(g_stream) that gives up after opts.comm_deadline_s on a sharded solver */
LSB_INTERNAL void drain_stream(lsb_hip_solver *sv, const char *what);
LSB_INTERNAL void wait_event(lsb_hip_solver *sv, hipEvent_t ev, const char *what);
/* One run of an iteration driver, described on the caller's stack: enqueue(ctx, count) puts count iterations on the
 * stream -- plain launches or a cached graph, the loop does not know -- and the loop polls the device state into the
 * two pinned slots of h_state until it has stopped; the final state ends in slot 0 (run_loop, hip_run.c). */
typedef void run_enqueue_fn(void *ctx, int count);
struct run_loop {
  const char *name;              /* the driver, as the cannot-happen message names it */
  const void *d_state;           /* the device state that is polled, */
  void *h_state;                 /* its pinned host copy, two slots, */
  size_t state_bytes;            /* and the size of one */
  size_t stop_off, progress_off; /* two ints inside it: the stop word, and the count the hint is taken from */
  int stop_is_running;           /* the stop word is a status (stopped: != RUNNING), or 1: the batch's `running` */
  run_enqueue_fn *enqueue;
  void *ctx;
  int chunk;                     /* iterations per poll */
  int even;                      /* a hinted count is rounded up to even */
  int max_piece;                 /* a hinted count longer than this goes out in equal even pieces, halved until they
                                    fit: graphs beyond ~1k iterations cost more to build than they save.  0: in one */
  long cap;                      /* never more than this on the stream in the whole run; < 0: no cap */
  const char *what_hinted, *what_poll, *what_drain; /* wait_event's and drain_stream's `what` */
};
LSB_INTERNAL void run_loop(lsb_hip_solver *sv, const struct run_loop *r, unsigned *hint);
LSB_INTERNAL void graph_launch(struct graph_cache *gc, int count, const void *key, run_enqueue_fn *plain, void *ctx);
LSB_INTERNAL void graph_drop(struct graph_cache *gc);
LSB_INTERNAL void drop_graphs(lsb_hip_solver *sv); /* every cache of the solver */
LSB_INTERNAL int run_chunk(double bytes, double floor_us, int lo, int hi);
/* iters, status and relres (from rr / bb) of a result out of a polled state */
LSB_INTERNAL void result_from_state(struct lsb_hip_result *r, const struct lsb_pcg_state *st);
/* hip_solver.c */
LSB_INTERNAL double *shard_vec(struct shard *s, size_t count);
LSB_INTERNAL void shard_vec_free(struct shard *s, void *p);
LSB_INTERNAL void sell_launch(struct shard *s, unsigned s0, unsigned ns, const double *xfull, double *y,
                              const double *xdot, double *partials, unsigned *np,
                              const struct lsb_pcg_state *st);
LSB_INTERNAL void spmv_shard(struct shard *s, const double *xfull, double *y, const double *xdot,
                             double *partials, unsigned *np, const struct lsb_pcg_state *st);
/* the same with the fp64 values whatever opts.precision says (residuals, y = Op x) */
LSB_INTERNAL void spmv_shard_exact(struct shard *s, const double *xfull, double *y, const double *xdot,
                                   double *partials, unsigned *np, const struct lsb_pcg_state *st);
LSB_INTERNAL void tune_spmv(lsb_hip_solver *sv, struct shard *s);
/* the halo split of the layout the shard's SpMV runs on and its unit count (ok = 0: the form has none) */
LSB_INTERNAL struct halo_split shard_split(const struct shard *s, unsigned *count);
/* hip_dist.c */
LSB_INTERNAL void p2p_setup(lsb_hip_solver *sv);
LSB_INTERNAL void overlap_setup(lsb_hip_solver *sv);
LSB_INTERNAL void exchange_on(lsb_hip_solver *sv, hipStream_t stream);
LSB_INTERNAL void exchange_p(lsb_hip_solver *sv, int gated);
LSB_INTERNAL void exchange_vec(lsb_hip_solver *sv, int gated, double *const *full);
LSB_INTERNAL void check_aux_status(lsb_hip_solver *sv, const char *where);
LSB_INTERNAL void allreduce_scal(lsb_hip_solver *sv, unsigned off, unsigned cnt, int gated);
/* sum red[shard][off .. off+cnt) (stride doubles per shard) over the shards of all ranks, the result in every
 * shard's copy: GMRES's and BiCGSTAB's scalars, not tied to a PCG state */
LSB_INTERNAL void red_allreduce(lsb_hip_solver *sv, double *red, unsigned stride, unsigned off, unsigned cnt);
LSB_INTERNAL void allreduce_pq(lsb_hip_solver *sv, unsigned cnt, int with2);
LSB_INTERNAL int can_overlap(const lsb_hip_solver *sv);
LSB_INTERNAL int can_fold_allreduce(const lsb_hip_solver *sv);
LSB_INTERNAL void allreduce_pq_contribute(lsb_hip_solver *sv);
LSB_INTERNAL void exchange_and_spmv(lsb_hip_solver *sv, int sample);
/* part 0 / 1 / 2 of the split SpMV: the units that need no halo, the ones before, the ones after them */
LSB_INTERNAL void spmv_range(struct shard *s, int part, double *y, double *partials, unsigned *np,
                             const struct lsb_pcg_state *st);
/* hip_pcg.c */
LSB_INTERNAL enum pcg_form pcg_choose_form(const lsb_hip_solver *sv);
LSB_INTERNAL void form_vecs(lsb_hip_solver *sv, enum pcg_form f);
/* sample k >= 0: events 4k, 4k+1 around shard 0's SpMV (and the bare pair 4k+2, 4k+3); k < 0: nothing */
LSB_INTERNAL void sample_open(lsb_hip_solver *sv, int k);
LSB_INTERNAL void sample_close(lsb_hip_solver *sv, int k);
LSB_INTERNAL void tune_blas1_nt(lsb_hip_solver *sv);
LSB_INTERNAL void persist_setup(lsb_hip_solver *sv);
LSB_INTERNAL solve_dev_fn pcg_solve_dev;
LSB_INTERNAL int pcg_run(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *res, int round);
/* products with the operator of a PCG solve and its correction runs, from the counts in *r */
LSB_INTERNAL unsigned pcg_spmvs(const lsb_hip_solver *sv, const struct lsb_hip_result *r);
/* hip_solve.c */
LSB_INTERNAL const struct solve_driver *solve_driver_for(int krylov);
LSB_INTERNAL solve_dev_fn solve_core;
LSB_INTERNAL solve_dev_fn solve_x0_core; /* the same from the x0 that d_x holds */
LSB_INTERNAL void gather_x(lsb_hip_solver *sv, const double *d_x);
LSB_INTERNAL void op_exact(lsb_hip_solver *sv, const double *d_x); /* q = S x in every shard, with the fp64 values */
LSB_INTERNAL void x0_vecs(lsb_hip_solver *sv); /* d_x0r and d_x0e, taken on first use */
LSB_INTERNAL double true_resid2(lsb_hip_solver *sv, const double *d_b, const double *d_x);
LSB_INTERNAL int direct_path_agrees(lsb_hip_solver *sv, const double *d_b, const double *d_x, double bb,
                                    struct lsb_hip_result *r, const char *then);
LSB_INTERNAL double mixed_floor_tol(const lsb_hip_solver *sv);
LSB_INTERNAL void verify_correct(lsb_hip_solver *sv, const double *d_b, double *d_x, struct lsb_hip_result *r,
                                 double bb, int twice);
/* What a driver that restarts in place hands run_restarting: run enqueues iterations until the device state leaves
 * RUNNING (*hint: what this stretch of the previous solve took), restart enqueues r = b - S x from the x reached
 * and the state that goes with it (more = 0: the last one, the status is final); the state begins with a struct
 * lsb_pcg_state and is polled into h_state */
struct restart_run {
  void (*run)(void *ctx, unsigned *hint);
  void (*restart)(void *ctx, int more);
  void *ctx;
  const void *d_state;
  void *h_state;
  size_t state_bytes;
  const char *what_drain;
};
LSB_INTERNAL unsigned run_restarting(lsb_hip_solver *sv, const struct restart_run *v, struct lsb_hip_result *r);
/* where a warm-started call of nrhs columns records its starting residuals (sets start_n) */
LSB_INTERNAL double *start_relres_slots(lsb_hip_solver *sv, unsigned nrhs);
/* hip_seq_drv.c */
LSB_INTERNAL void seq_free(lsb_hip_solver *sv);
/* hip_precond.c */
LSB_INTERNAL int generic_precond(const lsb_hip_solver *sv);
LSB_INTERNAL void precond_shard_blocks(struct shard *s, const int *offs, const int *cols,
                                       const double *vals, const struct lsb_hip_opts *o);
LSB_INTERNAL void precond_setup(lsb_hip_solver *sv);
LSB_INTERNAL void precond_apply(lsb_hip_solver *sv, int after_update);
LSB_INTERNAL void precond_free_shard(struct shard *s);
/* hip_gmg_drv.c: what LSB_PRECOND_GMG cannot run with is refused (gmg_check, before anything is built); the levels of
 * a shard that was handed its grid; level 0's buffer out of the slab, behind d_zfull; z = one V-cycle of r, on the
 * solver's stream, nothing allocated and nothing synchronised; free */
LSB_INTERNAL void gmg_check(const struct lsb_hip_opts *o, int sharded);
LSB_INTERNAL void precond_shard_gmg(struct shard *s, const struct lsb_hip_opts *o);
LSB_INTERNAL void gmg_finish_setup(struct shard *s);
LSB_INTERNAL void gmg_cycle(const struct shard *s, const double *r, double *z, const struct lsb_pcg_state *st);
LSB_INTERNAL void gmg_free(struct shard *s);
/* hip_amg_drv.c */
LSB_INTERNAL void precond_shard_amg(struct shard *s, const int *offs, const int *cols, const double *vals,
                                    const struct lsb_hip_opts *o);
LSB_INTERNAL void amg_finish_setup(struct shard *s); /* behind d_zfull: level 0's two vectors out of the slab */
LSB_INTERNAL void amg_free(struct shard *s);
/* bytes one cycle streams in the solver's precision: its matrices, its vector passes (lsb_hip_solver_amg_cycle_bytes is
 * their sum; a block of kp columns streams mat + kp vec) */
LSB_INTERNAL void amg_cycle_bytes_split(const struct amg_dev *a, unsigned long long *mat, unsigned long long *vec);
/* One application of the V-cycle, described on the caller's stack: z = M^-1 r in the solver's precision (kp = 0: one
 * column, vec = a->vec) or Z = M^-1 R on interleaved blocks of kp columns (vec = the block_work's; the cycle in fp32
 * takes no records and has no Chebyshev smoother there).  r and z are fp64 and may be anywhere.  records != NULL
 * (blocks): where the launch that writes Z leaves (r_c . z_c, r_c . r_c) of every column, and their number.  The gate of the launches: st (one column) or mst (blocks), NULL: always run. */
struct amg_run {
  const struct amg_dev *a;
  const struct amg_vecs *vec;
  unsigned kp, *nrecords;
  const double *r;
  double *z, *records;
  const struct lsb_pcg_state *st;
  const struct lsb_mrhs_state *mst;
};
LSB_INTERNAL void amg_cycle(const struct amg_run *c);
/* the cycle's vectors at width kp, zeroed: 256-byte aligned pieces of one allocation, which it returns -- Z, level 0's
 * tmp and r, four vectors per coarser level, then the Chebyshev smoother's direction blocks; fills v[0 .. nlev) */
LSB_INTERNAL char *amg_block_vecs(const struct amg_dev *a, unsigned kp, struct amg_vecs *v);
/* the same for the fp32 cycle on blocks: Z (fp64), then b, out, tmp, r as blocks of interleaved floats per level */
LSB_INTERNAL char *amg_block_vecs32(const struct amg_dev *a, unsigned kp, struct amg_vecs *v);
/* the launchers of hip_amg_f32_m.hip: lsb_k_amg32_first / _csr / _dense on blocks of kp = 2, 4 or 8 interleaved float
 * columns, per column bit for bit; in64 / b32, y64, ends64 as theirs, on fp64 blocks in hip_mrhs.hip's layout; st: a
 * no-op once st->running == 0 (NULL: always run) */
LSB_INTERNAL void lsb_k_amg32_first_m(unsigned kp, unsigned n, int in64, const void *b, const float *minv, float *x,
                                      float *b32, const struct lsb_mrhs_state *st, void *stream);
LSB_INTERNAL void lsb_k_amg32_csr_m(unsigned kp, int mode, const struct amg_mat32 *m, const float *xin, const float *b,
                                    const float *minv, float *y, double *y64, const struct lsb_mrhs_state *st,
                                    void *stream);
LSB_INTERNAL void lsb_k_amg32_dense_m(unsigned kp, unsigned nc, unsigned lanes, int ends64, const float *cinv,
                                      const void *b, void *out, const struct lsb_mrhs_state *st, void *stream);
/* hip_gmres_drv.c */
LSB_INTERNAL solve_dev_fn gmres_solve_dev;
/* hip_bicgstab_drv.c */
LSB_INTERNAL solve_dev_fn bicgstab_solve_dev;
LSB_INTERNAL void bicgstab_free(lsb_hip_solver *sv); /* before the shards go: its vectors may sit in their slabs */
/* hip_rich_drv.c, and the launchers of hip_rich.hip (n rows; the 16-byte form where every operand is 16-byte
 * aligned, else the 8-byte form with the same bits; partials: one per workgroup, *npartials of them) */
LSB_INTERNAL solve_dev_fn richardson_solve_dev;
/* what --krylov richardson cannot run with, refused at creation: a preconditioner other than AMG, shards, persistent */
LSB_INTERNAL void richardson_check(const struct lsb_hip_opts *o, int sharded);
LSB_INTERNAL void lsb_k_rich_init(unsigned n, const double *b, double *x, double *r, double *partials,
                                  unsigned *npartials, void *stream);
LSB_INTERNAL void lsb_k_rich_init_state(struct lsb_pcg_state *st, const double *parts, unsigned nparts, double tol,
                                        int maxit, void *stream);
LSB_INTERNAL void lsb_k_rich_update(unsigned n, const double *z, const double *q, double *x, double *r,
                                    const struct lsb_pcg_state *st, double *partials, unsigned *npartials,
                                    void *stream);
LSB_INTERNAL void lsb_k_rich_step(struct lsb_pcg_state *st, const double *parts, unsigned nparts, void *stream);
LSB_INTERNAL void lsb_k_rich_restart(unsigned n, const double *b, const double *ax, double *r, double *partials,
                                     unsigned *npartials, void *stream);
LSB_INTERNAL void lsb_k_rich_restart_state(struct lsb_pcg_state *st, const double *parts, unsigned nparts, int more,
                                           void *stream);
/* hip_rich_m_drv.c: the iteration on blocks of right-hand sides, and the launchers of hip_rich_m.hip (kp: 2, 4 or 8;
 * interleaved blocks; records: kp doubles per workgroup of a sweep, *nrecords of them; per column the bits of the
 * launchers above on that column alone) */
LSB_INTERNAL void richm_free(lsb_hip_solver *sv); /* the work areas of every width */
LSB_INTERNAL void lsb_k_richm_init(unsigned kp, unsigned n, const double *b, double *x, double *r, double *records,
                                   unsigned *nrecords, void *stream);
LSB_INTERNAL void lsb_k_richm_init_state(unsigned kp, struct lsb_mrhs_state *st, const double *records,
                                         unsigned nrecords, double tol, int maxit, void *stream);
LSB_INTERNAL void lsb_k_richm_update(unsigned kp, unsigned n, const double *z, const double *q, double *x, double *r,
                                     const struct lsb_mrhs_state *st, double *records, unsigned *nrecords,
                                     void *stream);
LSB_INTERNAL void lsb_k_richm_step(unsigned kp, struct lsb_mrhs_state *st, const double *records, unsigned nrecords,
                                   void *stream);
/* the verify round: r = b - ax for the columns called converged; then their recomputed norms decide, a column with
 * fewer than max_restarts restarts behind it may cycle on */
LSB_INTERNAL void lsb_k_richm_restart(unsigned kp, unsigned n, const double *b, const double *ax, double *r,
                                      const struct lsb_mrhs_state *st, double *records, unsigned *nrecords,
                                      void *stream);
LSB_INTERNAL void lsb_k_richm_restart_state(unsigned kp, struct lsb_mrhs_state *st, const double *records,
                                            unsigned nrecords, int max_restarts, void *stream);
/* hip_direct_drv.c, and the launchers of hip_direct.hip */
LSB_INTERNAL solve_dev_fn direct_solve_dev;
/* what --krylov direct cannot run with, refused at creation (shards, persistent); what it does not consult is set
 * aside (precond, reorder), and mixed precision falls back to fp64, said aloud */
LSB_INTERNAL void direct_check(struct lsb_hip_opts *o, int sharded);
/* order, count, factorise on the host in `tiers` tiers (1: the single skyline; 0: the fewest that fit): refuses an
 * operator over the entry budget before anything is allocated, and one that is not symmetric positive definite */
LSB_INTERNAL struct lsb_tierinv *direct_factor(const struct csr *S, const struct lsb_hip_opts *o, int tiers,
                                               unsigned *height, double *seconds);
LSB_INTERNAL void direct_tier_upload(lsb_hip_solver *sv, struct lsb_tierinv *T, unsigned height, double seconds); /* frees T */
LSB_INTERNAL void direct_free(lsb_hip_solver *sv);
LSB_INTERNAL int direct_apply_dev(lsb_hip_solver *sv, const double *d_r, double *d_z); /* z = L^-T L^-1 r, once */
/* a direct solver whose factor has more than one tier: coupling, z, 4 m - 2 launches per round, blocks of right-hand
 * sides through lsb_hip_solver_solve_direct_tier_multi[_dev] alone */
static inline int direct_tiered(const lsb_hip_solver *sv) { return sv->dir->k.ntier > 1; }
/* what a round on a block of width kp streams (kp = 1: a single solve) */
LSB_INTERNAL unsigned long long direct_round_bytes(const lsb_hip_solver *sv, unsigned kp);
LSB_INTERNAL void lsb_k_dir_init_state(struct lsb_pcg_state *st, double tol, int maxit, void *stream);
LSB_INTERNAL void lsb_k_dir_resid(unsigned n, const int *offs, const int *cols, const double *vals, unsigned lanes,
                                  const double *b, const double *x, double *r, double *records, unsigned *nrecords,
                                  const struct lsb_pcg_state *st, void *stream);
LSB_INTERNAL void lsb_k_dir_step(struct lsb_pcg_state *st, const double *records, unsigned nrecords, void *stream);
/* the launchers of hip_direct_t.hip, the products on tier t: src 0 = the operand by the state (b in round 1, r
 * afterwards), 1 = b whatever the state says; mode 0 = x by the state (stored in round 1, added to afterwards), 1 =
 * stored; z may be NULL in lsb_k_dirt_cols (one tier) */
LSB_INTERNAL void lsb_k_dirt_rows(const struct lsb_dirt_dev *d, unsigned t, const double *b, const double *r,
                                  const double *v, double *y, const struct lsb_pcg_state *st, int src, void *stream);
LSB_INTERNAL void lsb_k_dirt_cols(const struct lsb_dirt_dev *d, unsigned t, const double *y, double *z, double *x,
                                  const struct lsb_pcg_state *st, int mode, void *stream);
LSB_INTERNAL void lsb_k_dirt_fwd(const struct lsb_dirt_dev *d, unsigned t, const double *b, const double *r,
                                 const double *y, double *z, const struct lsb_pcg_state *st, int src, void *stream);
LSB_INTERNAL void lsb_k_dirt_bwd(const struct lsb_dirt_dev *d, unsigned t, const double *z, double *y,
                                 const struct lsb_pcg_state *st, void *stream);
/* the same on a block of kp = 2, 4 or 8 interleaved right-hand sides (hip_direct_tm.hip): B, R, X of the work area in
 * the caller's numbering, Y = k->p and Z = k->q (NULL at one tier) in the factor's; st: the gate, NULL for one
 * un-gated application that reads k->b and stores k->x */
LSB_INTERNAL void direct_tier_enqueue_m(lsb_hip_solver *sv, const struct block_work *k,
                                        const struct lsb_mrhs_state *st);
LSB_INTERNAL void lsb_k_dirt_rows_m(unsigned kp, const struct lsb_dirt_dev *d, unsigned t, const double *b,
                                    const double *r, const double *v, double *y, const struct lsb_mrhs_state *st,
                                    void *stream);
LSB_INTERNAL void lsb_k_dirt_cols_m(unsigned kp, const struct lsb_dirt_dev *d, unsigned t, const double *y, double *z,
                                    double *x, const struct lsb_mrhs_state *st, void *stream);
LSB_INTERNAL void lsb_k_dirt_fwd_m(unsigned kp, const struct lsb_dirt_dev *d, unsigned t, const double *b,
                                   const double *r, const double *y, double *z, const struct lsb_mrhs_state *st,
                                   void *stream);
LSB_INTERNAL void lsb_k_dirt_bwd_m(unsigned kp, const struct lsb_dirt_dev *d, unsigned t, const double *z, double *y,
                                   const struct lsb_mrhs_state *st, void *stream);
/* hip_direct_m_drv.c: the direct solver on blocks of right-hand sides, and the launchers of hip_direct_m.hip (kp: 2, 4
 * or 8; interleaved blocks; st: the gate) */
LSB_INTERNAL void direct_multi_free(lsb_hip_solver *sv); /* the work areas of every width */
LSB_INTERNAL void lsb_k_dir_init_state_m(struct lsb_mrhs_state *st, unsigned kp, double tol, int maxit, void *stream);
LSB_INTERNAL void lsb_k_dir_resid_m(unsigned kp, unsigned n, const int *offs, const int *cols, const double *vals,
                                    unsigned lanes, const double *b, const double *x, double *r, double *records,
                                    unsigned *nrecords, const struct lsb_mrhs_state *st, void *stream);
LSB_INTERNAL void lsb_k_dir_step_m(unsigned kp, struct lsb_mrhs_state *st, const double *records, unsigned nrecords,
                                   void *stream);
/* hip_block.c: what the two drivers on interleaved blocks share */
/* the service rules: the SpMM on blocks; the solves on blocks (the SpMM's, less an AMG cycle smoothed by multicolour
 * Gauss-Seidel); whether z = M^-1 r is a block of its own there (AMG, FSAI) or the diagonal's */
LSB_INTERNAL int block_spmm_serves(const lsb_hip_solver *sv);
LSB_INTERNAL int block_serves(const lsb_hip_solver *sv);
LSB_INTERNAL int block_fsai(const lsb_hip_solver *sv);
LSB_INTERNAL int block_zblock(const lsb_hip_solver *sv);
LSB_INTERNAL unsigned block_width(unsigned nrhs); /* 2, 4 or 8: what nrhs <= 8 columns run at */
LSB_INTERNAL unsigned block_fsai_lanes(const lsb_hip_solver *sv, const struct fsai_csr *c); /* of G or of G^T */
/* 1: a call on nrhs columns (max_nrhs != 0: no more than that) with leading dimensions lda, ldb is refused */
LSB_INTERNAL int block_args_bad(const lsb_hip_solver *sv, unsigned nrhs, unsigned max_nrhs, const void *a, size_t lda,
                                const void *b, size_t ldb);
/* The slab of a work area, zeroed: nblk blocks of n kp doubles (the five; 7: z and t behind them; 4: b, x, r, p alone,
 * the direct solver's), then `behind` bytes of the owner's, whose address it returns.  The first slab of a solver reads
 * the lanes per row. */
LSB_INTERNAL char *block_work_slab(lsb_hip_solver *sv, struct block_work *w, unsigned kp, unsigned nblk, size_t behind);
/* z where the slab does not hold it, zeroed.  FSAI: z, t and `behind` bytes of the owner's (returned) in zmem.
 * AMG: the cycle's block vectors with z at their head; behind must be 0, returns NULL. */
LSB_INTERNAL char *block_work_z(lsb_hip_solver *sv, struct block_work *w, size_t behind);
LSB_INTERNAL void block_work_free(struct block_work *w);
/* T = G R by the SpMM's rule, un-gated (FSAI).  Its records of r_c . t_c, which nobody reads, go into rec: kp
 * LSB_MAX_PARTIALS doubles that no launch still in front of its next writer reads. */
LSB_INTERNAL void block_fsai_g(const lsb_hip_solver *sv, const struct block_work *w, const double *r, double *rec);
/* Z = M^-1 R of every column into w->z, un-gated and without records: FSAI's two products (rec: as above), or one
 * V-cycle */
LSB_INTERNAL void block_zapply(const lsb_hip_solver *sv, const struct block_work *w, const double *r, double *rec);
/* What run_loop enqueues on a work area: `iters` launches a linear chain of that many iterations on internal buffers,
 * so under opts.use_graph its graphs are keyed on the count alone (w->g) */
struct block_enq {
  lsb_hip_solver *sv;
  struct block_work *w;
  run_enqueue_fn *iters;
  void *ctx;
};
LSB_INTERNAL void block_enqueue(void *block_enq, int iters);
/* A _dev entry point on host buffers: B in, the call, X out -- whatever it answered (x_always) or only where it
 * answered 0.  The caller has checked the arguments and the service rule. */
typedef int block_dev_fn(lsb_hip_solver *, unsigned, const double *, size_t, double *, size_t, struct lsb_hip_result *);
LSB_INTERNAL int block_solve_host(block_dev_fn *dev, int x_always, lsb_hip_solver *sv, unsigned nrhs, const double *B,
                                  size_t ldb, double *X, size_t ldx, struct lsb_hip_result *res);
/* hip_mrhs_drv.c */
LSB_INTERNAL void mrhs_free(lsb_hip_solver *sv); /* before the shards go */
/* hip_bcg_drv.c */
LSB_INTERNAL void blockcg_free(lsb_hip_solver *sv); /* before the shards go */

#endif
