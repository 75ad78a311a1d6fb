/*
 * C-ABI of the MI355X (gfx950) sparse-solve backend for lsbench.
 *
 * Everything here is `extern "C"`, plain pointers and sizes.  The library that
 * exports it is liblsbench_hip.so (built by lsbench_amd/csrc/Makefile).  Three
 * layers, outermost first:
 *
 *   1. the backend trio  hip_cdna4_{init,finalize,bench}  -- the drop-in
 *      boundary: the same three-function contract every reference backend
 *      implements (reference: src/lsbench-impl.h:42-68; template
 *      src/cusparse.c:137-213);
 *   2. the solver-handle API  lsb_hip_solver_*  -- what hip_cdna4_bench is made
 *      of, exposed so a caller can keep the operator resident in HBM and solve
 *      repeatedly (bench.py, tests);
 *   3. kernel-level entry points  lsb_hip_<op>_f64  -- one per hand-written HIP
 *      kernel, raw device pointers + a hipStream_t passed as void*.
 *
 * Return convention (reference: src/cusparse.c:139-140,154-155,166-167):
 * 0 = ok, 1 = backend not initialised / already initialised / no device,
 * 2 = bad argument.  A failing HIP or RCCL call is fatal: errx(EXIT_FAILURE,
 * "file:line ...") exactly like the reference's chk_rt macro
 * (src/cusparse.c:24-31).  Nothing in this library falls back to a CPU path.
 */
#ifndef LSBENCH_HIP_H
#define LSBENCH_HIP_H

#include "lsbench.h"
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Data layouts handed across the boundary                                   */
/* ------------------------------------------------------------------------ */

/* Run configuration.  Layout = reference src/lsbench-impl.h:14-20. */
struct lsbench {
  char *matrix;
  lsbench_solver_t solver;
  lsbench_ordering_t ordering;
  lsbench_precision_t precision;
  unsigned verbose, trials;
};

/* CSR container.  Layout = reference src/lsbench-impl.h:22-26.
 * offs[nrows+1] is always 0-based; cols[] keep the file's base (0 or 1); rows
 * are sorted by column with duplicates summed (src/lsbench-csr.c:54-63). */
struct csr {
  unsigned nrows, base;
  unsigned *offs, *cols;
  double *vals;
};

/* ------------------------------------------------------------------------ */
/* 1. Backend trio (drop-in boundary)                                        */
/* ------------------------------------------------------------------------ */

/* Replaces nothing, adds the 7th backend next to cusparse_init
 * (src/lsbench-impl.h:42).  Creates the HIP stream; returns 1 quietly when no
 * device is present, because lsbench_init initialises every backend whatever
 * --solver says (src/lsbench.c:143-147). */
int hip_cdna4_init(void);

/* Counterpart of cusparse_finalize (src/lsbench-impl.h:43). */
int hip_cdna4_finalize(void);

/* Counterpart of cusparse_bench / cholmod_bench (src/lsbench-impl.h:44-45,
 * 57-58).  x: caller-owned, length nrows, zero on entry (initial guess),
 * receives the solution in original row order (src/cusparse.c:203-204).
 * r: right-hand side, length nrows.  Protocol (src/cholmod-impl.h:34-71):
 * untimed setup, cb->trials warm-up solves, cb->trials timed solves, one CSV
 * record on stdout.  The operator solved is the one CHOLMOD is given:
 * S = triu(A) + triu(A,1)^T (src/cholmod-impl.h:5-16). */
int hip_cdna4_bench(double *x, struct csr *A, const double *r,
                    const struct lsbench *cb);

/* Two optional companions of the trio for a host program's command line and loader
 * (integration/hip-flags.patch adds the calls to src/lsbench.c:84-133 and
 * src/lsbench-csr.c:29; with ENABLE_HIP=OFF the stub file answers 1 / NULL):
 * set one option of hip_cdna4_bench by name -- "tol", "maxit", "ngpus", "krylov",
 * "operator", "precond", "cheb-degree", "block-size", "precision", "nvirt", "restart",
 * "reorder", "comm", "overlap", "verify", ... (hip_cdna4.c: OPTS; the same names upper-
 * cased behind LSBENCH_HIP_ are the environment switches) -- 0 = set, 1 = no such option
 * or not a value it takes; and the backend's synthetic operators (configs 3-5) as a
 * `struct csr *` the reference's lsbench_matrix_free can free. */
int hip_cdna4_set_option(const char *name, const char *value);
struct csr *hip_cdna4_matrix_synth(const char *spec);

/* ------------------------------------------------------------------------ */
/* Options / results (additive; the reference has no such knobs)             */
/* ------------------------------------------------------------------------ */

enum { LSB_OP_CHOLMOD_UPPER = 0, /* S = triu(A)+triu(A,1)^T (default)      */
       LSB_OP_RAW = 1 };         /* the CSR exactly as handed in            */
enum { LSB_PRECOND_JACOBI = 0, LSB_PRECOND_NONE = 1,
       LSB_PRECOND_L1JACOBI = 2, /* M = diag(sum_j |S_ij|): SPD for every
                                    symmetric S with non-empty rows, no
                                    stored diagonal needed */
       LSB_PRECOND_CHEBYSHEV = 3,   /* z = p_k(D^-1 S) D^-1 r: Chebyshev polynomial
                                       of degree m = opts.cheb_degree on the interval
                                       [l / max(30, 16 m^2), l], l = 1.1 lmax of D^-1 S
                                       from a power iteration at setup (the smoother the
                                       reference's AMG backends configure,
                                       src/hypre.c:126-158, src/amgx.c:78-85) */
       LSB_PRECOND_BLOCKJACOBI = 4,   /* M = blockdiag(S) with opts.block_size rows
                                       per block, blocks inverted at setup (the
                                       block form of src/ginkgo.cpp:57-58's
                                       Jacobi preconditioner)                 */
       LSB_PRECOND_FSAI = 5,          /* factorised sparse approximate inverse,
                                       M^-1 = G^T G with G on the pattern of tril(S^k),
                                       k = opts.fsai_power: the expensive part (one small
                                       dense SPD solve per row, on the device) happens
                                       once, outside the timed loop -- the reference's
                                       own protocol for its CPU path, which factorises
                                       in csr_init (src/cholmod-impl.h:25-26) and times
                                       only solves (:59-62); an application is two SpMVs,
                                       no triangular solve, no reduction        */
       LSB_PRECOND_AMG = 6,           /* smoothed-aggregation algebraic multigrid: one
                                       symmetric V-cycle with l1-Jacobi smoothing (or a
                                       Chebyshev polynomial in D^-1 A of the same cost:
                                       opts.amg_smoother), the hierarchy built on the
                                       host at solver creation (lsb_amg_setup), applied
                                       by hip_amg.hip; one shard, classic PCG  */
       LSB_PRECOND_GMG = 7 };         /* geometric multigrid on a constant-coefficient 5- or
                                       7-point grid operator (lsb_gmg_detect; anything else is
                                       refused at creation): one symmetric V-cycle with damped
                                       Jacobi smoothing, no matrix on any level -- every level
                                       is the stencil, the kernels stream vectors only
                                       (lsb_gmg.c, hip_gmg_drv.c, hip_gmg.hip).  Reads the
                                       multigrid members amg_sweeps, amg_coarse and
                                       amg_max_levels; one shard, fp64, classic PCG; opt-in */
enum { LSB_AMG_SMOOTH_L1JACOBI = 0,   /* nu sweeps x += diag(sum_j |a_ij|)^-1 (b - A x)  */
       LSB_AMG_SMOOTH_CHEB = 1,       /* the Chebyshev polynomial of degree nu in D^-1 A on
                                       [rho / opts.amg_cheb_ratio, rho], rho the level's
                                       Gershgorin bound (lsb_amg_gershgorin): a guaranteed
                                       bound, so the cycle stays SPD; nu row launches as nu
                                       sweeps, one more vector (the direction d) per level */
       LSB_AMG_SMOOTH_MCGS = 2 };     /* multicolour Gauss-Seidel: nu forward sweeps before and nu
                                       backward sweeps after the coarse correction, in place, a
                                       launch per colour of a greedy colouring (lsb_amg_colour), on
                                       every level of at most LSB_AMG_MCGS_COLOURS colours; the other
                                       levels keep l1-Jacobi.  No spectral bound; opt-in
                                       (hip_amg_mcgs.hip; one column only) */
enum { LSB_AMG_PREC_FP64 = 0,         /* the V-cycle in fp64 (default)                          */
       LSB_AMG_PREC_FP32 = 1 };       /* the whole hierarchy and every level vector in fp32, inside
                                       a Krylov loop that stays fp64 (x, r, p, q, every dot product,
                                       the stop test): 8 B per stored entry and 4 B per vector
                                       element where the fp64 cycle moves 12 and 8 (hip_amg_f32.hip);
                                       no one-launch tail, no blocks of columns               */
enum { LSB_KRYLOV_PCG = 0,    /* preconditioned CG (symmetric operators)    */
       LSB_KRYLOV_GMRES = 1,  /* restarted GMRES(m), right-preconditioned,
                                 for LSB_OP_RAW / unsymmetric operators;
                                 single shard only in this round            */
       LSB_KRYLOV_PCG1 = 2,   /* single-reduction CG (Chronopoulos-Gear): the
                                 same iterates with 2 launches and 1 global
                                 reduction per iteration instead of 3 and 2 */
       LSB_KRYLOV_AUTO = 3,   /* PCG1 when the operator is spread over several
                                 shards (one collective less per iteration),
                                 PCG otherwise                              */
       LSB_KRYLOV_BICGSTAB = 4, /* BiCGSTAB, right-preconditioned by a diagonal
                                 (Jacobi, l1-Jacobi, none): the reference's Ginkgo
                                 backend (src/ginkgo.cpp:55-64); short recurrences
                                 for unsymmetric operators -- seven vectors, two
                                 SpMVs and four sweeps per iteration; one shard or
                                 several; trust it with opts.verify = 1        */
       LSB_KRYLOV_RICHARDSON = 5, /* AMG as the solver (LSB_PRECOND_AMG only, one shard):
                                 stationary V-cycle iterations, the way the reference's AMG
                                 backends run (src/hypre.c:185-186, src/amgx.c:78-85 --
                                 maxit = 2, tol = 0 is their protocol).  x = 0, r = b; cycle
                                 k: z = M^-1 r (one V-cycle, either smoother, fp64 or fp32),
                                 q = S z, x += z, r -= q, iters = k, then stop: r.r <=
                                 tol^2 b.b CONVERGED, r.r not finite BREAKDOWN, k >= maxit
                                 MAXIT.  tol = 0 never converges: exactly maxit cycles.  x
                                 and r stay fp64 (around the fp32 cycle: iterative
                                 refinement); iters counts cycles, relres^(1/iters) is the
                                 convergence factor per cycle; opts.verify as in PCG       */
       LSB_KRYLOV_DIRECT = 6 }; /* a sparse direct solve (one shard, fp64; hip_direct.hip): at creation a nested-
                                 dissection ordering, a Cholesky factor and its explicit inverse W = L^-1 as a
                                 skyline (lsb_csr_skyline_inverse), untimed like every set-up; a round is
                                 x (+)= W^T (W (P r)), two launches with no dot product and no host poll between
                                 them, then -- tol > 0 -- r = b - S x and the stop test on that RECOMPUTED residual:
                                 r.r <= tol^2 b.b CONVERGED, not finite BREAKDOWN, rounds >= maxit MAXIT.  iters
                                 counts rounds (rounds after the first are iterative refinement), relres and
                                 true_relres are both the recomputed figure, spmvs counts residuals.  tol = 0: exactly
                                 maxit rounds, the last without a residual, MAXIT, relres = -1; maxit = 1, tol = 0 is
                                 the reference's direct protocol (src/cholmod-impl.h:59-62).  opts.precond and
                                 opts.reorder are not consulted: the factor is the method and orders for itself.
                                 For operators of a few thousand to a few tens of thousands of rows
                                 (LSB_DIRECT_MAX_ENTRIES); a larger one, shards and persistent are refused */
enum { LSB_SPMV_AUTO = 0,     /* pick by mean row length                    */
       LSB_SPMV_ADAPTIVE = 1, /* row-blocked: LDS-streamed short rows +
                                 wavefront-per-row long rows                */
       LSB_SPMV_SUBWAVE = 2,  /* 2..64 lanes per row, shuffle reduction     */
       LSB_SPMV_SCALAR = 3,   /* one lane per row (test/debug baseline)     */
       LSB_SPMV_PANEL = 4,    /* column panels with an L2-resident x window,
                                 for scattered rows (solver handle only)    */
       LSB_SPMV_SELL = 5,     /* sliced-ELL copy of the rows (lsb_csr_sellize):
                                 128-row slices stored column-major, two rows
                                 per lane, no LDS; for near-uniform row lengths */
       LSB_SPMV_TWOPHASE = 7, /* scattered operators: products streamed out by
                                 column chunk (x window in LDS), added up by row
                                 bin (y rows in LDS): lsb_csr_pbize             */
       LSB_SPMV_BINNED = 6 }; /* scattered operators: entries binned by column
                                 panel (an L2-sized window of x) and sorted by
                                 row inside a bin, streamed as (row, col, value)
                                 with a segmented reduction per row -- uniform
                                 work per lane whatever the row lengths
                                 (lsb_csr_binize; solver handle only)         */
enum { LSB_STATUS_RUNNING = 0, LSB_STATUS_CONVERGED = 1,
       LSB_STATUS_BREAKDOWN = 2, LSB_STATUS_MAXIT = 3,
       LSB_STATUS_COMM = 4 /* a peer never arrived (direct xGMI path) */ };
/* how sharded solves communicate */
enum { LSB_COMM_AUTO = 0,  /* direct xGMI stores where they validate and win */
       LSB_COMM_RCCL = 1,  /* RCCL send/recv + all-reduce                    */
       LSB_COMM_P2P = 2 }; /* direct xGMI stores, or fail                    */

struct lsb_hip_opts {
  double tol;        /* stop when ||r||_2 <= tol*||b||_2            [1e-12] */
  unsigned maxit;    /* iteration cap                               [20000] */
  int op_mode;       /* LSB_OP_*                          [CHOLMOD_UPPER]   */
  int precond;       /* LSB_PRECOND_*                             [JACOBI]  */
  int spmv_variant;  /* LSB_SPMV_*                                  [AUTO]  */
  int check_every;   /* iterations enqueued per host poll             [0=auto] */
  int use_graph;     /* replay iterations from a hipGraph (1 rank)     [1]  */
  int sample_spmv;   /* HIP-event-time every Nth SpMV launch (0=off)   [0]  */
  int nvirt;         /* >1: split into that many row-range shards on ONE
                        device, exchanging by device copies (test mode) [1] */
  int comm;          /* LSB_COMM_*                                      [0] */
  int overlap;       /* multi-shard: start the SpMV's interior rows while the
                        halo is in flight; 1 on, 0 off, -1 = on when some
                        halo is >= 64 Ki doubles (the split costs launches) [-1] */
  int spmv_tune;     /* -1: time the SpMV flavours at creation and keep the
                        fastest; >= 0: force flags (bit 0 prefetch, bit 1
                        nontemporal)                                   [-1] */
  int spmv_grid;     /* workgroup cap of the SpMV launch, 0 = tuned     [0] */
  int reorder;       /* 1: solve P S P^T with P = reverse Cuthill-McKee, permute
                        b, un-permute x (single shard)                  [0] */
  int krylov;        /* LSB_KRYLOV_* (PCG, GMRES, PCG1, AUTO, BICGSTAB,
                        RICHARDSON)                                  [AUTO] */
  int restart;       /* GMRES restart length m, 1..32                  [30] */
  int verbose;
  int ngpus;         /* hip_cdna4_bench only: row-partition the operator over
                        this many GPUs of the node, all driven from the ONE
                        caller process (one host thread per GPU); 0 = every
                        visible device.  Also LSBENCH_HIP_NGPUS, --ngpus   [1] */
  int verify;        /* 1: a solve the recurrence calls converged is reported
                        only once ||b - S x||_2 <= tol ||b||_2 holds for the
                        residual RECOMPUTED from x; if it does not, CG restarts
                        on the true residual (correction solve) until it does;
                        lsb_hip_result.true_relres carries the number      [0] */
  int cheb_degree;   /* LSB_PRECOND_CHEBYSHEV: degree of the polynomial, 1..32 [4] */
  int block_size;    /* LSB_PRECOND_BLOCKJACOBI: rows per diagonal block,
                        2, 4, 8, 16 or 32                                  [8] */
  int precision;     /* LSB_PREC_FP64, or LSB_PREC_MIXED: matrix values stored
                        and streamed as fp32, vectors and every accumulation
                        in fp64, fp64 iterative refinement around it -- the
                        same tolerance on the fp64 operator's residual   [FP64] */
  int persistent;    /* launch-bound operators (everything fits one XCD's L2):
                        the whole solve as ONE launch confined to one XCD;
                        1 on, 0 off, -1 = time both forms at solver creation
                        and keep the faster (which form runs then depends on
                        a timing: iterates differ in the last bits between
                        the forms).  Measured 2x slower than the two-launch
                        iteration on tests/xn3b_A_18.txt, hence             [0] */
  double comm_deadline_s; /* sharded solves: the host gives a poll of the device
                        state at most this long before it reports a hung
                        collective and exits non-zero                    [120] */
  int fsai_power;    /* LSB_PRECOND_FSAI: G lives on the pattern of tril(S^k),
                        k = 1..3 (rows of more than 128 pattern entries are cut
                        to the 128 nearest the diagonal)                    [3] */
  int blas1_nt;      /* which operands of the BLAS-1 sweeps are loaded nontemporal:
                        -1 = timed per solver at creation (tune_blas1_nt); else a mask
                        (bit 0 x, 1 p and q, 2 r in k_pcg_update_xr; 3 r, 4 p in
                        k_pcg_update_p; 5 k_cg1_update; 1 = all)              [-1] */
  /* LSB_PRECOND_AMG (lsb_amg.c, hip_amg_drv.c, hip_amg.hip).  amg_sweeps, amg_coarse and amg_max_levels are the
   * multigrid members: LSB_PRECOND_GMG reads these three too (nu, the row count at which coarsening stops, the level
   * cap) and ignores every other amg_* member */
  double amg_theta;  /* strength threshold: j strong for i when
                        |a_ij| >= theta sqrt(|a_ii a_jj|)                 [0.08] */
  int amg_sweeps;    /* l1-Jacobi sweeps before and after the coarse correction  [1] */
  int amg_coarse;    /* coarsening stops at this many rows (dense coarse solve) [256] */
  int amg_max_levels; /* levels at most, the coarsest included               [20] */
  int amg_tail_rows; /* levels of at most this many rows, and the coarse solve, run
                        in ONE launch of one workgroup (k_amg_tail); 0 = off, a launch
                        per step: measured faster at every size tried (one workgroup
                        is latency-bound; profiles/r05_amg.txt)                 [0] */
  int amg_precision; /* LSB_AMG_PREC_*: the precision of the V-cycle, whatever `precision`
                        says; under FP32 amg_tail_rows is ignored and the solver does
                        not serve blocks of columns; a hierarchy with an entry that does
                        not fit a float is refused at creation.  (It sits here, in what
                        was the alignment hole behind five ints: the size of the struct
                        and the offset of amg_cheb_ratio hold)                [FP64] */
  int amg_smoother;  /* LSB_AMG_SMOOTH_*; under CHEB amg_sweeps is the polynomial's
                        degree and amg_tail_rows is ignored (the one-launch tail is
                        not built for it); under MCGS amg_sweeps counts the forward
                        sweeps before and the backward sweeps after the coarse
                        correction, amg_tail_rows is ignored and the solver does not
                        serve blocks of columns                    [L1JACOBI] */
  double amg_cheb_ratio; /* hi / lo of the Chebyshev smoother's interval; values below
                        1.5 are taken as 1.5                                  [10] */
  /* The tail: members appended behind the ones above, so that none of their offsets moves.  An
   * anonymous struct -- they are members of lsb_hip_opts like the others (o.fsai_blocks) -- which
   * the Python mirror (_lib.Opts) keeps apart in the same way: its field list is the members above,
   * and tests pin that list's end and compare it with them. */
  struct {
    int fsai_blocks; /* LSB_PRECOND_FSAI: 1 = the solver serves blocks of right-hand sides
                        (solve_multi[_dev], solve_multi_x0_dev, precond_multi_dev) where it
                        is otherwise servable; its single-column paths are unchanged.  0: it
                        answers 2 on blocks and allocates nothing for them.  Ignored under
                        every other preconditioner.  A later change may flip the default  [0] */
  };
};
enum { LSB_PREC_FP64 = 0, LSB_PREC_MIXED = 1 };

struct lsb_hip_result {
  unsigned iters;        /* PCG iterations performed                        */
  int status;            /* LSB_STATUS_*                                    */
  double relres;         /* sqrt(r.r / b.b) of the recurrence residual      */
  double seconds;        /* wall-clock of this solve (host, after sync)     */
  double spmv_ms;        /* mean duration of the sampled SpMV launches      */
  unsigned spmv_samples; /* how many launches were sampled                  */
  unsigned corrections;  /* opts.verify / mixed precision: correction solves
                            (restarts on the recomputed residual) it took   */
  double true_relres;    /* ||b - S x|| / ||b|| recomputed from x (fp64
                            operator); -1 when not computed                 */
  unsigned spmvs;        /* multiplications by S the solve enqueued up to its
                            last iteration (outer iterations x (1 + Chebyshev
                            degree) + set-up ones)                          */
};

void lsb_hip_opts_default(struct lsb_hip_opts *o);
/* Options used by hip_cdna4_bench (which has no room for them in its
 * signature).  Also read from the environment at hip_cdna4_init:
 * LSBENCH_HIP_TOL, LSBENCH_HIP_MAXIT, LSBENCH_HIP_OPERATOR=raw|upper,
 * LSBENCH_HIP_NVIRT, LSBENCH_HIP_GRAPH, LSBENCH_HIP_SPMV. */
void lsb_hip_set_opts(const struct lsb_hip_opts *o);
void lsb_hip_get_opts(struct lsb_hip_opts *o);
/* Result of the last timed trial of the last hip_cdna4_bench call. */
void lsb_hip_last_result(struct lsb_hip_result *res);
int lsb_hip_device_count(void);

/* ------------------------------------------------------------------------ */
/* Host-side matrix helpers (no GPU needed)                                  */
/* ------------------------------------------------------------------------ */

/* Frees a CSR made by any helper below or by lsbench_matrix_synth (the three
 * arrays and the struct, like lsbench_matrix_free, src/lsbench-csr.c:101-108;
 * the backend library does not export the reference's own symbols). */
void lsb_csr_free(struct csr *A);
/* The operator CHOLMOD factorises, as a full 0-based CSR (both triangles):
 * restates the triplet construction of src/cholmod-impl.h:5-21.  Caller frees
 * with lsb_csr_free (or lsbench_matrix_free: same malloc'd layout). */
struct csr *lsb_csr_symmetrize_upper(const struct csr *A);
/* Deep copy with cols rebased to 0. */
struct csr *lsb_csr_copy_base0(const struct csr *A);
/* Rows [r0, r1) as a new CSR that keeps GLOBAL column ids (base 0 in, base 0
 * out): the shard one rank owns under 1-D row-range partitioning. */
struct csr *lsb_csr_row_slice(const struct csr *A, unsigned r0, unsigned r1);
/* Row-range partition balanced by non-zeros: bounds[0..nparts], with
 * bounds[0]=0, bounds[nparts]=nrows (prefix-sum split of offs). */
int lsb_csr_partition_rows(const struct csr *A, unsigned nparts,
                           unsigned *bounds);
/* Row blocks for the adaptive SpMV: consecutive rows are packed greedily into
 * blocks of at most `cap` non-zeros; a row longer than `cap` gets a block of
 * its own.  Returns the number of blocks and a malloc'd array of nblk+1 row
 * ids in *rowblk (caller frees with free()). */
unsigned lsb_csr_row_blocks(const struct csr *A, unsigned cap,
                            unsigned **rowblk);
/* Lanes per row (1..64, a power of two) the adaptive SpMV uses to add up the
 * rows of each block; lanes[] holds nblk entries. */
void lsb_csr_block_lanes(const struct csr *A, const unsigned *rowblk,
                         unsigned nblk, unsigned char *lanes);
/* Reverse Cuthill-McKee ordering of a structurally symmetric CSR:
 * perm[new] = old (cf. the host permutation Q of src/cusparse.c:67-85).
 * Returns 0, or 2 on allocation failure. */
/* Line padding of a constant-coefficient 2-D grid operator (0-based, sorted rows): grid lines of nx
 * rows re-numbered to start at multiples of `slice` rows, the gained rows holding the same stencil
 * among themselves (block-diagonal: real block = S).  map[new row] = row of S, or -1 for a pad
 * row (malloc'ed; free()).  NULL where S is no such operator (offsets out of {-nx, -1, 0, 1, nx}
 * with one value each, no +-1 entry across a line end), nx is a multiple of `slice` already, or
 * the padding would exceed 1/16 of the rows.  See lsb_operator.c. */
struct csr *lsb_csr_pad_lines(const struct csr *S, unsigned slice, unsigned *nx, unsigned *nxp, int **map);
int lsb_csr_rcm(const struct csr *S, unsigned *perm);
/* The direct solver's host side (lsb_direct.c, rules there; LSB_KRYLOV_DIRECT), pure host logic.
 * lsb_csr_nd: a nested-dissection ordering of a structurally symmetric pattern, perm[new] = old, by recursive
 * bisection along the smallest BFS level that leaves both sides 30 % of the part.  Returns 0 and a permutation for
 * any input (disconnected graphs, rows that hold only their diagonal, n = 1), 2 on allocation failure.
 * lsb_csr_nd_bounded: the same, but gives up with 3 as soon as the entries of W this ordering cannot avoid -- n + the
 * sum of |side below| |separator| over its bisections, *lower -- exceed `budget`; perm is then a permutation still,
 * only not a finished ordering. */
int lsb_csr_nd(const struct csr *S, unsigned *perm);
int lsb_csr_nd_bounded(const struct csr *S, unsigned *perm, unsigned long long budget, unsigned long long *lower);
/* Entries of W = L^-1 for P S P^T = L L^T: the sum over the columns of their depth in the elimination tree (a root
 * has depth 1), symbolic -- Liu's algorithm with path compression, no numeric work; *height (may be NULL): the
 * deepest column.  0 when perm is no permutation or memory runs out. */
unsigned long long lsb_csr_skyline_count(const struct csr *S, const unsigned *perm, unsigned *height);
/* The inverse factor as a skyline.  perm is perm_in composed with a postorder of its elimination tree (perm[new] =
 * old), in which the subtree of k is the run of indices first[k] .. k; row k of W is exactly that run of columns,
 * dense, at vals[woff[k] .. woff[k] + k - first[k]] -- no column indices.  parent[k]: the tree (n on a root);
 * run_end[k]: the last index of the maximal run k, k + 1, ... in which parent(i) = i + 1, so that a walk to the root
 * is a few dozen jumps.  x = P^T W^T W P b solves S x = b.  NULL with *why (may be NULL) = 1: a pivot <= 0 or not
 * finite (S is not symmetric positive definite), 2: more than LSB_DIRECT_MAX_ENTRIES entries, 3: out of memory or
 * perm_in is no permutation. */
#define LSB_DIRECT_MAX_ENTRIES (1ull << 28) /* 2 GB of doubles: operators of a few thousand to a few tens of
                                               thousands of rows */
struct lsb_skyinv {
  unsigned n;
  unsigned *perm, *first;
  unsigned long long *woff; /* n + 1 */
  double *vals;
  unsigned *parent, *run_end;
};
struct lsb_skyinv *lsb_csr_skyline_inverse(const struct csr *S, const unsigned *perm_in, int *why);
void lsb_skyinv_free(struct lsb_skyinv *W);
/* The inverse factor in tiers, for operators whose single skyline is over the budget (lsb_direct.c).  With the
 * thresholds T_1 < ... < T_(m-1), T_i the smallest integer with T_i^m >= n^i, tier(k) is the number of thresholds the
 * subtree of k is larger than; tiers never decrease towards the root, tiers nobody is in are dropped (ntier <= m), and
 * the rows are numbered tier by tier, in postorder inside a tier: tier t is lo[t] .. lo[t + 1] - 1, lo[ntier] = n.  L
 * is then block lower triangular.  W_tt = (L_tt)^-1 are skylines as in struct lsb_skyinv, one after another in the
 * same arrays: row k is the run of columns first[k] .. k >= lo[tier(k)], parent[k] = n on the root of a tier's tree,
 * run_end[k] stays inside k's tier.  The blocks below the diagonal are the rows of L themselves, twice: C by rows --
 * row i >= lo[1] at coffs[i - lo[1]] .. coffs[i - lo[1] + 1], columns < lo[tier(i)] ascending -- and C^T by tier and
 * column -- for t = 1 .. ntier - 1 the columns j < lo[t], lo[t] + 1 offsets each, tier t's at toffs[sum over
 * 1 <= s < t of (lo[s] + 1)], the rows of tier t ascending.  Both hold the same values bit for bit.  A solve is
 *   forward   y_t = W_tt ((P b)_t - C_t y_<t)                 t = 0 .. ntier - 1
 *   backward  x_t = W_tt^T (y_t - sum over s > t of (C_s^T x_s)_t)   t = ntier - 1 .. 0, then x = P^T x.
 * The budget: w_entries + 3 coupling_entries <= LSB_DIRECT_MAX_ENTRIES (a coupling entry is kept twice at 12 B).
 * lsb_csr_tiered_count: symbolic, O(nnz(L)): the entries of the W_tt, of C, and the height of the whole tree, for
 * tiers = 1 .. LSB_DIRECT_MAX_TIERS; returns 0, 2 for tiers out of range or a perm that is none, 3 out of memory.
 * lsb_csr_tiered_inverse: tiers = 1 is lsb_csr_skyline_inverse's factor byte for byte with nothing coupled; tiers = 0
 * takes the fewest tiers that fit the budget by the symbolic count (LSB_DIRECT_MAX_TIERS if none does, which is then
 * refused with 2); *why as for lsb_csr_skyline_inverse, 3 also for tiers > LSB_DIRECT_MAX_TIERS. */
#define LSB_DIRECT_MAX_TIERS 6
struct lsb_tierinv {
  unsigned n, ntier;
  unsigned lo[LSB_DIRECT_MAX_TIERS + 1];
  unsigned *perm, *first;
  unsigned long long *woff; /* n + 1 */
  double *vals;
  unsigned *parent, *run_end;
  unsigned *coffs, *ccols; /* C: n - lo[1] + 1 offsets (1 when ntier = 1) */
  double *cvals;
  unsigned *toffs, *tcols; /* C^T, tier by tier */
  double *tvals;
};
struct lsb_tierinv *lsb_csr_tiered_inverse(const struct csr *S, const unsigned *perm_in, unsigned tiers, int *why);
void lsb_tierinv_free(struct lsb_tierinv *W);
int lsb_csr_tiered_count(const struct csr *S, const unsigned *perm, unsigned tiers, unsigned long long *w_entries,
                         unsigned long long *coupling_entries, unsigned *height);
/* P S P^T for perm[new] = old, as a new 0-based CSR (src/cusparse.c:87-97). */
struct csr *lsb_csr_permute_sym(const struct csr *S, const unsigned *perm);
/* max |row - col| over the stored entries */
unsigned lsb_csr_bandwidth(const struct csr *S);
/* Column-panel form of a CSR (for scattered operators): the (row, panel) pairs
 * of panel-major order as the rows of one CSR.  See lsb_csr_panelize. */
struct lsb_panel_csr {
  unsigned npanels, width, npairs, nrows;
  unsigned *pair_begin; /* npanels+1: first pair of each panel            */
  unsigned *pair_row;   /* npairs: original row of each pair              */
  unsigned *offs;       /* npairs+1 into cols/vals                        */
  unsigned *cols;       /* 0-based global column ids, panel-major copy    */
  double *vals;
};
struct lsb_panel_csr *lsb_csr_panelize(const struct csr *A, unsigned width);
void lsb_panel_csr_free(struct lsb_panel_csr *P);
/* Binned form of a CSR for LSB_SPMV_BINNED (scattered operators: the gather of a
 * row strays over far more of x than an XCD's 4 MiB L2 holds, so a row-major
 * sweep fetches a 128-byte line per non-zero).  The entries are binned by column
 * panel -- `width` consecutive columns, an L2-sized window of x -- and sorted by
 * row inside a bin (column order inside a row is kept); a bin is streamed as
 * (row, col, value) triplets and every lane does the same work whatever the row
 * lengths are.  A bin is cut into CHUNKS of whole (row, bin) runs holding at
 * most LSB_BIN_CHUNK entries (a longer run is a chunk of its own), so that
 * exactly one workgroup adds to a given y entry per bin: no atomics, results
 * bit-identical from run to run. */
#define LSB_BIN_CHUNK 2048
struct lsb_binned {
  unsigned nbins, width, nrows, nchunks;
  unsigned chunk_cap;    /* entries a chunk holds at most: LSB_BIN_CHUNK, or 1024 /
                            1536 / 2048 from LSBENCH_HIP_BIN_CHUNK (tuning)   */
  unsigned long long nnz;
  unsigned *bin_chunk;   /* nbins+1: first chunk of each bin                */
  unsigned *chunk_begin; /* nchunks+1: first entry of each chunk            */
  unsigned *rows;        /* nnz: row of each entry (local to A)             */
  unsigned *cols;        /* nnz: 0-based column                             */
  double *vals;
};
/* NULL when A or width is unusable, or the copy does not fit 32-bit offsets. */
struct lsb_binned *lsb_csr_binize(const struct csr *A, unsigned width);
void lsb_binned_free(struct lsb_binned *B);
/* Two-phase form of a CSR for LSB_SPMV_TWOPHASE (scattered operators; "propagation
 * blocking"): no gather ever leaves a compute unit.
 *   phase 1  the entries are cut by COLUMN into chunks of `cols` columns; a
 *            workgroup copies its chunk's window of x into LDS (8 * cols bytes)
 *            and streams its entries -- value (8 B), column inside the window
 *            (2 B) -- writing each product into the product array;
 *   phase 2  the product array is ROW-BIN major (`rows` rows per bin): a WAVEFRONT
 *            owns a bin, streams its slots -- product (8 B) + row inside the bin
 *            (2 B) -- and adds them into its LDS copy of the bin's rows
 *            (ds_add_f64, the wavefront's own 8 * rows bytes: nobody else touches
 *            them, so the order of the additions is the wavefront's program
 *            order), then writes the rows of y, coalesced.
 * Both orders keep the entries of one (chunk, bin) pair -- a PIECE -- together and in
 * the same order, chunk-major for phase 1 and bin-major for phase 2, so the slot of
 * a product is its entry index plus a per-piece constant (`delta`); which piece an
 * entry belongs to is read off two words per group of 64 entries (`grp_first`,
 * `grp_mask`).  The entries of a chunk start on a multiple of 64 (vals = 0 in the
 * gaps, never read).  18.2 B read/written per non-zero in phase 1, 10 B in phase 2,
 * instead of a 128-byte line per gather. */
#define LSB_PB_COLS 8192 /* defaults; LSBENCH_HIP_PB_COLS / _ROWS (<= 16384 / <= 4096) */
#define LSB_PB_ROWS 2048
struct lsb_pb {
  unsigned nrows, ncols_lo, nchunks, nbins, nitems, npieces;
  unsigned cols, rows;     /* chunk width (columns), bin height (rows)          */
  unsigned long long nnz;  /* = slots of the product array                      */
  unsigned long long nent; /* length of the phase-1 arrays (a multiple of 64)   */
  double *vals;            /* nent, in (chunk, bin, row, col) order             */
  unsigned short *colw;    /* nent: column - (ncols_lo + chunk * cols)          */
  unsigned *grp_first;     /* nent / 64: piece of the group's first entry       */
  unsigned long long *grp_mask; /* nent / 64: bit j > 0: entry j starts a piece */
  unsigned *delta;         /* npieces: slot - entry index, mod 2^32             */
  unsigned *item;          /* 3 * nitems: {chunk, first entry, end entry} of
                              the phase-1 work items                            */
  unsigned *bin_ptr;       /* nbins + 1: first slot of each bin                 */
  unsigned short *roww;    /* nnz: row - bin * rows, in slot order              */
};
/* cols, rows: 0 = the defaults */
struct lsb_pb *lsb_csr_pbize2(const struct csr *A, unsigned cols, unsigned rows);
struct lsb_pb *lsb_csr_pbize(const struct csr *A);
void lsb_pb_free(struct lsb_pb *P);
/* Host-side assertions of the bounds the two kernels rely on: every index they form against
 * arrays of prod_len / roww_len slots as the caller allocated them (the backend allocates
 * nnz + 2).  0 = all hold; else a code, and the violated rule in why[whylen].  deep: also
 * every entry's 16-bit offsets.  Run at every upload (shallow) and under ASan (deep). */
int lsb_pb_check(const struct lsb_pb *P, unsigned long long prod_len, unsigned long long roww_len, int deep,
                 char *why, size_t whylen);
/* Pattern of the factorised sparse approximate inverse (LSB_PRECOND_FSAI): row i holds the
 * columns j <= i that row i of S^power reaches (S taken as a graph: its stored pattern, both
 * triangles, diagonal included), cut to the `cap` largest (nearest the diagonal) where there
 * are more; sorted, the diagonal last.  offs[n+1], cols[offs[n]]; pure host logic. */
struct lsb_fsai_pattern {
  unsigned n, cap;
  unsigned long long nnz;
  unsigned *offs, *cols;
};
#define LSB_FSAI_CAP 128
struct lsb_fsai_pattern *lsb_csr_fsai_pattern(const struct csr *S, int power, unsigned cap);
void lsb_fsai_pattern_free(struct lsb_fsai_pattern *P);
/* Smoothed-aggregation AMG hierarchy (LSB_PRECOND_AMG), pure host logic (lsb_amg.c, rules
 * there).  lv[0].A = S as a 0-based CSR with sorted columns; level l < nlev - 1 has P
 * (n x n_next) and R = P^T; the coarsest level lv[nlev - 1] has neither and is solved by
 * coarse_inv (nc x nc, row-major, symmetric).  Every level's rows have sorted columns.  An
 * operator that is not SPD (a diagonal <= 0 on some level, a coarse pivot <= 0) makes it exit
 * with a "positive definite" message. */
struct lsb_amg_level {
  unsigned n;
  struct csr *A, *P, *R;
};
struct lsb_amg_hier {
  unsigned nlev;
  struct lsb_amg_level *lv;
  unsigned nc;
  double *coarse_inv;
};
struct lsb_amg_hier *lsb_amg_setup(const struct csr *S, double theta, unsigned coarse, unsigned max_levels);
/* the aggregates of one level (malloc'ed, n entries; -1 = not aggregated), *naggr of them */
int *lsb_amg_aggregate(const struct csr *A, double theta, unsigned *naggr);
/* max_i sum_j |a_ij| / a_ii >= lambda_max(D^-1 A): the bound behind the prolongator's omega and the upper
 * end of the Chebyshev smoother's interval.  Deterministic (no eigen-iteration). */
double lsb_amg_gershgorin(const struct csr *A);
/* Coefficients of the Chebyshev smoother of degree deg on [hi / ratio, hi] (ratio < 1.5 is taken as 1.5);
 * c1, c2: deg doubles each.  Step k (0 .. deg - 1) on (x, d), s = A x:
 *   d_i <- fma(c2[k] / a_ii, b_i - s_i, c1[k] d_i),  x_i <- x_i + d_i ;  c1[0] = 0 and step 0 does not read d. */
void lsb_amg_cheb_coeffs(double hi, double ratio, unsigned deg, double *c1, double *c2);
void lsb_amg_free(struct lsb_amg_hier *h);
/* Geometric multigrid on grids (LSB_PRECOND_GMG), pure host logic (lsb_gmg.c, rules there).
 * lsb_gmg_detect: 0 when S (any base) is a constant-coefficient grid operator -- row (k ny + j) nx + i holds exactly a
 * diagonal a and -c at each grid neighbour that exists, c > 0, a == 2 dim c, nx, ny [, nz] >= 2 -- and then *g is the
 * grid (n[d] = 1 beyond dim); else the number of the rule it breaks: 1 fewer than 4 rows, 2 the pattern, 3 the
 * off-diagonal value, 4 the diagonal.
 * lsb_gmg_plan: the levels, lv[0] the grid itself with delta = 1; coarse points at the fine indices 2 j + 1, so
 * n' = n / 2, delta' = delta / 2 (n even) or (1 + delta) / 2 (n odd), all dimensions together; stops at <= coarse
 * rows, when some n_d < 4, or at max_levels (at most cap, the length of lv).  Returns the number of levels, -1 when the
 * coarsest level would have more than LSB_GMG_COARSE_MAX rows (a very thin grid), -2 for a bad argument. */
#define LSB_GMG_MAX_LEVELS 32
#define LSB_GMG_COARSE_MAX 4096
struct lsb_gmg_grid {
  unsigned dim, n[3];
  double c;
};
struct lsb_gmg_level {
  unsigned n[3];
  double delta[3]; /* distance from the last point to the far boundary, in the level's spacing */
};
int lsb_gmg_detect(const struct csr *S, struct lsb_gmg_grid *g);
int lsb_gmg_plan(const struct lsb_gmg_grid *g, unsigned coarse, unsigned max_levels, struct lsb_gmg_level *lv,
                 unsigned cap);
/* Multicolour Gauss-Seidel smoothing (LSB_AMG_SMOOTH_MCGS), pure host logic.
 * lsb_amg_colour: the greedy colouring of A's stored pattern -- rows in ascending order, each takes the smallest
 * colour that none of its stored off-diagonal neighbours already holds (a stored zero counts); serial, so the same
 * for any thread count.  A malloc'ed int[nrows] (at least one), the number of colours in *ncolours. */
#define LSB_AMG_MCGS_COLOURS 16 /* a level with more colours keeps l1-Jacobi; LSBENCH_HIP_AMG_MCGS_COLOURS, 1 .. 64 */
int *lsb_amg_colour(const struct csr *A, unsigned *ncolours);
/* The colour-sorted copy of a level's matrix: its rows regrouped colour by colour, ascending row order inside a
 * colour (stable), so that the launch of colour c streams the contiguous rows cbeg[c] .. cbeg[c + 1) of the copy.
 * rowid[p] is the row at position p; offs / cols / vals are the rows in that order, entry for entry, columns
 * 0-based and in the level's numbering (the vectors are not permuted). */
struct lsb_mcgs {
  unsigned n, ncolours;
  unsigned *cbeg;  /* ncolours + 1 */
  unsigned *rowid; /* n */
  unsigned *offs;  /* n + 1 */
  unsigned *cols;  /* offs[n] */
  double *vals;
};
/* NULL when a colour is outside 0 .. ncolours - 1 */
struct lsb_mcgs *lsb_csr_mcgs(const struct csr *A, const int *colour, unsigned ncolours);
void lsb_mcgs_free(struct lsb_mcgs *M);
/* Host-side assertions of what the in-place kernels rely on, run at every upload.  0 = all hold; else the number
 * of the violated rule and its text in why[whylen]: 2 the colour ranges cover 0 .. n and ascend; 3 rowid is a
 * permutation; 4 every row lies in the range of its own colour (so in exactly one); 5 columns are rows of the
 * level; 6 every stored a_ij, i != j, has colour[i] != colour[j] (looked for in every row, so an unsymmetric
 * pattern is caught); 7 every diagonal is > 0; 8 the copy's rows are the original rows entry for entry. */
int lsb_mcgs_check(const struct csr *A, const int *colour, const struct lsb_mcgs *M, char *why, size_t whylen);
/* The entries of a CSR as the fp32 V-cycle streams them: a malloc'ed array of offs[nrows] 8-byte words (at least
 * one), word j = the 0-based column of entry j in the low 32 bits, the bit pattern of (float)vals[j] (round to
 * nearest even) in the high 32.  NULL when a value is not finite or rounds to +-inf; subnormal results are kept.
 * The caller frees with free(). */
unsigned long long *lsb_csr_pack_f32(const struct csr *A);
/* Sliced-ELL copy of a CSR for LSB_SPMV_SELL: rows in slices of LSB_SELL_ROWS,
 * every slice padded to its longest row and stored column-major (entry j of
 * row 128s+i at sptr[s] + 128j + i), so that a wavefront's lane l reads the
 * j-th entries of rows 2l and 2l+1 as one int2 / double2.  Padding entries
 * carry value 0 and the row's last column (a column the row references anyway).
 * cols are 0-based whatever A->base is. */
#define LSB_SELL_ROWS 128
struct lsb_sell {
  unsigned nrows, nslice;
  unsigned long long stored; /* entries incl. padding = sptr[nslice]        */
  unsigned *sptr;            /* nslice+1                                    */
  int *cols;                 /* stored (+ LSB_SELL_ROWS slack); NULL in the
                                16-bit form                                 */
  double *vals;
  /* 16-bit form (lsb_csr_sellize16): column of the entry in slot j of row r =
   * r + row_begin + base + code with {base, k} = sbase[2q], sbase[2q+1],
   * q = sptr[s]/128 + j; k >= 0: the slot's 128 codes are codes[128k ..);
   * k = -1: all its live entries share one code, which has been folded into
   * the base (every slot of a structured-grid operator).  A slot of a slice holds
   * entries of ONE diagonal band (+-32767 around its base), so a row's entries
   * may be interleaved with padding (value 0: the kernel does not gather for
   * those).  Entries of a row keep their column order. */
  short *codes;              /* 128 * ncode_slots, or NULL in the 32-bit form */
  int *sbase;                /* 2 * stored / LSB_SELL_ROWS                  */
  unsigned ncode_slots;
};
/* entries a sliced-ELL copy of A would store (to decide before building it) */
unsigned long long lsb_csr_sell_stored(const struct csr *A);
/* NULL when the copy would not fit 32-bit offsets */
struct lsb_sell *lsb_csr_sellize(const struct csr *A);
/* The 16-bit form, 10 instead of 12 bytes per entry; row_begin = global index
 * of A's first row (column ids are global).  NULL when some slice would need
 * more than 255 slots or the copy does not fit 32-bit offsets. */
struct lsb_sell *lsb_csr_sellize16(const struct csr *A, unsigned row_begin);
void lsb_sell_free(struct lsb_sell *S);
/* Constant slots of the 16-bit form: a slot whose 128 values are one and the same
 * non-zero number -- a diagonal of a constant-coefficient stencil inside a slice, unit
 * weights of a graph Laplacian -- needs no value array.  slots[4q .. 4q+3] = {base, code
 * slot or -1 (as sbase), VALUE slot or -1, 0}; vconst[q] = the slot's value where the
 * value slot is -1; vals holds the nval_slots remaining slots' 128 values, packed in slot
 * order.  Lossless: the kernel forms the same products in the same order. */
struct lsb_sell_vc {
  unsigned long long nslots; /* = stored / LSB_SELL_ROWS of the copy it was made from */
  unsigned nval_slots;
  int *slots;     /* 4 * (nslots + 1) */
  double *vconst; /* nslots + 1 */
  double *vals;   /* (nval_slots + 1) * LSB_SELL_ROWS */
};
struct lsb_sell_vc *lsb_sell16_value_slots(const struct lsb_sell *S);
void lsb_sell_vc_free(struct lsb_sell_vc *V);
/* Slice TEMPLATES of the constant-slot layout.  A code-free slice is described by its slots'
 * {base, constant or "keeps its values"} records, and on a structured grid a handful of such
 * descriptions cover everything: slices with identical records share ONE template, tid[slice]
 * says which (255 = none: the slice goes the per-slot way) and vbase[slice] where the slice's
 * kept value slots start (they are consecutive: the k-th kept slot of the slice is value slot
 * vbase + k).  The device copy packs {tid, vbase, first mask, 0} into ONE 16-byte record per slice
 * (a single scalar load); the kernel then reads that and the template out of the scalar cache
 * instead of 24 bytes of cold records per slot.  Where a template holds a slot c with
 * base[c-1] = base[c]-1 and base[c+1] = base[c]+1 (the three inner diagonals of a stencil) it
 * is SHAPED: [nfar far slots][c-1, c, c+1][nfar far slots] with the set's one nfar -- lanes
 * take the operands of c-1 and c+1 from the centre's 16-byte pair by a lane shift: three
 * gathers instead of five on a 5-point row, none misaligned.  In a shaped template the far
 * slots and the centre are constant; c-1 and c+1 may keep their values (a grid line that
 * ends inside the slice: padding zeros there) -- and where those values are ONE number or
 * zero (every such slot of a constant-coefficient stencil), the slot is MASKED: the number
 * in the template, a 128-bit mask per slice and slot instead of 1 KB of values.  Every other
 * template is all-constant.  Lossless: the same products in the same order. */
#define LSB_TMPL_SLOTS 8
struct lsb_sell_tmpl { /* 176 bytes, read by scalar loads */
  int nslots;
  int shaped; /* 1: [nfar][c-1, c, c+1][nfar], nfar = the set's */
  int base[LSB_TMPL_SLOTS];
  int kidx[LSB_TMPL_SLOTS]; /* -1: constant cst[j]; k >= 0: the slice's k-th kept value slot
                               (kind 1) or k-th mask (kind 2) */
  int kind[LSB_TMPL_SLOTS]; /* 0 constant, 1 keeps its 128 values, 2 masked constant cst[j] */
  int pad_[2];
  double cst[LSB_TMPL_SLOTS];
};
struct lsb_sell_tmpls {
  unsigned nslice, ntmpl, nfar;
  unsigned long long covered, shaped; /* slices that have a template / a shaped one */
  unsigned long long nmask;           /* masks (two 64-bit words each: bit r = row r of the slice) */
  unsigned long long kept_read;       /* value slots the template kernel still reads (kind 1 slots
                                         of templated slices + the slices without a template) */
  unsigned char *tid;                 /* nslice + 8 */
  unsigned *vbase;                    /* 2 * (nslice + 8): {first kept value slot, first mask} */
  unsigned long long *mask;           /* 2 * (nmask + 1) */
  struct lsb_sell_tmpl *t;            /* ntmpl <= 254 */
};
/* NULL when fewer than 7/8 of the slices get a template, shaped ones cover less than 3/4,
 * or the copy has code slots (not a structured grid). */
struct lsb_sell_tmpls *lsb_sell16_templates(const struct lsb_sell *S, const struct lsb_sell_vc *V);
void lsb_sell_tmpls_free(struct lsb_sell_tmpls *T);
/* Host-side check of the bounds k_spmv_sell16's constant-slot path and k_spmv_tmpl rely on (their
 * unguarded 16-byte gathers; value-slot, mask and template indices), for the shard whose first
 * global row is row_begin, that holds nrows rows and gathers from a vector of xlen entries.  0 =
 * every rule holds; else a rule number, the rule in `why`.  T may be NULL (no templates).  Run by
 * the backend at every upload; deep != 0 also walks values and masks. */
int lsb_tmpl_check(const struct lsb_sell *S, const struct lsb_sell_vc *V, const struct lsb_sell_tmpls *T,
                   unsigned row_begin, unsigned nrows, unsigned xlen, int deep, char *why, size_t whylen);
/* Z-COLUMNS of the template layout (k_spmv_tmpl_col).  On a 3-D stencil whose planes are whole
 * slices (period = slices per plane) the outermost far slots of a shaped template reach exactly
 * one plane down and up: base[0] = base[c] - 128 period, base[last] = base[c] + 128 period.  The
 * operand pair a lane gathers for slot 0 of slice s + period is then the very pair it gathered for
 * the centre of slice s, and the centre pair of s + period is what slot `last` of s asked for: a
 * wavefront that walks s, s + period, s + 2 period, ... keeps three centre pairs in registers and
 * gathers ONE new plane per step instead of three.  A column is a run of 2..kmax such slices that
 * share one template and one set of mask words (the host checks it: every interior z-column of a
 * structured grid qualifies), so the template and the masks are looked at once per column.
 * Everything else -- first / last plane, slices that keep values, ragged ends -- is an item of
 * one slice and goes slot by slot off the slot records.
 * item[4i..4i+3] = {first slice, slices (1: a single slice; >= 2: a column), template id, first
 * mask}; the items run z-group after z-group (at most kmax planes each, as equal as they come),
 * positions ascending, and XCD k takes [xbeg[k], xbeg[k+1]): a contiguous run with an eighth of the
 * slices -- a band of planes.
 * Lossless: the same operands and products in the same order as k_spmv_tmpl / k_spmv_sell16.
 * WALK DIRECTION: a column re-reads the plane below its first slice and the plane above its last, and
 * the column next to it in z owns that plane.  Walked upward both, column g asks for its bottom halo at
 * step 0 and column g - 1 for the same plane at its last step: by then the L2 has turned over.  Where a
 * z-group's neighbours are dealt into the same turn of the workgroups (2 period <= the items an XCD
 * takes per turn, LSB_TMPL_COL_TURN), the z-groups of odd index walk DOWNWARD: two neighbouring columns
 * then touch their shared planes at the same step.  down[i / 32] bit i % 32 = item i is walked from its
 * top slice down (= the parity of its z-group, for columns of >= 3 slices: the PCG kernels take shorter
 * items slice by slice, upward, and the SpMV forms the same dot partials as they do); down = NULL: every
 * item upward.  The items themselves
 * are the same either way; the device plan carries the bits behind the items (LSB_TMPL_COL_DOWN). */
#define LSB_TMPL_COL_MAX 16
/* the resident grid of the two-launch PCG kernels (lsb_k_pcg_col_px / _r) and the items an XCD takes per turn
 * of it (4 waves per workgroup, 8 XCDs) -- what the walk directions are planned against */
#define LSB_TMPL_COL_GRID(nfar) ((nfar) >= 2 ? 768u : 1280u)
#define LSB_TMPL_COL_TURN(nfar) (4u * LSB_TMPL_COL_GRID(nfar) / 8u)
/* the sliced-ELL, template and z-column SpMV launchers' grid where none is asked for */
#define LSB_SELL_GRID 1536u
/* the device plan: xbeg[9] at [0, 9), [LSB_TMPL_COL_DOWN] = the offset in words of the direction bits
 * (0: none), the items from word 16, the bits behind them */
#define LSB_TMPL_COL_DOWN 9
#define LSB_TMPL_COL_LOCKSTEP 0x80000000u /* bit 31 of an item's slice count: the four items of a workgroup's
                                             turn are columns of one length (a barrier per plane keeps them in step) */
struct lsb_tmpl_cols {
  unsigned nitem, kmax, period;
  unsigned s_lo, s_hi;          /* the slices the items cover: [s_lo, s_hi) */
  unsigned xbeg[9];
  unsigned *item;               /* 4 * (nitem + 1) */
  unsigned long long in_cols;   /* slices inside columns (the rest are single items) */
  int centre0;                  /* every column's centre slot has base 0 (the diagonal): where the fused
                                   dot is with the gathered vector itself, the centre pair is its operand */
  unsigned *down;               /* (nitem + 31) / 32 words: bit i = item i walks downward; NULL: none does */
};
/* NULL where the layout has no such columns (period < 8, no shaped template with plane-reaching
 * far slots) or fewer than 3/4 of the slices fall inside columns. */
struct lsb_tmpl_cols *lsb_sell_tmpl_columns(const struct lsb_sell_tmpls *T, unsigned period, unsigned kmax);
/* the same for the slices [s_lo, s_hi) only (the interior launch of a sharded SpMV that runs while
 * the halo travels): every slice of the range in exactly one item, none outside it */
struct lsb_tmpl_cols *lsb_sell_tmpl_columns_range(const struct lsb_sell_tmpls *T, unsigned period, unsigned kmax,
                                                  unsigned s_lo, unsigned s_hi);
void lsb_tmpl_cols_free(struct lsb_tmpl_cols *C);
/* The rules k_spmv_tmpl_col relies on, as host assertions (run at every upload): every slice in
 * [s_lo, s_hi) in exactly one item, none outside; a column's slices s + k period share the item's template -- shaped,
 * constant or masked slots only, outermost far slots one plane away -- and its mask words bit
 * for bit; with direction bits, only where the deal allows them and every item's bit the parity of its
 * z-group (0 for items of fewer than 3 slices).  0 or a rule number with the rule in `why`. */
int lsb_tmpl_cols_check(const struct lsb_sell_tmpls *T, const struct lsb_tmpl_cols *C, char *why, size_t whylen);
/* mean |col - (row + row_begin)| over a sample of the rows */
double lsb_csr_mean_scatter(const struct csr *A, unsigned row_begin);
/* [lo,hi) column range referenced by A (0-based). */
void lsb_csr_col_hull(const struct csr *A, unsigned *lo, unsigned *hi);
/* One contiguous range [offset, offset+count) (in doubles) of the exchanged
 * vector, to or from shard/rank `peer`. */
struct lsb_xfer {
  int peer;
  size_t offset, count;
};
/* Exchange plan of shard `me` out of `nall`, from the table
 * hull[4q..4q+3] = {row_begin, nrows, col_lo, col_hi}; recv/send hold nall
 * entries.  Pure host logic (tested on the CPU with gloo ranks). */
void lsb_plan_exchange(int me, int nall, const unsigned *hull,
                       struct lsb_xfer *recv, int *nrecv,
                       struct lsb_xfer *send, int *nsend);
/* Synthetic operators (BASELINE.json configs 3-5), rows [r0,r1) only, global
 * 0-based column ids, generated on the host.  spec:
 *   "lap2d:nx=3162,ny=3162"          5-point Laplacian, diag 4, off -1
 *   "lap3d:nx=400,ny=400,nz=400"     7-point Laplacian, diag 6, off -1
 *   "lap2d:...,coef=K" / "lap3d:...,coef=K" (K != 0)  same pattern, GENERAL values: one
 *                                    weight in [1/2, 3/2) per grid edge from a counter-
 *                                    based hash keyed by K, diagonal = sum of the row's
 *                                    edge weights (Dirichlet) -- SPD, nothing to elide
 *   "powerlaw:n=8000000,avg=32,max=4096,seed=20240607[,spd=1]"
 * r1 = 0 means "to the last row".  *n_global receives the full row count. */
struct csr *lsbench_matrix_synth(const char *spec, unsigned r0, unsigned r1,
                                 unsigned *n_global);

/* ------------------------------------------------------------------------ */
/* 2. Solver handle: operator resident in HBM, repeated solves               */
/* ------------------------------------------------------------------------ */

typedef struct lsb_hip_solver lsb_hip_solver;

/* Whole matrix on this process' device (or on o->nvirt virtual shards of it).
 * Applies o->op_mode.  Untimed setup: counterpart of csr_init
 * (src/cusparse.c:47-125, src/cholmod-impl.h:1-32). */
lsb_hip_solver *lsb_hip_solver_create(const struct csr *A,
                                      const struct lsb_hip_opts *o);
/* One rank's shard of a row-partitioned operator: rows
 * [row_begin, row_begin + A_rows->nrows) with GLOBAL 0-based column ids, used
 * as-is (LSB_OP_RAW).  Collective over the communicator set up by
 * lsb_hip_comm_init_rank; every rank must call it. */
lsb_hip_solver *lsb_hip_solver_create_dist(const struct csr *A_rows,
                                           unsigned row_begin,
                                           unsigned n_global,
                                           const struct lsb_hip_opts *o);
void lsb_hip_solver_destroy(lsb_hip_solver *s);

/* One solve from x0 = 0.  Host buffers, local rows only (length n_local);
 * H2D of b and D2H of x are outside res->seconds. */
int lsb_hip_solver_solve(lsb_hip_solver *s, const double *b, double *x,
                         struct lsb_hip_result *res);
/* Same with device-resident b and x (length n_local each). */
int lsb_hip_solver_solve_dev(lsb_hip_solver *s, const double *d_b, double *d_x,
                             struct lsb_hip_result *res);
/* The same solve from an initial guess: d_x (x) holds x0 on entry and the solution on return.  Every solver that
 * solve[_dev] serves is served -- every Krylov method, preconditioner and PCG form, the persistent one-launch solve,
 * mixed precision, re-numbered and line-padded solvers, shards: q = S x0 is formed the way a recomputed residual is,
 * one sweep leaves r0 = b - q with r0.r0 and b.b, the solver's own driver solves S e = r0 from e = 0, x = x0 + e.
 * The stop rule stays relative to ||b||, never to ||b - S x0||: the run stops at ||r|| <= tol ||b||, res->relres is
 * relative to ||b||, res->iters counts the iterations run from x0 and opts.maxit caps them; opts.verify and the
 * refinement of LSB_PREC_MIXED work on the recomputed b - S x as in a cold solve (under BiCGSTAB and Richardson
 * through correction solves S e = b - S x, where their cold solve restarts in place; GMRES recomputes nothing).
 * opts.verify here forms b - S x off the CSR arrays as in twice the working precision: true_relres is good to 1e-3
 * of itself down to the rounding level of an fp64 product, where the cold solve's fp64 value is not.
 *   b = 0: x = 0, CONVERGED, 0 iterations -- the cold rule, whatever x0 holds.
 *   ||b - S x0|| <= tol ||b|| with tol > 0: CONVERGED, 0 iterations, x is x0 untouched, bit for bit.
 *   x0 = 0: x, iters, status and relres of solve[_dev] (x compares equal; the sign of a zero may differ).  With
 *   opts.verify the two recompute b - S x differently (below): x, iters and status are still the cold solve's as
 *   long as neither needs a correction run, relres = true_relres differ by the rounding of the cold solve's fp64
 *   residual, at most (len + 2) 2^-53 || |S||x| + |b| || / ||b|| with len the longest row; where a recomputed
 *   residual sits that close to tol, one of the two may run a correction the other does not.
 * Return codes as for solve[_dev]; 2 leaves x untouched.  res->spmvs counts the product S x0. */
int lsb_hip_solver_solve_x0(lsb_hip_solver *s, const double *b, double *x,
                            struct lsb_hip_result *res);
int lsb_hip_solver_solve_x0_dev(lsb_hip_solver *s, const double *d_b, double *d_x,
                                struct lsb_hip_result *res);
/* ||b_c - S x0_c|| / ||b_c|| of the columns of the last solve, if that was one from an initial guess (solve_x0[_dev]:
 * nrhs = 1; solve_multi_x0_dev: its nrhs); 0 where b_c = 0.  Accuracy: a single solve forms b - S x0 with the solver's
 * fp64 SpMV, so its value (and the decision ||b - S x0|| <= tol ||b||) carries an absolute error of about
 * 2^-53 || |S||x0| + |b| || / ||b|| -- a start at 1e-12 .. 1e-13 of a well-scaled system is good to a per cent or so;
 * a batch forms it with the compensated SpMM of its verify rounds, good to about 1e-15 of itself.  struct
 * lsb_hip_result keeps its layout: this is where the starting residual is read.  2 if the last solve was a cold one, if nrhs does not match, or on null arguments. */
int lsb_hip_solver_start_relres(const lsb_hip_solver *s, unsigned nrhs, double *out);
/* Successive right-hand sides (time stepping, a Newton loop): the solver keeps an S-orthonormal basis X~ of up to
 * `depth` earlier solutions on the device -- pairs (x~_k, S x~_k) of n_local doubles, X~^T S X~ = I -- and starts each
 * solve of the sequence from x0 = X~ (X~^T b), the S-norm best approximation of the solution in their span (Fischer,
 * CMAME 163, 1998).  Opt-in: nothing else reads or disturbs the basis, a solver that never asks for one allocates
 * nothing.
 *   seq_begin: depth = 1 .. LSB_SEQ_MAX_DEPTH allocates the pairs and empties the basis; again: empties it, and
 *   re-allocates if depth changed; depth = 0 frees everything.  2, and nothing allocated, for depth > LSB_SEQ_MAX_DEPTH
 *   and on a solver this does not serve: more than one shard (virtual shards included), ranks, and the unsymmetric
 *   drivers GMRES and BiCGSTAB -- the projection needs a symmetric positive definite operator.  Every other solver that
 *   solve_x0 serves on one shard is served.
 *   solve_seq[_dev]: b and x in the caller's numbering as in solve[_dev]; x need not be initialised.  With an empty
 *   basis it IS solve[_dev], bit for bit.  Otherwise x0 = X~ (X~^T b) and solve_x0's rules from there: the stop rule
 *   relative to ||b||, ||b - S x0|| <= tol ||b|| returns x0 with 0 iterations, b = 0 gives x = 0, res->iters counts
 *   from x0 and lsb_hip_solver_start_relres(s, 1, .) reports ||b - S x0|| / ||b||.  2 before seq_begin and on null
 *   arguments; 2 leaves x untouched.
 *   Behind a solve that ended CONVERGED after at least one iteration (opts.tol > 0) the basis takes the correction
 *   d = x - x0 (the first solve: d = x): w = S d by the fp64 product of a recomputed residual, two Gram-Schmidt passes
 *   against the held pairs (d -= sum beta_k x~_k, w -= sum beta_k S x~_k with beta_k = x~_k . w), nu = d . w, and
 *   (d, w) / sqrt(nu) becomes the next pair -- unless nu is not finite or not > 0, then the basis stays as it was.  A
 *   full basis restarts first: it is emptied and d = x, the whole current solution (restarts counts these).  Under
 *   opts.verify or mixed precision, where correction runs moved x on, x0 is formed again and d = x - x0.
 *   One host read of three doubles ends the update; it is the only one the feature adds to a solve.
 *   seq_info: depth (0: none), pairs held, restarts since seq_begin, device bytes the feature holds; any may be NULL.
 *   seq_basis_dev: pair k < held in the caller's numbering into d_xk, d_sxk (n_local doubles each, either may be
 *   NULL); 2 for k >= held.  For tests. */
#define LSB_SEQ_MAX_DEPTH 16
int lsb_hip_solver_seq_begin(lsb_hip_solver *s, unsigned depth);
int lsb_hip_solver_solve_seq_dev(lsb_hip_solver *s, const double *d_b, double *d_x, struct lsb_hip_result *res);
int lsb_hip_solver_solve_seq(lsb_hip_solver *s, const double *b, double *x, struct lsb_hip_result *res);
int lsb_hip_solver_seq_info(const lsb_hip_solver *s, unsigned *depth, unsigned *held, unsigned *restarts,
                            unsigned long long *bytes);
int lsb_hip_solver_seq_basis_dev(lsb_hip_solver *s, unsigned k, double *d_xk, double *d_sxk);
/* Device time of the last solve_seq[_dev]'s projection (0: the basis was empty) and update (0: there was none), in
 * microseconds between events on the solver's stream; 2 before seq_begin.  For tools/bench_seq.py.  The events are
 * recorded on request only: the first call behind a seq_begin that (re-)allocated the basis answers 0, 0 and turns the
 * recording on -- four event records per solve from then on; a sequence that never asks records none. */
int lsb_hip_solver_seq_last_us(lsb_hip_solver *s, double *project_us, double *update_us);
/* y_local = Op * x: d_x holds this rank's rows (length n_local); remote
 * entries are exchanged first when the solver is distributed. */
int lsb_hip_solver_spmv_dev(lsb_hip_solver *s, const double *d_x, double *d_y);
/* The product the Krylov loop issues, where spmv_dev is the exact one: the same gather, exchange and
 * status check, then the launches of an iteration's SpMV -- the solver's form, flags, grid, period
 * and value arrays, split into interior / boundary launches where the solver overlaps its exchange.
 * An fp64 solver: S x, the bits of spmv_dev.  LSB_PREC_MIXED: S~ x with S~ = fp32(S), what the inner
 * CG multiplies by.  d_dot (may be NULL; one shard only, else 2): the launch's fused x.y, reduced
 * from its own partial sums. */
int lsb_hip_solver_spmv_inner_dev(lsb_hip_solver *s, const double *d_x, double *d_y, double *d_dot);
/* z = M^-1 r once, the preconditioner the solver was made with (LSB_PRECOND_AMG: one V-cycle),
 * on the solver's stream; device buffers of length n_local in the caller's numbering.  2 for a
 * preconditioner that is not applied as a vector of its own (the diagonal ones: see
 * lsb_hip_solver_jacobi_sweep_dev). */
int lsb_hip_solver_precond_dev(lsb_hip_solver *s, const double *d_r, double *d_z);
/* For tests, LSB_PRECOND_GMG only (2 for every other solver): the same application in the solver's own numbering --
 * buffers of n_local + lsb_hip_solver_padded rows, row (j, i) of a line-padded grid at j pitch + i, the pad rows of r
 * to be 0 -- which is what the launches themselves read and write: tests look at the pad rows of z there. */
int lsb_hip_solver_precond_padded_dev(lsb_hip_solver *s, const double *d_r, double *d_z);
/* LSB_PRECOND_AMG: levels of the hierarchy, the coarsest included, and how many of them (with
 * the coarse solve) run in the one-launch tail; 2 for another preconditioner. */
int lsb_hip_solver_amg_info(lsb_hip_solver *s, unsigned *levels, unsigned *tail_levels);
/* LSB_PRECOND_AMG with LSB_AMG_SMOOTH_CHEB: the interval [lo, hi] of D^-1 A the smoother of `level` was built
 * on (hi = lsb_amg_gershgorin of the level, lo = hi / amg_cheb_ratio); 2 for another preconditioner or
 * smoother and for a level that is not smoothed (the coarsest, or beyond). */
int lsb_hip_solver_amg_cheb_interval(lsb_hip_solver *s, unsigned level, double *lo, double *hi);
/* LSB_PRECOND_AMG with LSB_AMG_SMOOTH_MCGS: the colours of `level`'s Gauss-Seidel sweeps; *ncolours = 0 for a level
 * whose colouring has more than the cap and which therefore keeps l1-Jacobi.  2 for the coarsest level, a level out
 * of range and a solver of another smoother or preconditioner. */
int lsb_hip_solver_amg_colours(lsb_hip_solver *s, unsigned level, unsigned *ncolours);
/* The precision of the V-cycle: LSB_AMG_PREC_FP64 (0) or LSB_AMG_PREC_FP32 (1); 2 for a solver without AMG. */
int lsb_hip_solver_amg_precision(lsb_hip_solver *s);
/* Bytes one application of the V-cycle must move, 0 without AMG.  fp64: 12 per stored entry for every launch that
 * streams a matrix (A 2 nu times per level, P and R once), 8 nc^2 for the coarse inverse, 8 per element pass of
 * the level vectors.  fp32: 8 per stored entry, 4 nc^2, 4 per element pass; the fine level's r is read once
 * and z written once at 8, and the fp32 copy of r is written once.
 * A level smoothed by multicolour Gauss-Seidel (LSB_AMG_SMOOTH_MCGS), M entries of which M0 in rows of colour 0,
 * n rows of which n0 of colour 0: the colour-sorted copy once per sweep less M0 (the first forward sweep starts
 * from zero and streams the colours >= 1 only) and A once for the residual, (2 nu + 1) M - M0 entries; per sweep
 * b, dinv, x in and x out of every row, 8 nu n element passes, plus n - 2 n0 because the first launch writes all
 * of x and reads b and dinv on colour 0 only; the residual, restriction and prolongation as on every level, 6 n.
 * Row offsets and rowid are left out, as the offsets are everywhere above. */
unsigned long long lsb_hip_solver_amg_cycle_bytes(const lsb_hip_solver *s);
/* LSB_PRECOND_GMG: the levels of the cycle, the coarsest included, the grid (dims[d] = 1 beyond its dimension) and the
 * pitch of the fine level's grid lines in the solver's numbering (dims[0], or more under line padding); each may be
 * NULL.  2 for another preconditioner. */
int lsb_hip_solver_gmg_info(lsb_hip_solver *s, unsigned *levels, unsigned dims[3], unsigned *pitch);
/* ... level l's points and delta per dimension (lsb_gmg_plan's); 2 for a level out of range */
int lsb_hip_solver_gmg_level(lsb_hip_solver *s, unsigned level, unsigned n[3], double delta[3]);
/* Bytes one application of the geometric V-cycle must move, 0 without it: vectors only.  Per level of n rows and n'
 * coarse rows, 8 B per element pass -- fused (nu = 1): the way down reads b and writes x and b', 16 n + 8 n', the way
 * up reads x, b and x' and writes the result, 24 n + 8 n'; plain steps: x = w b 16 n, each of the 2 nu - 1 sweeps
 * 24 n, the restriction 16 n + 8 n', the prolongation 16 n + 8 n'.  The coarsest level: 8 nc^2 + 16 nc. */
unsigned long long lsb_hip_solver_gmg_cycle_bytes(const lsb_hip_solver *s);
/* The direct solver's factor (LSB_KRYLOV_DIRECT): entries of W = L^-1, height of the elimination tree, and the bytes
 * the two products of one round stream (16 per entry, and the index and vector traffic per row); each may be NULL.
 * 2 for any other solver. */
int lsb_hip_solver_direct_info(const lsb_hip_solver *s, unsigned long long *entries, unsigned *height,
                               unsigned long long *bytes_per_round);
/* A direct solver (o->krylov must be LSB_KRYLOV_DIRECT; o = NULL: the backend's current options) whose inverse factor
 * is kept in tiers (struct lsb_tierinv; hip_direct_t.hip, hip_direct_drv.c): for operators whose single skyline is
 * over LSB_DIRECT_MAX_ENTRIES.  tiers = 1 is lsb_hip_solver_create itself; 2 .. LSB_DIRECT_MAX_TIERS asks for that
 * many (the factor may have fewer: tiers nobody is in are dropped); 0 takes the fewest that fit the budget
 * w_entries + 3 coupling_entries <= LSB_DIRECT_MAX_ENTRIES by the symbolic count -- where that is one, the solver IS
 * lsb_hip_solver_create's.  A factor of one tier is the single skyline however it was asked for: two launches, 56
 * bytes per row and round, served by the block entry points of the single skyline.  NULL for another krylov or tiers
 * out of range; what lsb_hip_solver_create refuses for a direct solver is refused in the same way, and so is a factor
 * over the budget in the tiers asked for.  A round is 4 m - 2 launches for m tiers instead of 2, then the residual
 * and the stop test as before.  Every solve entry point of a direct solver works on it (solve[_dev], solve_x0[_dev],
 * solve_seq[_dev], precond_dev, opts.verify) but, on more than one tier, the blocks of right-hand sides, which answer
 * 2: blocks on a tiered factor have entry points of their own, lsb_hip_solver_solve_direct_tier_multi[_dev] below.
 * On a solver of more than one tier lsb_hip_solver_direct_info reports the entries of the W_tt, the height of the whole tree, and as
 * bytes per round 16 per entry of the W_tt, 24 per coupling entry (C and C^T once each: a value and a 32-bit column),
 * and 104 per row (first / woff twice, the offsets of C and C^T, P r, y, z and x). */
lsb_hip_solver *lsb_hip_solver_create_direct(const struct csr *A, const struct lsb_hip_opts *o, int tiers);
/* Tiers of a direct solver's factor: how many, the entries of the W_tt and of the coupling C, the rows of each tier
 * (LSB_DIRECT_MAX_TIERS slots, 0 behind the last tier) and the launches of one application (4 m - 2); each may be
 * NULL.  A solver of lsb_hip_solver_create reports one tier and no coupling.  2 for a solver that is not direct. */
int lsb_hip_solver_direct_tier_info(const lsb_hip_solver *s, unsigned *ntiers, unsigned long long *w_entries,
                                    unsigned long long *coupling_entries, unsigned *tier_rows,
                                    unsigned *launches_per_round);
/* LSB_PRECOND_CHEBYSHEV: the interval [lmin, lmax] of D^-1 S the polynomial was built on at creation
 * (lmax = 1.1 x the power iteration's estimate, lmin = lmax / max(30, 16 degree^2), the degree
 * clamped to 1 .. 32); 2 for another preconditioner. */
int lsb_hip_solver_cheb_interval(const lsb_hip_solver *s, double *lmin, double *lmax);
/* Time `reps` back-to-back launches of the solver's SpMV kernel with HIP
 * events on the solver's stream (after `warm` untimed ones); *ms_avg = mean
 * milliseconds per launch.  No exchange, local shard 0. */
int lsb_hip_solver_time_spmv(lsb_hip_solver *s, int warm, int reps,
                             double *ms_avg);
/* One weighted-Jacobi sweep x <- x + w D^-1 (b - Op x), device buffers. */
int lsb_hip_solver_jacobi_sweep_dev(lsb_hip_solver *s, double w,
                                    const double *d_b, double *d_x);

/* Several right-hand sides at once (hip_mrhs.hip, hip_mrhs_amg.hip, hip_mrhs_drv.c): nrhs INDEPENDENT PCG
 * recurrences advanced by the same launches -- every column has its own alpha, beta, residual norms, iteration count
 * and status, a column that has stopped is frozen while the others run on, and the batch runs until every
 * column has stopped.  Not block-CG.  The blocks are column-major with a leading dimension (ld >= n_local),
 * like BLAS and CHOLMOD's dense matrices, in the caller's numbering.  Any nrhs >= 1: one column goes through
 * lsb_hip_solver_solve_dev and gives its bits; 2 .. 8 run as one batch of 2, 4 or 8 columns (padded with
 * zero columns, frozen from the start); more run in batches of 8 and a remainder.
 * Returns 1 when the backend is not initialised; 2 for bad arguments (nrhs == 0, ld < n_local, null
 * pointers) and for a solver this version does not serve.  Served: one shard in one process, LSB_PREC_FP64,
 * krylov PCG or AUTO, precond JACOBI / L1JACOBI / NONE / AMG (one V-cycle per iteration on the block of
 * residuals: every matrix of the hierarchy is streamed once for all columns, and a column's z has the bits of
 * the single-column cycle; opts.amg_tail_rows is ignored there), and FSAI where opts.fsai_blocks is set (z = G^T (G r)
 * on the block, the x / r update riding in the two products: four launches an iteration, hip_mrhs_fsai.hip; the
 * single-column paths of such a solver are unchanged); GMRES, BiCGSTAB, PCG1, Chebyshev, block-Jacobi,
 * FSAI without opts.fsai_blocks, nvirt > 1, distributed and persistent solvers answer 2, and so does an AMG solver smoothed by multicolour
 * Gauss-Seidel (LSB_AMG_SMOOTH_MCGS: its cycle is not built on blocks; lsb_hip_solver_spmm_dev still serves it) --
 * nothing falls back to a loop of single solves.
 * res[c] (nrhs entries) is column c's own result: iters, status, relres, corrections, true_relres are the
 * column's; seconds is the wall-clock of the batch the column ran in and spmvs the SpMM launches of that
 * batch, the same in all its entries; spmv_ms = 0, spmv_samples = 0 (opts.sample_spmv is ignored).
 * Stop rules per column as in a single solve: b_c = 0 -> CONVERGED, 0 iterations, x_c = 0; r.r <= tol^2 b.b
 * on the recurrence -> CONVERGED; iters >= maxit -> MAXIT; p.q zero or not finite -> BREAKDOWN.
 * opts.verify = 1: after the batch stops one SpMM recomputes ||b_c - S x_c|| / ||b_c|| into true_relres
 * (-1 without verify, and for b_c = 0); columns called converged whose recomputed residual misses tol restart
 * in place (r = b - S x, p = M^-1 r, x kept, iterations counted on), at most 6 rounds, after which a column
 * that still misses is MAXIT.  opts.use_graph is honoured through a graph cache of its own. */
/* Y = Op X for nrhs columns; column c of X at d_X + c*ldx, n_local doubles, caller's numbering (as spmv_dev) */
int lsb_hip_solver_spmm_dev(lsb_hip_solver *s, unsigned nrhs, const double *d_X, size_t ldx,
                            double *d_Y, size_t ldy);
/* x_c = S^-1 b_c from x0 = 0 for c < nrhs; res[c] is column c's own result */
int lsb_hip_solver_solve_multi_dev(lsb_hip_solver *s, unsigned nrhs, const double *d_B, size_t ldb,
                                   double *d_X, size_t ldx, struct lsb_hip_result *res);
int lsb_hip_solver_solve_multi(lsb_hip_solver *s, unsigned nrhs, const double *B, size_t ldb,
                               double *X, size_t ldx, struct lsb_hip_result *res);   /* host buffers */
/* solve_multi_dev from an initial guess: column c of d_X holds x0_c on entry.  Serves and refuses exactly what
 * solve_multi_dev does (2 leaves d_X untouched); nrhs == 1 is lsb_hip_solver_solve_x0_dev.  No correction solve here:
 * the batch starts in place on the device -- r = b - S x0 by the SpMM of a verify round, p = M^-1 r, and per column
 * b_c = 0 -> x_c = 0, CONVERGED; r.r <= tol^2 b.b -> CONVERGED with 0 iterations, x_c the bits of x0_c; else the
 * column runs, its iterations counted from x0, its threshold tol^2 b.b.  A column with x0_c = 0 has the bits, iters
 * and status of the same column in solve_multi_dev.  Only n_local doubles of a column are read and written: the
 * slack behind it stays the caller's.  lsb_hip_solver_start_relres(s, nrhs, out) reads the starting residuals. */
int lsb_hip_solver_solve_multi_x0_dev(lsb_hip_solver *s, unsigned nrhs, const double *d_B, size_t ldb,
                                      double *d_X, size_t ldx, struct lsb_hip_result *res);
/* bytes one iteration of the batch must move: 12 nnz + 4 (n + 1) + 8 n (11 Kp + 2 [the diagonal is a
 * vector]) with n the internal row count and Kp the batch width -- the CSR arrays once whatever the width,
 * 2 passes of the SpMM (x once, y once) and the 9 of the classic form's sweeps per column, the diagonal once
 * per sweep for all columns; 0 where solve_multi does not apply, and 0 for an AMG solver: an iteration around a
 * V-cycle has another shape, as lsb_hip_solver_iteration_bytes answers for every such preconditioner.
 * FSAI on blocks (opts.fsai_blocks): 12 (nnz_S + nnz_G + nnz_G^T) + 12 (n + 1) + 8 n 16 Kp -- the three matrices once
 * each whatever the width, and 16 vector passes per column: the SpMM 2; the launch of G 6 (q and r gathered, p and x
 * in, x and t out); the launch of G^T 5 (t gathered, q and r in, r and z out); the direction sweep 3 */
unsigned long long lsb_hip_solver_multi_iteration_bytes(const lsb_hip_solver *s, unsigned nrhs);
/* entries of G and of G^T of an LSB_PRECOND_FSAI solver (either pointer may be NULL); 2 for any other solver */
int lsb_hip_solver_fsai_nnz(const lsb_hip_solver *s, unsigned long long *g, unsigned long long *gt);
/* Z_c = M^-1 R_c for nrhs columns: the V-cycle of a batch's iteration on its own, or -- FSAI with opts.fsai_blocks --
 * the two products Z = G^T (G R) (blocks as above: column-major with a leading dimension, caller's numbering; any
 * nrhs >= 1, in batches of 8 and a remainder).  Under AMG column c of Z has the bits of
 * lsb_hip_solver_precond_dev on column c alone.  1 when the backend is not initialised; 2 for null pointers,
 * nrhs == 0, ld < n_local and for every solver that solve_multi does not serve under AMG or FSAI (Jacobi, Chebyshev
 * and block-Jacobi solvers, and FSAI without opts.fsai_blocks, among them); Z is not touched then. */
int lsb_hip_solver_precond_multi_dev(lsb_hip_solver *s, unsigned nrhs, const double *d_R, size_t ldr,
                                     double *d_Z, size_t ldz);

/* The direct solver on blocks of right-hand sides (LSB_KRYLOV_DIRECT; hip_direct_m.hip, hip_direct_m_drv.c): the rounds
 * x (+)= P^T W^T (W (P r)), r = b - S x of a single direct solve on nrhs columns at once.  A block of columns reads
 * every entry of W once per product for all of them, walks the row records once and pays the same launches -- what a
 * cached factor is for, and what CHOLMOD's solve takes a dense B for.  Entry points of their own: solve_multi[_dev],
 * solve_block[_dev], spmm_dev and precond_multi_dev keep answering 2 on a direct solver.
 * The contract: a column solved in a block is, bit for bit, that column solved alone by lsb_hip_solver_solve_dev on
 * the same solver -- x, iters, status, relres, true_relres, spmvs.  (So no MFMA: it sums in an order of its own.)
 * Blocks as for solve_multi: column-major, ld >= n_local, the caller's numbering; only n_local doubles of a column
 * are read or written, the slack stays the caller's.  Any nrhs >= 1: one column is forwarded to
 * lsb_hip_solver_solve_dev / _precond_dev; 2 .. 8 run as one block of width 2, 4 or 8, padded with zero columns that
 * are not reported; more run in blocks of 8 and a remainder.
 * Returns 1 when the backend is not initialised; 2 for bad arguments (nrhs == 0, ld < n_local, null pointers) and for
 * every solver that is not a direct solver -- X is untouched and nothing is allocated.  A direct solver allocates the
 * work area of a width when it first solves a block of that width, and nothing before.
 * res[c] is column c's own result with the single solve's meaning field by field (under tol = 0: relres =
 * true_relres = -1, spmvs = iters - 1); seconds is the wall clock of the block the column ran in.
 * Columns stop on their own: a column whose status has left RUNNING is frozen, the block runs until every column has
 * stopped.  b_c = 0 -> CONVERGED after round 1, x_c = 0, relres 0; a column with a NaN -> BREAKDOWN after round 1, and
 * it disturbs no other column; maxit = 0 -> x = 0, MAXIT; tol = 0 -> exactly maxit rounds, no residual behind the last.
 * opts.use_graph and opts.check_every are honoured as by the single solve.  Warm starts on blocks are not built: the
 * columns start from x0 = 0. */
/* x_c = S^-1 b_c for c < nrhs by the direct solver's rounds, W streamed once per product for a block of columns */
int lsb_hip_solver_solve_direct_multi_dev(lsb_hip_solver *s, unsigned nrhs, const double *d_B, size_t ldb,
                                          double *d_X, size_t ldx, struct lsb_hip_result *res);
int lsb_hip_solver_solve_direct_multi(lsb_hip_solver *s, unsigned nrhs, const double *B, size_t ldb,
                                      double *X, size_t ldx, struct lsb_hip_result *res);   /* host buffers */
/* Z_c = P^T W^T W P R_c once: precond_dev's application on a block */
int lsb_hip_solver_direct_apply_multi_dev(lsb_hip_solver *s, unsigned nrhs, const double *d_R, size_t ldr,
                                          double *d_Z, size_t ldz);
/* bytes one round of a block of width kp(nrhs) streams: 16 per entry of W and 24 per row whatever the width, 32 per
 * row and column (lsb_hip_solver_direct_info's figure at kp = 1); 0 for any other solver or nrhs == 0 */
unsigned long long lsb_hip_solver_direct_multi_round_bytes(const lsb_hip_solver *s, unsigned nrhs);
/* The same on every direct solver, one with a tiered factor (lsb_hip_solver_create_direct) included: there a round on
 * a block is the 4 m - 2 launches of the tiers in their block form (hip_direct_tm.hip), every entry of the W_tt, of C
 * and of C^T loaded once per product for all columns, then the residual and the stop test of the blocks above.  The
 * three entry points above keep answering 2 on a solver of more than one tier; on a single skyline (one tier, however
 * it was created) these are the three above.  Arguments, layout, block cutting, return values, results and the stop rules are theirs, and so is the
 * contract: a column of a block has the bits of that column solved alone by lsb_hip_solver_solve_dev (applied alone by
 * lsb_hip_solver_precond_dev) on the same solver; nrhs == 1 is forwarded to those.  1 when the backend is not
 * initialised; 2 for bad arguments and for a solver that is not direct: nothing is written.  The work area of a width
 * (five block vectors on a tiered solver) is made when the solver first sees a block of that width.
 * Not built on these blocks: warm starts, sequences and opts.verify; more than 8 columns per block; fp32 storage. */
int lsb_hip_solver_solve_direct_tier_multi_dev(lsb_hip_solver *s, unsigned nrhs, const double *d_B, size_t ldb,
                                               double *d_X, size_t ldx, struct lsb_hip_result *res);
int lsb_hip_solver_solve_direct_tier_multi(lsb_hip_solver *s, unsigned nrhs, const double *B, size_t ldb,
                                           double *X, size_t ldx, struct lsb_hip_result *res);   /* host buffers */
/* Z_c = P^T L^-T L^-1 P R_c once, un-gated: precond_dev's application on a block */
int lsb_hip_solver_direct_tier_apply_multi_dev(lsb_hip_solver *s, unsigned nrhs, const double *d_R, size_t ldr,
                                               double *d_Z, size_t ldz);
/* bytes one round of a block of width kp(nrhs) streams.  A tiered factor: fixed + kp per_column with fixed = 16 per
 * entry of the W_tt, 24 per coupling entry and 32 per row (first / woff twice, the offsets of C and C^T), per_column =
 * 72 per row (nine passes over P V, Y, Z and X); at nrhs = 1 lsb_hip_solver_direct_info's figure.  A single skyline:
 * lsb_hip_solver_direct_multi_round_bytes.  0 for any other solver or nrhs == 0 */
unsigned long long lsb_hip_solver_direct_tier_multi_round_bytes(const lsb_hip_solver *s, unsigned nrhs);

/* AMG as the solver on blocks of right-hand sides (hip_rich_m.hip, hip_rich_m_drv.c; the fp32 cycle on blocks:
 * hip_amg_f32_m.hip): the stationary V-cycle iteration of LSB_KRYLOV_RICHARDSON -- x = 0, r = b; per cycle z = M^-1 r,
 * q = S z, x += z, r -= q -- on nrhs columns at once.  A cycle is streams of the hierarchy's matrices, one product
 * with S and six vector passes; a block of columns reads each of those matrices once for all of its columns.  This
 * is the protocol of the reference's AMG backends on a block: maxit 2, tol 0 with the fp64 cycle, maxit 1, tol 0 with
 * the fp32 cycle.  Entry points of their own: solve_multi[_dev], solve_block[_dev], spmm_dev and precond_multi_dev keep
 * answering 2 on such a solver.
 * Served: krylov = LSB_KRYLOV_RICHARDSON with precond = LSB_PRECOND_AMG, one shard in one process, LSB_PREC_FP64
 * values, smoothed by l1-Jacobi with the cycle in fp64 or in fp32 (LSB_AMG_PREC_FP32), or by the Chebyshev smoother
 * with the cycle in fp64.  Returns 1 when the backend is not initialised; 2 for bad arguments (nrhs == 0,
 * ld < n_local, null pointers) and for every other solver -- multicolour Gauss-Seidel, the Chebyshev smoother in fp32
 * and AMG under PCG among them; X (or Z) is untouched then and nothing is allocated.  A served solver allocates the
 * work area of a width when it first sees a block of that width, and nothing before.
 * Blocks as for solve_multi: column-major, ld >= n_local, the caller's numbering (re-ordered and line-padded solvers
 * are served); only n_local doubles of a column are read or written.  Any nrhs >= 1: one column is forwarded to
 * lsb_hip_solver_solve_dev / _precond_dev; 2 .. 8 run as one block of width Kp = 2, 4 or 8, padded with zero columns
 * that are not reported; more run in blocks of 8 and a remainder.
 * opts.tol, maxit, check_every, use_graph and verify mean per column what they mean for the single solve, and res[c]
 * is column c's own result with the single solve's meaning field by field: spmvs = iters + the residuals recomputed
 * under opts.verify, true_relres = -1 without it; seconds is the wall clock of the block the column ran in.
 * Columns stop on their own: a column whose status has left RUNNING is frozen -- its x is no longer written -- and
 * the block runs until every column has stopped.  b_c = 0 -> CONVERGED, 0 cycles, x_c = 0; a column with a NaN ->
 * BREAKDOWN at cycle 1, and it disturbs no other column; maxit = 0 -> x = 0, MAXIT; tol = 0 -> exactly maxit cycles.
 * A column's x, iters, status and relres do not depend on the width of the block or on the other columns: its
 * z = M^-1 r has the bits of lsb_hip_solver_precond_dev, its q = S z those of lsb_hip_solver_spmm_dev, x + z and r - q
 * are single operations, and r.r is summed in the single solve's order.  Warm starts on blocks are not built. */
/* x_c ~ S^-1 b_c for c < nrhs by stationary V-cycle iterations from x0 = 0; res[c] is column c's own result */
int lsb_hip_solver_amg_solve_multi_dev(lsb_hip_solver *s, unsigned nrhs, const double *d_B, size_t ldb,
                                       double *d_X, size_t ldx, struct lsb_hip_result *res);
int lsb_hip_solver_amg_solve_multi(lsb_hip_solver *s, unsigned nrhs, const double *B, size_t ldb,
                                   double *X, size_t ldx, struct lsb_hip_result *res);   /* host buffers */
/* Z_c = M^-1 R_c, one V-cycle per column in the precision the solver cycles in: column c of Z has the bits of
 * lsb_hip_solver_precond_dev on column c alone */
int lsb_hip_solver_amg_cycle_multi_dev(lsb_hip_solver *s, unsigned nrhs, const double *d_R, size_t ldr,
                                       double *d_Z, size_t ldz);
/* bytes one cycle of a block of width Kp(nrhs) must move: the V-cycle's matrix bytes once whatever the width and its
 * vector bytes per column (the two parts of lsb_hip_solver_amg_cycle_bytes, fp64 or fp32), 12 nnz + 16 n Kp for the
 * SpMM, and the update's six vector passes per column, 48 n Kp; nrhs = 1: the single solve's cycle.  0 for a solver
 * that is not served and for nrhs == 0 */
unsigned long long lsb_hip_solver_amg_solve_multi_bytes(const lsb_hip_solver *s, unsigned nrhs);

/* Block-CG proper (hip_bcg.hip, hip_bcg_drv.c): ONE Krylov space for a block of right-hand sides, where solve_multi
 * runs nrhs independent recurrences.  Preconditioned BCGrQ from x0 = 0: the residual block is kept factored as
 * R = W sigma with W^T D^-1 W = I (Cholesky-QR in the inner product of the solver's diagonal preconditioner D^-1), the
 * search directions span the union of the columns' Krylov spaces, and the iteration count is the block's: every
 * res[c].iters is the same number.  Blocks as for solve_multi[_dev]: column-major, ld >= n_local, the caller's
 * numbering; res may be NULL.
 * Returns 0: solved, or stopped with a status; 1: backend not initialised; 2: not served -- X untouched, nothing
 * allocated; 3: the block is rank-deficient -- X untouched, res[c].status = LSB_STATUS_BREAKDOWN for every column.
 * Served: what solve_multi serves under the diagonal preconditioners (LSB_PRECOND_JACOBI, _L1JACOBI, _NONE) with
 * 2 <= nrhs <= 8; nrhs == 1 is lsb_hip_solver_solve_dev.  AMG, FSAI (with or without opts.fsai_blocks), Chebyshev,
 * block-Jacobi, nvirt > 1, fp32 values, persistent solvers, nrhs > 8, nrhs == 0, null pointers and ld < n_local
 * answer 2.  Widths 2 .. 8 run at 2, 4 or 8 columns, padded with zero columns.
 * Stop rule: the recurrence's ||r_c|| <= tol ||b_c|| for EVERY column, or maxit; the columns are coupled, so none is
 * frozen: all run until all meet the rule.  At maxit a column that meets its threshold is CONVERGED, the others are
 * MAXIT.  relres = ||r_c|| / ||b_c|| of the recurrence; spmvs = SpMM launches that did work.
 * Rank rule: at the start G = B^T D^-1 B is scaled to unit diagonal (a zero column counts as a zero pivot) and
 * factored; a Cholesky pivot <= 1e-10 or not finite answers 3.  Inside the loop a pivot of P^T S P or of the
 * residual block's Gram matrix that is <= 0 or not finite stops the block, every column LSB_STATUS_BREAKDOWN (0 is
 * returned; X holds the iterate reached).
 * opts.verify = 1: one SpMM recomputes ||b_c - S x_c|| / ||b_c|| into true_relres and relres after the stop; a
 * column called converged that misses tol there becomes MAXIT.  There is no in-place restart in the block form.
 * opts.use_graph and opts.check_every are honoured as by solve_multi; warm starts are not built. */
int lsb_hip_solver_solve_block_dev(lsb_hip_solver *s, unsigned nrhs, const double *d_B, size_t ldb,
                                   double *d_X, size_t ldx, struct lsb_hip_result *res);
int lsb_hip_solver_solve_block(lsb_hip_solver *s, unsigned nrhs, const double *B, size_t ldb,
                               double *X, size_t ldx, struct lsb_hip_result *res);   /* host buffers */
/* bytes one iteration of the block must move: 12 nnz + 4 (n + 1) + 8 n (12 Kp + 2 [the diagonal is a vector]) -- the
 * CSR arrays once whatever the width and 12 vector passes per column: the SpMM 2 (P gathered, Q out), pass A 6 (W, Q,
 * P, X in; W, X out), pass B 4 (W, P in; W, P out), the diagonal once in each of the two passes; 0 where the block
 * form is not served */
unsigned long long lsb_hip_solver_block_iteration_bytes(const lsb_hip_solver *s, unsigned nrhs);
/* ||r_c||^2 of the recurrence and ||b_c||^2 out of the device state of the last block solved (nrhs <= 8 doubles each,
 * either pointer may be NULL): what res[c].relres of a run without opts.verify was formed from.  2 where the solver has
 * solved no block */
int lsb_hip_solver_block_norms(const lsb_hip_solver *s, unsigned nrhs, double *rr, double *bb);

/* Block-CG under FSAI and AMG (hip_bcg_m.hip, the second half of hip_bcg_drv.c): the method of solve_block with D^-1
 * replaced by the solver's preconditioner M^-1 where that is a symmetric operator, so W^T M^-1 W = I and the
 * preconditioned block is a stored operand.  Signatures, return codes, stop rule, rank rule (on G = B^T M^-1 B),
 * opts.verify, opts.use_graph, opts.check_every and lsb_hip_solver_block_norms: exactly solve_block[_dev]'s.
 * Served: what solve_multi serves with z as a block of its own -- LSB_PRECOND_AMG in fp64 smoothed by l1-Jacobi or
 * Chebyshev, LSB_PRECOND_FSAI with opts.fsai_blocks = 1 -- with 2 <= nrhs <= 8, one shard, x0 = 0.  A solver under a
 * diagonal preconditioner is forwarded to solve_block[_dev] (the same bits); on a served solver nrhs == 1 is
 * lsb_hip_solver_solve_dev.  Everything else answers 2, X untouched, nothing allocated: AMG smoothed by multicolour
 * Gauss-Seidel or cycling in fp32, FSAI without opts.fsai_blocks, Chebyshev, block-Jacobi, nvirt > 1, fp32 values,
 * BiCGSTAB / GMRES / Richardson, nrhs == 0 or > 8, null pointers, ld < n_local.  solve_block[_dev] itself keeps
 * answering 2 on AMG and FSAI solvers.
 * An iteration under FSAI is 7 launches (SpMM, the small algebra, X and W~, the product with G, the product with G^T
 * carrying the Gram sums, the small algebra, W and P); under AMG 6 launches and the V-cycle.  The preconditioner's
 * launches inside the loop are not gated on the block's stop word: after the stop they run on for the rest of a
 * polling chunk (opts.check_every; by default at least 2 iterations under AMG) into buffers nobody reads. */
int lsb_hip_solver_solve_block_precond_dev(lsb_hip_solver *s, unsigned nrhs, const double *d_B, size_t ldb,
                                           double *d_X, size_t ldx, struct lsb_hip_result *res);
int lsb_hip_solver_solve_block_precond(lsb_hip_solver *s, unsigned nrhs, const double *B, size_t ldb,
                                       double *X, size_t ldx, struct lsb_hip_result *res);   /* host buffers */
/* bytes one iteration of solve_block_precond must move under FSAI: 12 (nnz + nnz_G + nnz_Gt) + 12 (n + 1) +
 * 8 n 18 Kp -- S, G and G^T once each whatever the width and 18 vector passes per column: the SpMM 2, X and W~ 6, the
 * product with G 2, the product with G^T and the Gram sums 3, W and P 5.  Under AMG 0, as
 * lsb_hip_solver_multi_iteration_bytes (a V-cycle has another shape); under a diagonal preconditioner
 * lsb_hip_solver_block_iteration_bytes; 0 where nothing is served */
unsigned long long lsb_hip_solver_block_precond_iteration_bytes(const lsb_hip_solver *s, unsigned nrhs);

unsigned lsb_hip_solver_nrows_local(const lsb_hip_solver *s);
/* rows the solver added inside: 0, or the pad rows of a line-padded 2-D grid (lsb_csr_pad_lines;
 * a constant-coefficient grid of >= 1 M rows whose lines are not whole slices, LSBENCH_HIP_PAD_LINES=0
 * turns it off).  b and x keep the caller's numbering and length. */
int lsb_hip_solver_padded(const lsb_hip_solver *s);
/* Which vectors of the two-launch PCG iteration lie inside the first shard's vector slab (one allocation: their
 * relative placement is the same in every solver): bit 0 r, 1 the gather vector (the first direction buffer),
 * 2 the second direction buffer, 3 / 4 the x / b of a padded or re-ordered solver. */
unsigned lsb_hip_solver_slab_mask(const lsb_hip_solver *s);
unsigned lsb_hip_solver_nrows_global(const lsb_hip_solver *s);
unsigned long long lsb_hip_solver_nnz_local(const lsb_hip_solver *s);
unsigned lsb_hip_solver_nblocks(const lsb_hip_solver *s);
int lsb_hip_solver_spmv_variant(const lsb_hip_solver *s);
/* What the timing pass at creation picked for shard 0: flags (bit 0 prefetch,
 * bit 1 nontemporal) and the workgroup cap of the SpMV launch. */
unsigned lsb_hip_solver_spmv_flags(const lsb_hip_solver *s);
unsigned lsb_hip_solver_spmv_grid(const lsb_hip_solver *s);
/* sliced-ELL: slices per plane the XCD dealing follows (every XCD the same eighth
 * of every plane of a 3-D stencil), 0 = contiguous eighths of the rows. */
unsigned lsb_hip_solver_spmv_period(const lsb_hip_solver *s);
/* slices the first shard's z-column plan walks in columns (k_spmv_tmpl_col, LSB_SP_COL of the
 * flags: a 3-D stencil whose planes are whole slices); 0 = no plan, the flag changes nothing */
unsigned long long lsb_hip_solver_spmv_col_slices(const lsb_hip_solver *s);
/* 16-bit sliced-ELL form in use: slots that keep their 128 values / all slots of the
 * first shard (lsb_sell16_value_slots); 0 / 0 for every other form */
void lsb_hip_solver_sell_value_slots(const lsb_hip_solver *s, unsigned *kept, unsigned *total);
/* 1 when the halo exchange of this solver runs behind its interior rows. */
int lsb_hip_solver_overlaps(const lsb_hip_solver *s);
/* 0 one shard; 1 RCCL (device copies between virtual shards); 2 direct xGMI
 * stores for the all-reduces; 3 for the halo exchange as well.  p2p_us/rccl_us
 * (may be NULL): what one exchange + all-reduce cost each way in the
 * creation-time self-test, 0 if it did not run. */
int lsb_hip_solver_comm(const lsb_hip_solver *s, double *p2p_us, double *rccl_us);
/* The exchange plan of this process's first shard, as a scaling line has to show it:
 * plan[0] ranks RCCL counts in the communicator (ncclCommCount; 0 = no communicator),
 * plan[1] peers it receives halos from, plan[2] peers it sends to, plan[3] / plan[4] bytes
 * received / sent per exchange (= per SpMV), plan[5] 1 when the plan is the in-place
 * all-gather (every shard needs every row), 0 for point-to-point halos, plan[6] shards
 * in this process, plan[7] 1 when the halo travels behind the interior rows. */
void lsb_hip_solver_comm_plan(const lsb_hip_solver *s, unsigned long long plan[8]);
/* opts.overlap = -1: the creation-time timing of the sharded SpMV's two forms on the real
 * communicator (hip_dist.c overlap_setup): us[0] per iteration with the SpMV behind the exchange,
 * us[1] with the interior rows in front of the halo (slowest rank's, 0 where the pass did not run).
 * Returns the form in use: 1 split, 0 plain. */
int lsb_hip_solver_overlap(const lsb_hip_solver *s, double us[2]);
/* Matrix-side bytes ONE launch of the SpMV form in use must stream (its index, code, slot
 * and value arrays as stored) + x read once + y written once, first shard; 0 for the
 * multi-pass forms (binned, two-phase).  SURVEY 8(d)'s CSR count is 12 nnz + 20 n + 4. */
unsigned long long lsb_hip_solver_spmv_layout_bytes(const lsb_hip_solver *s);
/* Bytes one iteration of the Krylov loop must move on this rank's first shard: the SpMV's layout
 * bytes + 8 B per row and vector pass of the sweeps (classic PCG: 9 passes, + 2 where the inverse
 * diagonal is a vector; single-reduction PCG: 9 or 11 + 1; BiCGSTAB: TWO layout counts + the 18
 * passes of its four sweeps, + 2 where the diagonal is a vector).  0 where the iteration has another
 * shape (GMRES, Chebyshev / block-Jacobi / FSAI, the fused forms of small operators, fp32 values,
 * multi-pass SpMV forms).  bench.py divides it by the measured time per iteration. */
unsigned long long lsb_hip_solver_iteration_bytes(const lsb_hip_solver *s);
/* 1: the PCG iteration runs in its single-reduction form (Chronopoulos & Gear; two launches, one
 * reduction per iteration) -- every sharded solve under krylov = auto, and one-shard solves of
 * large operators whose Jacobi diagonal is one constant; 0: the classic form (or GMRES). */
int lsb_hip_solver_single_reduction(const lsb_hip_solver *s);
/* 0: an iteration's direction update p = D^-1 r + beta p is a launch of its own; 1: it rides in the
 * NEXT iteration's SpMV launch, formed for every gathered operand (the sub-wavefront form of
 * launch-bound operators). */
int lsb_hip_solver_fused_p(const lsb_hip_solver *s);
/* Which operands of the BLAS-1 sweeps this solver loads nontemporal (bit 0 x, 1 p and q, 2 r in
 * k_pcg_update_xr; 3 r, 4 p in k_pcg_update_p; 5 k_cg1_update): timed at creation on the solver's
 * first shard, or LSBENCH_HIP_BLAS1_NT. */
int lsb_hip_solver_blas1_nt(const lsb_hip_solver *s);
/* hipStream_t of the backend (as void*), for callers that time with events. */
void *lsb_hip_stream(void);

/* ------------------------------------------------------------------------ */
/* Multi-GPU: one process per GPU, RCCL over xGMI                            */
/* ------------------------------------------------------------------------ */

#define LSB_HIP_UNIQUE_ID_BYTES 128
/* Rank 0 calls get_unique_id and ships the 128 bytes to the other ranks by
 * whatever side channel the launcher offers (bench.py: torch.distributed
 * broadcast); then every rank calls init_rank. */
int lsb_hip_comm_get_unique_id(void *id128);
int lsb_hip_comm_init_rank(const void *id128, int nranks, int rank);
int lsb_hip_comm_destroy(void);
int lsb_hip_comm_rank(void);
int lsb_hip_comm_size(void);
/* What RCCL itself says (ncclCommCount on this thread's communicator); 0 without one. */
int lsb_hip_comm_count(void);
/* In-place sum of `count` doubles over all ranks, device buffer, on the
 * backend stream; and a barrier built from it. */
int lsb_hip_comm_allreduce_sum_dev(double *d_buf, int count);
int lsb_hip_comm_barrier(void);

/* ------------------------------------------------------------------------ */
/* 3. Kernel-level entry points (device pointers; stream = hipStream_t)      */
/* ------------------------------------------------------------------------ */

/* y = A x for a 0-based int32 CSR.  variant = LSB_SPMV_*; d_rowblk/nblk from
 * lsb_csr_row_blocks (needed by ADAPTIVE, ignored otherwise); d_blklanes from
 * lsb_csr_block_lanes or NULL (lanes then follow the row count alone);
 * flags: bit 0 = prefetch the next block, bit 1 = nontemporal stream loads.
 * If d_dot != NULL the kernel also leaves sum_i xdot[i]*y[i] in d_dot[0]
 * (two-stage, fixed order; d_work must then hold
 * lsb_hip_partials_capacity() doubles). */
/* LSB_SPMV_SELL: pass the device copies of lsb_sell's sptr as d_offs, cols as
 * d_cols, vals as d_vals and nslice as nblk (d_rowblk, d_blklanes unused).
 * With flags & LSB_SPMV_FLAG_C16 (the 16-bit form, row_begin = 0): codes as
 * d_cols and sbase as d_rowblk. */
#define LSB_SPMV_FLAG_PREFETCH 1u
#define LSB_SPMV_FLAG_NT 2u
#define LSB_SPMV_FLAG_C16 4u
int lsb_hip_spmv_csr_f64(int variant, unsigned n, const int *d_offs,
                         const int *d_cols, const double *d_vals,
                         const int *d_rowblk, const unsigned char *d_blklanes,
                         unsigned nblk, unsigned mean_row_len, unsigned flags,
                         const double *d_x, double *d_y,
                         const double *d_xdot, double *d_dot, double *d_work,
                         void *stream);
unsigned lsb_hip_partials_capacity(void);
/* d_out[0] = sum a_i b_i (deterministic two-stage reduction). */
int lsb_hip_dot_f64(unsigned n, const double *d_a, const double *d_b,
                    double *d_out, double *d_work, void *stream);
/* d_out[0] = sqrt(sum a_i^2). */
int lsb_hip_nrm2_f64(unsigned n, const double *d_a, double *d_out,
                     double *d_work, void *stream);
/* y += alpha x, alpha read from device memory (no host sync). */
int lsb_hip_axpy_f64(unsigned n, const double *d_alpha, const double *d_x,
                     double *d_y, void *stream);
/* y = x + beta y, beta read from device memory. */
int lsb_hip_xpay_f64(unsigned n, const double *d_beta, const double *d_x,
                     double *d_y, void *stream);
/* dinv[i] = 1 / A(i, i + row_begin); *d_nzero counts rows without a usable
 * diagonal (their dinv is set to 0). */
int lsb_hip_jacobi_setup_f64(unsigned n, unsigned row_begin, const int *d_offs,
                             const int *d_cols, const double *d_vals,
                             double *d_dinv, int *d_nzero, void *stream);
/* z = dinv .* r */
int lsb_hip_jacobi_apply_f64(unsigned n, const double *d_dinv,
                             const double *d_r, double *d_z, void *stream);

/* Device memory helpers so that a C caller without HIP headers can drive the
 * kernel-level API (tests use torch tensors instead). */
void *lsb_hip_malloc(size_t bytes);
void lsb_hip_free(void *d_ptr);
int lsb_hip_memcpy_h2d(void *d_dst, const void *src, size_t bytes);
int lsb_hip_memcpy_d2h(void *dst, const void *d_src, size_t bytes);
int lsb_hip_sync(void);

#ifdef __cplusplus
}
#endif

#endif /* LSBENCH_HIP_H */
