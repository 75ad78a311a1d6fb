/*
 * hip_cdna4 -- the MI355X (gfx950) backend of lsbench: host side, plain C.
 *
 * Slots into the reference where every other backend does
 * (src/lsbench-impl.h:42-68): hip_cdna4_init / _finalize / _bench.  The
 * skeleton of _bench is that of the reference's only GPU backend that uploads
 * a raw CSR and writes x back (src/cusparse.c:164-213): untimed csr_init,
 * `trials` warm-up solves, sync, timer, `trials` solves, sync, timer, copy x
 * back, CSV record -- with a Jacobi-preconditioned CG (the Krylov+Jacobi
 * semantics of src/ginkgo.cpp:55-69,91-99: x reset to the initial guess
 * before every trial, reset not timed ... here the reset is fused into the
 * first sweep) made of the hand-written kernels in hip_kernels.hip and hip_sweeps.hip instead of
 * a vendor library call.
 *
 * The operator is what the reference's CHOLMOD path factorises,
 * S = triu(A)+triu(A,1)^T (src/cholmod-impl.h:5-21), so x matches CHOLMOD's
 * answer.
 *
 * Data layout in HBM, per shard (a shard = the contiguous row range one rank
 * owns; one shard per process, or `nvirt` shards on one device in test mode):
 *   offs[n+1] i32, cols[nnz] i32 (GLOBAL column ids), vals[nnz] f64,
 *   rowblk[nblk+1] i32, dinv[n], r[n], q[n] f64,
 *   pfull[n_global] f64  -- the search direction in GLOBAL index space; rows
 *                           [row_begin,row_begin+n) are owned, the rest is
 *                           filled by the exchange step.  SpMV gathers from it
 *                           with the global column ids, so no index
 *                           translation and no halo packing exists.
 *   partial sums + a 64-byte lsb_pcg_state with rz/rr/iters/status.
 * All scalars of the iteration (alpha, beta, stop test) live on the device;
 * the host only enqueues and, every `check_every` iterations, reads the
 * status word.
 */
#define _GNU_SOURCE
#include <ctype.h>
#include <stdarg.h>
#include <stddef.h>
#include <unistd.h>

#include "hip_solver.h"

/* ------------------------------------------------------------------------ */
/* backend globals (reference style: file statics, src/cusparse.c:33-36)     */
/* ------------------------------------------------------------------------ */
int lsb_initialized = 0;
__thread hipStream_t g_stream = 0;
static __thread hipStream_t g_comm_stream = 0;
__thread struct lsb_hip_result g_last;
static struct lsb_hip_opts g_opts;
static int g_opts_set = 0;

void lsb_give_up(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
  fflush(stdout), fflush(stderr);
  _exit(EXIT_FAILURE);
}

double wall_seconds(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

void lsb_hip_opts_default(struct lsb_hip_opts *o) {
  memset(o, 0, sizeof *o);
  o->tol = 1e-12;
  o->maxit = 20000;
  o->op_mode = LSB_OP_CHOLMOD_UPPER;
  o->precond = LSB_PRECOND_JACOBI;
  o->spmv_variant = LSB_SPMV_AUTO;
  o->check_every = 0;
  o->use_graph = 1;
  o->sample_spmv = 0;
  o->nvirt = 1;
  o->comm = LSB_COMM_AUTO;
  o->overlap = -1; /* on where the halos are large enough to pay for the split, DESIGN.md section 6 */
  o->spmv_tune = -1;
  o->spmv_grid = 0;
  o->reorder = 0;
  o->krylov = LSB_KRYLOV_AUTO; /* classic PCG on one shard, single-reduction CG across shards */
  o->restart = 30;
  o->verbose = 0;
  o->ngpus = 1;
  o->verify = 0;
  o->cheb_degree = 4;
  o->block_size = 8;
  o->precision = LSB_PREC_FP64;
  o->persistent = 0; /* measured: 2x slower than the two-launch iteration */
  o->comm_deadline_s = 120.0;
  o->fsai_power = 3;
  o->blas1_nt = -1;
  o->amg_theta = 0.08;
  o->amg_sweeps = 1;
  o->amg_coarse = 256;
  o->amg_max_levels = 20;
  o->amg_tail_rows = 0; /* measured: one workgroup is latency-bound, a launch per step is faster (profiles/r05_amg.txt) */
  o->amg_smoother = LSB_AMG_SMOOTH_L1JACOBI;
  o->amg_cheb_ratio = 10.0;
  o->amg_precision = LSB_AMG_PREC_FP64;
  o->fsai_blocks = 0; /* opt-in: an FSAI solver from default options answers 2 on blocks */
}

/* ONE typed table for everything a caller may set by name: the command line of a host
 * program (hip_cdna4_set_option -- the reference's lsbench_init after integration/
 * hip-flags.patch, the stand-in core's lsbench_init) and the environment
 * (LSBENCH_HIP_<NAME>, '-' -> '_', read once at the first lsb_hip_get_opts). */
enum { OT_DBL, OT_UINT, OT_INT, OT_ENUM };
struct optchoice {
  const char *word;
  int value;
};
static const struct optchoice CH_OPERATOR[] = {{"upper", LSB_OP_CHOLMOD_UPPER}, {"raw", LSB_OP_RAW}, {NULL, 0}};
static const struct optchoice CH_PRECOND[] = {{"jacobi", LSB_PRECOND_JACOBI},   {"none", LSB_PRECOND_NONE},
                                              {"l1", LSB_PRECOND_L1JACOBI},     {"cheb", LSB_PRECOND_CHEBYSHEV},
                                              {"bj", LSB_PRECOND_BLOCKJACOBI},  {"fsai", LSB_PRECOND_FSAI},
                                              {"amg", LSB_PRECOND_AMG},         {"gmg", LSB_PRECOND_GMG},
                                              {NULL, 0}};
static const struct optchoice CH_AMG_SMOOTHER[] = {{"l1", LSB_AMG_SMOOTH_L1JACOBI}, {"cheb", LSB_AMG_SMOOTH_CHEB},
                                                  {"mcgs", LSB_AMG_SMOOTH_MCGS}, {NULL, 0}};
static const struct optchoice CH_AMG_PRECISION[] = {{"fp64", LSB_AMG_PREC_FP64}, {"fp32", LSB_AMG_PREC_FP32}, {NULL, 0}};
static const struct optchoice CH_COMM[] = {{"auto", LSB_COMM_AUTO}, {"rccl", LSB_COMM_RCCL}, {"p2p", LSB_COMM_P2P}, {NULL, 0}};
static const struct optchoice CH_KRYLOV[] = {{"cg", LSB_KRYLOV_PCG},     {"pcg", LSB_KRYLOV_PCG}, /* (alias) */
                                             {"cg1", LSB_KRYLOV_PCG1},   {"pcg1", LSB_KRYLOV_PCG1},
                                             {"auto", LSB_KRYLOV_AUTO},  {"gmres", LSB_KRYLOV_GMRES},
                                             {"bicgstab", LSB_KRYLOV_BICGSTAB}, {"richardson", LSB_KRYLOV_RICHARDSON},
                                             {"direct", LSB_KRYLOV_DIRECT}, {NULL, 0}};
static const struct optchoice CH_PRECISION[] = {{"fp64", LSB_PREC_FP64}, {"fp32", LSB_PREC_MIXED},
                                                {"mixed", LSB_PREC_MIXED}, {NULL, 0}};
#define OPT(n, t, f, c) {n, t, offsetof(struct lsb_hip_opts, f), c}
static const struct optdef {
  const char *name;
  int type;
  size_t off;
  const struct optchoice *choices;
} OPTS[] = {
    OPT("tol", OT_DBL, tol, NULL),
    OPT("maxit", OT_UINT, maxit, NULL),
    OPT("operator", OT_ENUM, op_mode, CH_OPERATOR),
    OPT("nvirt", OT_INT, nvirt, NULL),
    OPT("graph", OT_INT, use_graph, NULL),
    OPT("spmv", OT_INT, spmv_variant, NULL),
    OPT("precond", OT_ENUM, precond, CH_PRECOND),
    OPT("comm", OT_ENUM, comm, CH_COMM),
    OPT("overlap", OT_INT, overlap, NULL),
    OPT("reorder", OT_INT, reorder, NULL),
    OPT("krylov", OT_ENUM, krylov, CH_KRYLOV),
    OPT("restart", OT_INT, restart, NULL),
    OPT("spmv-tune", OT_INT, spmv_tune, NULL),
    OPT("spmv-grid", OT_INT, spmv_grid, NULL),
    OPT("check-every", OT_INT, check_every, NULL),
    OPT("verbose", OT_INT, verbose, NULL),
    OPT("ngpus", OT_INT, ngpus, NULL),
    OPT("verify", OT_INT, verify, NULL),
    OPT("cheb-degree", OT_INT, cheb_degree, NULL),
    OPT("block-size", OT_INT, block_size, NULL),
    OPT("precision", OT_ENUM, precision, CH_PRECISION),
    OPT("persistent", OT_INT, persistent, NULL),
    OPT("comm-deadline-s", OT_DBL, comm_deadline_s, NULL),
    OPT("fsai-power", OT_INT, fsai_power, NULL),
    OPT("blas1-nt", OT_INT, blas1_nt, NULL),
    OPT("amg-theta", OT_DBL, amg_theta, NULL),
    OPT("amg-sweeps", OT_INT, amg_sweeps, NULL),
    OPT("amg-coarse", OT_INT, amg_coarse, NULL),
    OPT("amg-max-levels", OT_INT, amg_max_levels, NULL),
    OPT("amg-tail-rows", OT_INT, amg_tail_rows, NULL),
    OPT("amg-smoother", OT_ENUM, amg_smoother, CH_AMG_SMOOTHER),
    OPT("amg-cheb-ratio", OT_DBL, amg_cheb_ratio, NULL),
    OPT("amg-precision", OT_ENUM, amg_precision, CH_AMG_PRECISION),
    OPT("fsai-blocks", OT_INT, fsai_blocks, NULL),
};
#undef OPT
#define NOPTS (sizeof OPTS / sizeof OPTS[0])
/* --direct-tiers K (LSBENCH_HIP_DIRECT_TIERS): not a member of struct lsb_hip_opts, whose layout stays; the tiers of
 * the direct solver's inverse factor that hip_cdna4_bench asks lsb_hip_solver_create_direct for under --krylov direct:
 * 1 (the default) = the single skyline of lsb_hip_solver_create, 0 = the fewest that fit the entry budget */
static int g_direct_tiers = 1, g_direct_tiers_set;

static int direct_tiers_assign(const char *value) {
  char *end = NULL;
  const long v = value && *value ? strtol(value, &end, 10) : -1;
  if (!end || *end || v < 0 || v > LSB_DIRECT_MAX_TIERS)
    return 1;
  g_direct_tiers = (int)v, g_direct_tiers_set = 1;
  return 0;
}

static int direct_tiers(void) {
  const char *e;
  if (!g_direct_tiers_set) {
    g_direct_tiers_set = 1;
    if ((e = getenv("LSBENCH_HIP_DIRECT_TIERS")) && direct_tiers_assign(e))
      warnx("hip_cdna4: LSBENCH_HIP_DIRECT_TIERS=%s is not a value of option `direct-tiers' (0 .. %d); ignored", e,
            LSB_DIRECT_MAX_TIERS);
  }
  return g_direct_tiers;
}

static int opt_name_eq(const char *a, const char *b) { /* case-blind, '-' == '_' */
  for (; *a && *b; a++, b++) {
    const int ca = *a == '_' ? '-' : tolower((unsigned char)*a), cb = *b == '_' ? '-' : tolower((unsigned char)*b);
    if (ca != cb)
      return 0;
  }
  return !*a && !*b;
}

static int opt_assign(struct lsb_hip_opts *o, const struct optdef *d, const char *value) {
  char *field = (char *)o + d->off, *end = NULL;
  if (!value || !*value)
    return 1;
  switch (d->type) {
  case OT_DBL: {
    const double v = strtod(value, &end);
    if (end == value || *end)
      return 1;
    *(double *)field = v;
    return 0;
  }
  case OT_UINT: {
    const unsigned long v = strtoul(value, &end, 10);
    if (end == value || *end)
      return 1;
    *(unsigned *)field = (unsigned)v;
    return 0;
  }
  case OT_INT: {
    const long v = strtol(value, &end, 10);
    if (end == value || *end)
      return 1;
    *(int *)field = (int)v;
    return 0;
  }
  default:
    for (const struct optchoice *c = d->choices; c->word; c++)
      if (!strcasecmp(c->word, value)) {
        *(int *)field = c->value;
        return 0;
      }
    return 1;
  }
}

static void opts_from_env(struct lsb_hip_opts *o) {
  const char *e;
  for (size_t k = 0; k < NOPTS; k++) {
    char var[64] = "LSBENCH_HIP_";
    size_t z = strlen(var);
    for (const char *p = OPTS[k].name; *p && z + 1 < sizeof var; p++)
      var[z++] = *p == '-' ? '_' : (char)toupper((unsigned char)*p);
    var[z] = 0;
    if ((e = getenv(var)) && opt_assign(o, &OPTS[k], e))
      warnx("hip_cdna4: %s=%s is not a value of option `%s'; ignored", var, e, OPTS[k].name);
  }
}

/* Set one option of hip_cdna4_bench by name ("tol", "maxit", "ngpus", "krylov", "operator",
 * "precond", ...: the table above).  What a host program's command line calls: the reference's
 * lsbench_init after integration/hip-flags.patch (src/lsbench.c:84-92 gains --tol, --maxit,
 * --ngpus, ... and hands name + optarg over), the stand-in core's.  0 = set, 1 = unknown name
 * or a value the option does not take (a warning says which). */
int hip_cdna4_set_option(const char *name, const char *value) {
  struct lsb_hip_opts o;
  if (!name)
    return 1;
  lsb_hip_get_opts(&o);
  if (opt_name_eq(name, "direct-tiers")) {
    if (direct_tiers_assign(value)) {
      warnx("hip_cdna4: `%s' is not a value of option `direct-tiers' (0 .. %d)", value ? value : "(null)",
            LSB_DIRECT_MAX_TIERS);
      return 1;
    }
    return 0;
  }
  for (size_t k = 0; k < NOPTS; k++)
    if (opt_name_eq(name, OPTS[k].name)) {
      if (opt_assign(&o, &OPTS[k], value)) {
        warnx("hip_cdna4: `%s' is not a value of option `%s'", value ? value : "(null)", OPTS[k].name);
        return 1;
      }
      lsb_hip_set_opts(&o);
      return 0;
    }
  warnx("hip_cdna4: no option `%s'", name);
  return 1;
}

/* The backend's synthetic operators (BASELINE.json configs 3-5; lsb_synth.c) for a host
 * program whose loader only reads files: the reference's lsbench_matrix_read after
 * integration/hip-flags.patch returns this for a `synth:SPEC' matrix name
 * (src/lsbench-csr.c:29).  The arrays are malloc'ed: lsbench_matrix_free frees them
 * (src/lsbench-csr.c:101-108).  NULL for a spec the generator does not know. */
struct csr *hip_cdna4_matrix_synth(const char *spec) { return lsbench_matrix_synth(spec, 0, 0, NULL); }

void lsb_hip_set_opts(const struct lsb_hip_opts *o) {
  g_opts = *o;
  g_opts_set = 1;
}

void lsb_hip_get_opts(struct lsb_hip_opts *o) {
  if (!g_opts_set) {
    lsb_hip_opts_default(&g_opts);
    opts_from_env(&g_opts);
    g_opts_set = 1;
  }
  *o = g_opts;
}

void lsb_hip_last_result(struct lsb_hip_result *res) { *res = g_last; }

int lsb_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

void *lsb_hip_stream(void) { return (void *)g_stream; }
int lsb_hip_is_initialized(void) { return lsb_initialized; }

int hip_cdna4_init(void) {
  if (lsb_initialized)
    return 1;
  /* lsbench_init calls every backend's init whatever --solver says
   * (src/lsbench.c:143-147): no device => stay uninitialised, quietly. */
  if (lsb_hip_device_count() < 1)
    return 1;
  const char *e = getenv("LSBENCH_HIP_DEVICE");
  if (e)
    LSB_CHK_HIP(hipSetDevice(atoi(e)));
  LSB_CHK_HIP(hipStreamCreate(&g_stream)); /* cf. src/cusparse.c:142 */
  struct lsb_hip_opts o;
  lsb_hip_get_opts(&o);
  lsb_initialized = 1;
  return 0;
}

hipStream_t comm_stream(void) {
  if (!g_comm_stream)
    LSB_CHK_HIP(hipStreamCreate(&g_comm_stream));
  return g_comm_stream;
}

/* a worker thread of hip_multi.c becomes a rank: its own device and stream */
void rank_thread_attach(int device) {
  LSB_CHK_HIP(hipSetDevice(device));
  LSB_CHK_HIP(hipStreamCreate(&g_stream));
}

void rank_thread_detach(void) {
  LSB_CHK_HIP(hipStreamSynchronize(g_stream));
  LSB_CHK_HIP(hipStreamDestroy(g_stream));
  if (g_comm_stream)
    LSB_CHK_HIP(hipStreamDestroy(g_comm_stream));
  g_stream = 0, g_comm_stream = 0;
}

int hip_cdna4_finalize(void) {
  if (!lsb_initialized)
    return 1;
  LSB_CHK_HIP(hipStreamSynchronize(g_stream));
  LSB_CHK_HIP(hipStreamDestroy(g_stream));
  if (g_comm_stream)
    LSB_CHK_HIP(hipStreamDestroy(g_comm_stream));
  g_stream = 0, g_comm_stream = 0;
  lsb_initialized = 0;
  return 0;
}

/* ------------------------------------------------------------------------ */
/* device helpers for C callers                                              */
/* ------------------------------------------------------------------------ */
void *lsb_hip_malloc(size_t bytes) {
  void *p = NULL;
  LSB_CHK_HIP(hipMalloc(&p, bytes ? bytes : 8));
  return p;
}
void lsb_hip_free(void *p) {
  if (p)
    LSB_CHK_HIP(hipFree(p));
}
int lsb_hip_memcpy_h2d(void *d, const void *s, size_t bytes) {
  LSB_CHK_HIP(hipMemcpy(d, s, bytes, hipMemcpyHostToDevice));
  return 0;
}
int lsb_hip_memcpy_d2h(void *d, const void *s, size_t bytes) {
  LSB_CHK_HIP(hipMemcpy(d, s, bytes, hipMemcpyDeviceToHost));
  return 0;
}
int lsb_hip_sync(void) {
  if (!lsb_initialized)
    return 1;
  LSB_CHK_HIP(hipStreamSynchronize(g_stream));
  return 0;
}

void *dev_upload(const void *h, size_t bytes) {
  void *d = lsb_hip_malloc(bytes);
  if (bytes)
    LSB_CHK_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, g_stream));
  return d;
}

/* ------------------------------------------------------------------------ */
/* kernel-level entry points                                                 */
/* ------------------------------------------------------------------------ */
unsigned lsb_hip_partials_capacity(void) { return 2 * LSB_MAX_PARTIALS; }

int lsb_hip_spmv_csr_f64(int variant, unsigned n, const int *d_offs,
                         const int *d_cols, const double *d_vals,
                         const int *d_rowblk, const unsigned char *d_blklanes,
                         unsigned nblk, unsigned mean_row_len, unsigned flags,
                         const double *d_x, double *d_y,
                         const double *d_xdot, double *d_dot, double *d_work,
                         void *stream) {
  if (!lsb_initialized)
    return 1;
  if (variant == LSB_SPMV_AUTO)
    variant = d_rowblk ? LSB_SPMV_ADAPTIVE : LSB_SPMV_SUBWAVE;
  if (variant == LSB_SPMV_ADAPTIVE && (!d_rowblk || nblk == 0))
    return 2;
  if ((variant < LSB_SPMV_ADAPTIVE || variant > LSB_SPMV_SCALAR) && variant != LSB_SPMV_SELL)
    return 2;
  if (n == 0 || (variant == LSB_SPMV_SELL && nblk != (n + LSB_SELL_ROWS - 1) / LSB_SELL_ROWS))
    return 2;
  if (d_dot && (!d_work || !d_xdot))
    return 2;
  const unsigned L = row_lanes(mean_row_len);

  unsigned np = 0;
  if (variant == LSB_SPMV_SELL) {
    if ((flags & LSB_SP_C16) && !d_rowblk)
      return 2; /* the 16-bit form needs its slot bases */
    lsb_k_spmv_sell(flags, 0, 0, (const unsigned *)d_offs, 0, nblk, n, 0, n, d_cols, d_rowblk, d_vals, NULL, 0,
                    d_x, d_y, d_dot ? d_xdot : NULL, d_dot ? d_work : NULL, &np, NULL, NULL, NULL, stream);
  } else
  lsb_k_spmv(variant, n, d_offs, d_cols, d_vals, d_rowblk, d_blklanes, nblk, L, flags, 0,
             d_x, d_y, d_dot ? d_xdot : NULL, d_dot ? d_work : NULL, &np, NULL, NULL, NULL, stream);
  if (d_dot)
    lsb_k_reduce_final(d_work, np, 1, d_dot, 0, NULL, stream);
  return 0;
}

int lsb_hip_dot_f64(unsigned n, const double *d_a, const double *d_b,
                    double *d_out, double *d_work, void *stream) {
  if (!lsb_initialized)
    return 1;
  unsigned np = 0;
  lsb_k_dot(n, d_a, d_b, d_work, &np, stream);
  lsb_k_reduce_final(d_work, np, 1, d_out, 0, NULL, stream);
  return 0;
}

int lsb_hip_nrm2_f64(unsigned n, const double *d_a, double *d_out,
                     double *d_work, void *stream) {
  if (!lsb_initialized)
    return 1;
  unsigned np = 0;
  lsb_k_dot(n, d_a, d_a, d_work, &np, stream);
  lsb_k_reduce_final(d_work, np, 1, d_out, 1, NULL, stream);
  return 0;
}

int lsb_hip_axpy_f64(unsigned n, const double *d_alpha, const double *d_x,
                     double *d_y, void *stream) {
  if (!lsb_initialized)
    return 1;
  lsb_k_axpy(n, d_alpha, d_x, d_y, stream);
  return 0;
}

int lsb_hip_xpay_f64(unsigned n, const double *d_beta, const double *d_x,
                     double *d_y, void *stream) {
  if (!lsb_initialized)
    return 1;
  lsb_k_xpay(n, d_beta, d_x, d_y, stream);
  return 0;
}

int lsb_hip_jacobi_setup_f64(unsigned n, unsigned row_begin, const int *d_offs,
                             const int *d_cols, const double *d_vals,
                             double *d_dinv, int *d_nzero, void *stream) {
  if (!lsb_initialized)
    return 1;
  lsb_k_jacobi_setup(n, row_begin, d_offs, d_cols, d_vals, d_dinv, d_nzero, stream);
  return 0;
}

int lsb_hip_jacobi_apply_f64(unsigned n, const double *d_dinv,
                             const double *d_r, double *d_z, void *stream) {
  if (!lsb_initialized)
    return 1;
  lsb_k_jacobi_apply(n, d_dinv, d_r, d_z, stream);
  return 0;
}

/* ------------------------------------------------------------------------ */
/* the drop-in entry point                                                   */
/* ------------------------------------------------------------------------ */
int hip_cdna4_bench(double *x, struct csr *A, const double *r,
                    const struct lsbench *cb) {
  if (!lsb_initialized)
    return 1;
  struct lsb_hip_opts o;
  lsb_hip_get_opts(&o);
  const unsigned m = A->nrows, nnz = A->offs[m];
  const size_t bytes = (size_t)m * sizeof(double);
  /* several GPUs of the node, driven from this one caller process */
  const int ngpus = o.ngpus == 0 ? lsb_hip_device_count() : o.ngpus;
  if (ngpus > 1)
    return bench_multi(x, A, r, cb, &o, ngpus);

  /* untimed setup: operator build, upload, Jacobi, row blocks
   * (counterpart of csr_init, src/cusparse.c:47-125) */
  lsb_hip_solver *sv = o.krylov == LSB_KRYLOV_DIRECT && direct_tiers() != 1
                           ? lsb_hip_solver_create_direct(A, &o, direct_tiers())
                           : lsb_hip_solver_create(A, &o);
  if (!sv)
    errx(EXIT_FAILURE, "hip_cdna4: cannot set up the solver");
  double *d_r = (double *)lsb_hip_malloc(bytes), *d_x = (double *)lsb_hip_malloc(bytes);
  LSB_CHK_HIP(hipMemcpy(d_r, r, bytes, hipMemcpyHostToDevice));
  LSB_CHK_HIP(hipMemset(d_x, 0, bytes)); /* --trials=0: x stays the initial guess */

  struct lsb_hip_result res;
  memset(&res, 0, sizeof res);
  /* warm-up (src/cholmod-impl.h:44-55, src/cusparse.c:182-186) */
  for (unsigned i = 0; i < cb->trials; i++)
    lsb_hip_solver_solve_dev(sv, d_r, d_x, &res);

  /* timed (src/cusparse.c:189-197).  Wall clock, not clock(): clock() is
   * process CPU time and would not see the device. */
  LSB_CHK_HIP(hipDeviceSynchronize());
  const double t0 = wall_seconds();
  for (unsigned i = 0; i < cb->trials; i++)
    lsb_hip_solver_solve_dev(sv, d_r, d_x, &res);
  LSB_CHK_HIP(hipDeviceSynchronize());
  const double elapsed = wall_seconds() - t0;

  LSB_CHK_HIP(hipMemcpy(x, d_x, bytes, hipMemcpyDeviceToHost)); /* :199 */

  /* the reference's record, verbatim (src/cholmod-impl.h:68-70) ... */
  printf("===matrix,n,nnz,trials,solver,ordering,elapsed===\n");
  printf("%s,%u,%u,%u,%u,%d,%.15lf\n", cb->matrix, m, nnz, cb->trials, cb->solver,
         cb->ordering, elapsed);
  /* ... plus what an iterative backend owes its reader */
  printf("===hip_cdna4:iterations,relres,status,tol,solves_per_sec,nshards===\n");
  printf("%u,%.6e,%d,%.3e,%.6f,%d\n", res.iters, res.relres, res.status, o.tol,
         elapsed > 0 ? cb->trials / elapsed : 0.0, sv->nshard);
  fflush(stdout);

  lsb_hip_free(d_r), lsb_hip_free(d_x);
  lsb_hip_solver_destroy(sv);
  return 0;
}

