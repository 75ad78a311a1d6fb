// Block-CG proper: the kernels of lsb_hip_solver_solve_block[_dev] (driver: hip_bcg_drv.c).  ONE Krylov space for the
// KP = 2, 4 or 8 columns of a block: preconditioned BCGrQ, the residual block kept factored as R = W sigma with
// W^T D^-1 W = I (Cholesky-QR in the D^-1 inner product), D^-1 the solver's diagonal preconditioner, x0 = 0.
//
//   start: G = B^T D^-1 B, bb_c = b_c . b_c (k_bcg_init) ; L L^T = G, sigma = L^T (k_bcg_small<START>) ;
//          W = B sigma^-1, P = D^-1 W, X = 0 (k_bcg_start)
//   iter:  Q = S P, Gamma = P^T Q                                        k_bcg_spmm
//          C C^T = Gamma, xi = Gamma^-1, xs = xi sigma                   k_bcg_small<GAMMA>
//          X += P xs, W~ = W - Q xi, G = W~^T D^-1 W~, H = W~^T W~       k_bcg_pass_a
//          rr_c = sigma_c^T H sigma_c, the stop test ; L L^T = G,
//          zeta = L^T, zeta^-1, sigma = zeta sigma                       k_bcg_small<G>
//          W = W~ zeta^-1, P = D^-1 W + P zeta^T                         k_bcg_pass_b
//
// Layout: hip_mrhs.hip's interleaved blocks, element (i, c) at i KP + c, packed and un-packed by its kernels.  A row's
// KP values meet a KP x KP matrix, so a lane of the three streaming kernels owns whole ROWS: it takes a row's KP
// doubles of every operand with KP / 2 16-byte loads, and the matrices come out of the state through uniform (scalar)
// loads.  The Gram matrices leave the launches as records of their upper triangle, one record per workgroup.
//
// The small algebra is done ONCE, by the single-workgroup k_bcg_small between the streaming launches (not redone by
// every workgroup of the next pass): it re-reduces the records in an order that depends on their number only (no
// atomics: the same bits from run to run), factors, inverts, multiplies, takes the stop / breakdown / maxit decision
// and writes lsb_blockcg_state.  Nobody else writes the state.  `running` is never written and tested by different
// workgroups of one launch: the SpMM and the passes only read it, and the launch that clears it has one workgroup,
// whose threads have all read it before the first barrier.  Once it is 0 the SpMM stores nothing and every other
// kernel returns at once.  The columns are coupled, so nothing is frozen per column: all run until all meet the stop
// rule.  Columns >= nrhs are the block's padding: zero in every vector, the identity in every small matrix.
#include "hip_kcommon.h"
#include "hip_mrhs_k.h"

#define BS LSB_MRHS_MAX // stride of the small matrices in the state and in LDS
#define WGS 1024        // threads of k_bcg_small: its record sums are a few hundred loads a thread otherwise
// (tri_at, tri_of, the dealt triangle, row_load, row_store, wg_sum_store, pass_grid: hip_mrhs_k.h, shared with
// hip_bcg_m.hip)

// --------------------------------------------------------------------------
// Q = S P by the row rule (block_row_product, hip_mrhs_k.h), so Q has the bits of lsb_hip_solver_spmm_dev on the same
// P.  Every lane of the row's group then takes the row of P and its entries of the upper triangle of p_row^T q_row
// (the dealt triangle, hip_mrhs_k.h).  One record of T doubles per workgroup, rows dealt XCD-contiguously.
// --------------------------------------------------------------------------
template <int L, int KP>
__global__ __launch_bounds__(WG) void k_bcg_spmm(unsigned n, unsigned rows_per_wg, const int *__restrict__ offs,
                                                 const int *__restrict__ cols, const double *__restrict__ vals,
                                                 const double *__restrict__ x, double *__restrict__ y,
                                                 double *__restrict__ records,
                                                 const lsb_blockcg_state *__restrict__ st) {
  constexpr int T = tri_of(KP), NA = tri_dealt(KP, L);
  constexpr unsigned SLOTS = WG / L;
  __shared__ double sred[4 * T];
  const unsigned tid = threadIdx.x, slot = tid / L, l = tid % L;
  const unsigned w = xcd_contiguous_wg();
  const unsigned ra = min(w * rows_per_wg, n), rb = min(ra + rows_per_wg, n);
  const int stopped = !st->running;
  double g[1][NA]; // P^T Q, this lane's entries
#pragma unroll
  for (int k = 0; k < NA; k++)
    g[0][k] = 0.0;
  for (unsigned base = ra; base < rb; base += SLOTS) {
    const unsigned r = base + slot;
    double a[KP];
    block_row_product<L, KP>(offs, cols, vals, x, r, r < rb, l, a);
    if (stopped)
      return;
    if (r < rb) {
      double pr[KP];
      row_load<KP>(x, r, pr);
      if (l == 0)
        row_store<KP>(y, r, a);
      tri_dealt_fma<L, KP>(pr, {a}, l, g);
    }
  }
  if (stopped)
    return;
  tri_dealt_store<L, KP>(g, sred, records + (size_t)w * T);
}

// --------------------------------------------------------------------------
// The streaming launches.  dinv == NULL: the constant dc.
// --------------------------------------------------------------------------
// records of (B^T D^-1 B upper triangle, then b_c . b_c per column)
template <int KP>
__global__ __launch_bounds__(WG) void k_bcg_init(unsigned n, const double *__restrict__ b,
                                                 const double *__restrict__ dinv, double dc,
                                                 double *__restrict__ records) {
  constexpr int T = tri_of(KP), W = T + KP;
  __shared__ double sred[4 * W];
  const size_t gsz = (size_t)gridDim.x * WG;
  double acc[W];
#pragma unroll
  for (int k = 0; k < W; k++)
    acc[k] = 0.0;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += gsz) {
    double bv[KP];
    row_load<KP>(b, i, bv);
    const double d = dinv ? dinv[i] : dc;
#pragma unroll
    for (int r = 0; r < KP; r++) {
      const double db = d * bv[r];
#pragma unroll
      for (int c = r; c < KP; c++)
        acc[tri_at(KP, r, c)] = fma(db, bv[c], acc[tri_at(KP, r, c)]);
      acc[T + r] = fma(bv[r], bv[r], acc[T + r]);
    }
  }
  wg_sum_store<W>(acc, sred, records + (size_t)blockIdx.x * W);
}

// W = B zinv (zinv = sigma^-1, upper triangular), P = D^-1 W, X = 0.  Not gated: X = 0 is the answer of a block that
// does not run (maxit = 0).
template <int KP>
__global__ __launch_bounds__(WG) void k_bcg_start(unsigned n, const double *__restrict__ b,
                                                  const double *__restrict__ dinv, double dc, double *__restrict__ w,
                                                  double *__restrict__ p, double *__restrict__ x,
                                                  const lsb_blockcg_state *__restrict__ st) {
  const size_t gsz = (size_t)gridDim.x * WG;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += gsz) {
    double bv[KP], wv[KP], pv[KP], zero[KP];
    row_load<KP>(b, i, bv);
    const double d = dinv ? dinv[i] : dc;
#pragma unroll
    for (int c = 0; c < KP; c++) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r <= c; r++)
        s = fma(bv[r], st->zinv[r * BS + c], s);
      wv[c] = s, pv[c] = d * s, zero[c] = 0.0;
    }
    row_store<KP>(w, i, wv);
    row_store<KP>(p, i, pv);
    row_store<KP>(x, i, zero);
  }
}

// X += P xs ; W~ = W - Q xi, in place ; one record per workgroup: the upper triangles of W~^T D^-1 W~, then of W~^T W~
template <int KP>
__global__ __launch_bounds__(WG) void k_bcg_pass_a(unsigned n, double *__restrict__ w, const double *__restrict__ q,
                                                   const double *__restrict__ p, double *__restrict__ x,
                                                   const double *__restrict__ dinv, double dc,
                                                   const lsb_blockcg_state *__restrict__ st,
                                                   double *__restrict__ records) {
  constexpr int T = tri_of(KP);
  __shared__ double sred[4 * 2 * T];
  if (!st->running)
    return;
  const size_t gsz = (size_t)gridDim.x * WG;
  double acc[2 * T];
#pragma unroll
  for (int k = 0; k < 2 * T; k++)
    acc[k] = 0.0;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += gsz) {
    double wv[KP], qv[KP];
    row_load<KP>(w, i, wv);
    row_load<KP>(q, i, qv);
    {
      double pv[KP], xv[KP];
      row_load<KP>(p, i, pv);
      row_load<KP>(x, i, xv);
#pragma unroll
      for (int c = 0; c < KP; c++) {
#pragma unroll
        for (int r = 0; r < KP; r++)
          xv[c] = fma(pv[r], st->xs[r * BS + c], xv[c]);
      }
      row_store<KP>(x, i, xv);
    }
    const double d = dinv ? dinv[i] : dc;
#pragma unroll
    for (int c = 0; c < KP; c++) {
#pragma unroll
      for (int r = 0; r < KP; r++)
        wv[c] = fma(-qv[r], st->xi[r * BS + c], wv[c]);
    }
    row_store<KP>(w, i, wv);
#pragma unroll
    for (int r = 0; r < KP; r++) {
      const double dw = d * wv[r];
#pragma unroll
      for (int c = r; c < KP; c++) {
        acc[tri_at(KP, r, c)] = fma(dw, wv[c], acc[tri_at(KP, r, c)]);
        acc[T + tri_at(KP, r, c)] = fma(wv[r], wv[c], acc[T + tri_at(KP, r, c)]);
      }
    }
  }
  wg_sum_store<2 * T>(acc, sred, records + (size_t)blockIdx.x * 2 * T);
}

// W = W~ zinv (upper triangular) ; P = D^-1 W + P zeta^T (zeta upper triangular)
template <int KP>
__global__ __launch_bounds__(WG) void k_bcg_pass_b(unsigned n, double *__restrict__ w, double *__restrict__ p,
                                                   const double *__restrict__ dinv, double dc,
                                                   const lsb_blockcg_state *__restrict__ st) {
  if (!st->running)
    return;
  const size_t gsz = (size_t)gridDim.x * WG;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += gsz) {
    double wt[KP], pv[KP], wv[KP], pn[KP];
    row_load<KP>(w, i, wt);
    row_load<KP>(p, i, pv);
    const double d = dinv ? dinv[i] : dc;
#pragma unroll
    for (int c = 0; c < KP; c++) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r <= c; r++)
        s = fma(wt[r], st->zinv[r * BS + c], s);
      wv[c] = s;
      double t = d * s;
#pragma unroll
      for (int r = c; r < KP; r++) // (P zeta^T)_c = sum_r p_r zeta[c][r], zeta[c][r] = 0 for r < c
        t = fma(pv[r], st->zeta[c * BS + r], t);
      pn[c] = t;
    }
    row_store<KP>(w, i, wv);
    row_store<KP>(p, i, pn);
  }
}

// --------------------------------------------------------------------------
// k_bcg_small: one workgroup of WGS threads sums the records; the algebra behind that is the FIRST WAVEFRONT's alone
// (KP KP <= 64 elements), so its steps are ordered by wave_sync() -- a fence the compiler may not move LDS accesses
// across; the LDS serves one wave's accesses in issue order -- and cost no workgroup barrier.  Matrices in LDS,
// row-major with stride BS; thread t < KP KP is element (t / KP, t % KP).  Every helper below small_sum_records is
// called by all 64 lanes of that wave.
// --------------------------------------------------------------------------
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// a thread's own share of small_sum_records: records s, s + NR, ... of component k, U loads at a time
template <int W, int U>
__device__ __forceinline__ double small_sum_own(const double *__restrict__ parts, unsigned nparts, unsigned s,
                                                unsigned k) {
  constexpr unsigned NR = WGS / W;
  double v = 0.0;
  for (unsigned i = s; i < nparts; i += U * NR) {
    double tv[U];
#pragma unroll
    for (int u = 0; u < U; u++) { // (every element loads: no branch around a load)
      const unsigned r = i + u * NR;
      tv[u] = parts[(size_t)(r < nparts ? r : s) * W + k];
    }
#pragma unroll
    for (int u = 0; u < U; u++)
      v = i + u * NR < nparts ? v + tv[u] : v;
  }
  return v;
}

// sums of `nparts` records of width W per component into sout[W]: thread t takes component t mod W of records
// t / W, t / W + WGS / W, ..., the WGS / W threads of a component are added in ascending order.  sred: WGS doubles.
template <int W>
__device__ __forceinline__ void small_sum_records(const double *__restrict__ parts, unsigned nparts, double *sred,
                                                  double *sout) {
  constexpr unsigned NR = WGS / W;
  const unsigned t = threadIdx.x, k = t % W, s = t / W;
  double v = 0.0;
  if (s < NR) { // U loads in flight per thread; added in ascending order of the record whatever U is
    if (nparts > 4 * NR)
      v = small_sum_own<W, 16>(parts, nparts, s, k);
    else
      v = small_sum_own<W, 4>(parts, nparts, s, k);
  }
  __syncthreads();
  sred[t] = v;
  __syncthreads();
  if (t < W) {
    double a = 0.0;
    for (unsigned j = 0; j < NR; j++)
      a += sred[j * W + t];
    sout[t] = a;
  }
  __syncthreads();
}

// the symmetric matrix of an upper-triangle record, the identity on the padding
template <int KP> __device__ __forceinline__ void small_sym(const double *tri, unsigned nrhs, double *A) {
  const unsigned t = threadIdx.x;
  if (t < KP * KP) {
    const unsigned i = t / KP, j = t % KP, lo = i < j ? i : j, hi = i < j ? j : i;
    double v = tri[lo * KP - lo * (lo - 1) / 2 + (hi - lo)];
    if (i == j && i >= nrhs)
      v = 1.0;
    A[i * BS + j] = v;
  }
  wave_sync();
}

// A = L L^T in place (right-looking; the upper triangle zeroed).  A pivot that is not > floor, or not finite, sets
// *sbad; *spiv: the smallest pivot.  The factor of a matrix that failed holds garbage, and nobody uses it.
template <int KP> __device__ __forceinline__ int small_chol(double *A, double floor, int *sbad, double *spiv) {
  const unsigned t = threadIdx.x, i = t / KP, k = t % KP;
  if (t == 0)
    *sbad = 0, *spiv = INFINITY;
  wave_sync();
  for (unsigned j = 0; j < KP; j++) {
    if (t == 0) {
      const double d = A[j * BS + j];
      if (!(d > floor) || !isfinite(d))
        *sbad = 1;
      if (!(d >= *spiv))
        *spiv = d;
      A[j * BS + j] = sqrt(d);
    }
    wave_sync();
    if (t > j && t < KP)
      A[t * BS + j] /= A[j * BS + j];
    wave_sync();
    if (t < KP * KP && i > j && k > j && k <= i)
      A[i * BS + k] -= A[i * BS + j] * A[k * BS + j];
    wave_sync();
  }
  if (t < KP * KP && k > i)
    A[i * BS + k] = 0.0;
  wave_sync();
  return *sbad;
}

// Linv = L^-1 of a lower triangular L: thread c < KP forms column c by forward substitution
template <int KP> __device__ __forceinline__ void small_linv(const double *Lm, double *Linv) {
  const unsigned c = threadIdx.x;
  if (c < KP) {
    for (unsigned i = 0; i < c; i++)
      Linv[i * BS + c] = 0.0;
    Linv[c * BS + c] = 1.0 / Lm[c * BS + c];
    for (unsigned i = c + 1; i < KP; i++) {
      double s = 0.0;
      for (unsigned m = c; m < i; m++)
        s = fma(Lm[i * BS + m], Linv[m * BS + c], s);
      Linv[i * BS + c] = -s / Lm[i * BS + i];
    }
  }
  wave_sync();
}

template <int KP> __device__ __forceinline__ void small_all_status(lsb_blockcg_state *st, int status) {
  for (unsigned c = 0; c < (unsigned)st->nrhs; c++)
    st->status[c] = status;
}

template <int KP, int PHASE>
__global__ __launch_bounds__(WGS) void k_bcg_small(lsb_blockcg_state *__restrict__ st,
                                                   const double *__restrict__ records, unsigned nrecords,
                                                   unsigned nrhs_in, double tol_in, int maxit_in) {
  constexpr int T = tri_of(KP);
  constexpr int W = PHASE == LSB_BLOCKCG_START ? T + KP : PHASE == LSB_BLOCKCG_GAMMA ? T
                    : PHASE == LSB_BLOCKCG_G   ? 2 * T : KP;
  __shared__ double sred[WGS], sout[W], A[BS * BS], Bm[BS * BS], Cm[BS * BS], Sg[BS * BS], srr[BS], spiv;
  __shared__ int sbad, sstop;
  const unsigned t = threadIdx.x, i = t / KP, j = t % KP;
  const bool el = t < KP * KP;
  if constexpr (PHASE == LSB_BLOCKCG_GAMMA || PHASE == LSB_BLOCKCG_G) {
    if (!st->running) // every thread reads the word before the first barrier; thread 0 writes it behind the last one
      return;
  }
  const unsigned nrhs = PHASE == LSB_BLOCKCG_START ? nrhs_in : (unsigned)st->nrhs;
  small_sum_records<W>(records, nrecords, sred, sout);
  if (t >= 64) // the algebra is the first wavefront's; no workgroup barrier lies behind this line
    return;

  if constexpr (PHASE == LSB_BLOCKCG_START) {
    // G scaled to unit diagonal (a zero diagonal: 0 / 0, a pivot that is not finite), factored; L = diag(d) Ls
    small_sym<KP>(sout, nrhs, A);
    if (t < KP)
      srr[t] = sqrt(A[t * BS + t]);
    wave_sync();
    if (el)
      Bm[i * BS + j] = A[i * BS + j] / (srr[i] * srr[j]);
    wave_sync();
    const int bad = small_chol<KP>(Bm, 1e-10, &sbad, &spiv);
    if (el)
      A[i * BS + j] = srr[i] * Bm[i * BS + j]; // L
    wave_sync();
    small_linv<KP>(A, Cm); // L^-1
    // every matrix of the state starts as the identity, so that what lies beyond KP stays it
    for (unsigned e = t; e < BS * BS; e += 64) {
      const double id = e / BS == e % BS ? 1.0 : 0.0;
      st->xi[e] = id, st->xs[e] = id, st->zeta[e] = id, st->zinv[e] = id, st->sigma[e] = id;
    }
    wave_sync();
    if (el && !bad) {
      st->sigma[i * BS + j] = A[j * BS + i]; // sigma = L^T
      st->zeta[i * BS + j] = A[j * BS + i];
      st->zinv[i * BS + j] = Cm[j * BS + i]; // sigma^-1 = (L^-1)^T
    }
    if (t < BS) {
      const bool mine = t < nrhs;
      const double bb = mine ? sout[T + t] : 0.0;
      st->bb[t] = bb, st->rr[t] = bb, st->thresh2[t] = tol_in * tol_in * bb;
      st->true_relres[t] = -1.0;
      st->status[t] = !mine ? LSB_STATUS_CONVERGED
                      : bad ? LSB_STATUS_BREAKDOWN
                            : (maxit_in <= 0 ? LSB_STATUS_MAXIT : LSB_STATUS_RUNNING);
    }
    if (t == 0) {
      st->tol = tol_in, st->min_pivot = spiv;
      st->iters = 0, st->maxit = maxit_in, st->nrhs = (int)nrhs;
      st->running = !bad && maxit_in > 0;
      st->nspmm = 0;
      st->rank_bad = bad;
    }
  }

  if constexpr (PHASE == LSB_BLOCKCG_GAMMA) {
    small_sym<KP>(sout, nrhs, A);
    if (el)
      Sg[i * BS + j] = st->sigma[i * BS + j];
    const int bad = small_chol<KP>(A, 0.0, &sbad, &spiv); // Gamma = C C^T
    small_linv<KP>(A, Cm);                                // C^-1
    if (el) {                                             // xi = C^-T C^-1
      double s = 0.0;
      for (unsigned m = (i > j ? i : j); m < KP; m++)
        s = fma(Cm[m * BS + i], Cm[m * BS + j], s);
      Bm[i * BS + j] = s;
    }
    wave_sync();
    if (el && !bad) {
      double s = 0.0; // xs = xi sigma, sigma upper triangular
      for (unsigned m = 0; m <= j; m++)
        s = fma(Bm[i * BS + m], Sg[m * BS + j], s);
      st->xi[i * BS + j] = Bm[i * BS + j];
      st->xs[i * BS + j] = s;
    }
    if (t == 0) {
      st->nspmm += 1; // the SpMM in front of this launch worked
      if (bad) {
        small_all_status<KP>(st, LSB_STATUS_BREAKDOWN);
        st->running = 0;
      }
    }
  }

  if constexpr (PHASE == LSB_BLOCKCG_G) {
    small_sym<KP>(sout, nrhs, A);      // G
    small_sym<KP>(sout + T, nrhs, Bm); // H
    if (el)
      Sg[i * BS + j] = st->sigma[i * BS + j];
    wave_sync();
    if (t < KP) { // rr_c = sigma_c^T H sigma_c, sigma_c: column c of the sigma the residual was factored with
      double s = 0.0;
      for (unsigned a = 0; a <= t; a++) {
        double u = 0.0;
        for (unsigned b = 0; b <= t; b++)
          u = fma(Bm[a * BS + b], Sg[b * BS + t], u);
        s = fma(Sg[a * BS + t], u, s);
      }
      srr[t] = s;
    }
    wave_sync();
    if (t == 0) {
      const int it = st->iters + 1;
      st->iters = it;
      int all = 1;
      for (unsigned c = 0; c < nrhs; c++) {
        st->rr[c] = srr[c];
        all &= srr[c] <= st->thresh2[c];
      }
      int stop = 0;
      if (all) {
        small_all_status<KP>(st, LSB_STATUS_CONVERGED);
        stop = 1;
      } else if (it >= st->maxit) {
        for (unsigned c = 0; c < nrhs; c++)
          st->status[c] = srr[c] <= st->thresh2[c] ? LSB_STATUS_CONVERGED : LSB_STATUS_MAXIT;
        stop = 1;
      }
      if (stop)
        st->running = 0;
      sstop = stop;
    }
    wave_sync();
    if (sstop)
      return;
    const int bad = small_chol<KP>(A, 0.0, &sbad, &spiv); // G = L L^T
    small_linv<KP>(A, Cm);                                // L^-1
    if (el && !bad) {
      double s = 0.0; // sigma = zeta sigma, zeta = L^T: sum_m L[m][i] sigma[m][j], i <= m <= j
      for (unsigned m = i; m <= j && m < KP; m++)
        s = fma(A[m * BS + i], Sg[m * BS + j], s);
      st->sigma[i * BS + j] = s;
      st->zeta[i * BS + j] = A[j * BS + i];
      st->zinv[i * BS + j] = Cm[j * BS + i];
    }
    if (t == 0 && bad) {
      small_all_status<KP>(st, LSB_STATUS_BREAKDOWN);
      st->running = 0;
    }
  }

  if constexpr (PHASE == LSB_BLOCKCG_VERIFY) {
    // the residual recomputed from x: a column called converged that misses the tolerance is MAXIT (no restart)
    if (t < nrhs && st->bb[t] > 0.0) {
      const double tr = sqrt(sout[t] / st->bb[t]);
      st->true_relres[t] = tr;
      if (st->status[t] == LSB_STATUS_CONVERGED && !(tr <= st->tol))
        st->status[t] = LSB_STATUS_MAXIT;
    }
  }
}

// --------------------------------------------------------------------------
// Launchers (C ABI).  kp: 2, 4 or 8.
// --------------------------------------------------------------------------
template <int KP>
static void bcg_spmm_launch(unsigned lanes, unsigned g, unsigned n, const int *offs, const int *cols,
                            const double *vals, const double *p, double *q, double *records,
                            const struct lsb_blockcg_state *st, hipStream_t s) {
  ROW_KERNEL_LAUNCH(lanes, (k_bcg_spmm<L, KP>), g, s, n, offs, cols, vals, p, q, records, st);
}

template <int KP>
static void bcg_small_launch(int phase, struct lsb_blockcg_state *st, const double *records, unsigned nrecords,
                             unsigned nrhs, double tol, int maxit, hipStream_t s) {
  switch (phase) {
  case LSB_BLOCKCG_START:
    k_bcg_small<KP, LSB_BLOCKCG_START><<<1, WGS, 0, s>>>(st, records, nrecords, nrhs, tol, maxit);
    break;
  case LSB_BLOCKCG_GAMMA:
    k_bcg_small<KP, LSB_BLOCKCG_GAMMA><<<1, WGS, 0, s>>>(st, records, nrecords, nrhs, tol, maxit);
    break;
  case LSB_BLOCKCG_G:
    k_bcg_small<KP, LSB_BLOCKCG_G><<<1, WGS, 0, s>>>(st, records, nrecords, nrhs, tol, maxit);
    break;
  case LSB_BLOCKCG_VERIFY:
    k_bcg_small<KP, LSB_BLOCKCG_VERIFY><<<1, WGS, 0, s>>>(st, records, nrecords, nrhs, tol, maxit);
    break;
  default:
    errx(EXIT_FAILURE, "hip_bcg: no phase %d", phase);
  }
}

extern "C" {

unsigned lsb_k_blockcg_tri(unsigned kp) { return kp * (kp + 1) / 2; }

void lsb_k_blockcg_init(unsigned kp, unsigned n, const double *b, const double *dinv, double dc, double *records,
                        unsigned *nrecords, void *stream) {
  const unsigned g = pass_grid(n);
  *nrecords = g;
  KP_DISPATCH(kp, (k_bcg_init<KP><<<g, WG, 0, (hipStream_t)stream>>>(n, b, dinv, dc, records)));
}

void lsb_k_blockcg_small(unsigned kp, int phase, struct lsb_blockcg_state *st, const double *records,
                         unsigned nrecords, unsigned nrhs, double tol, int maxit, void *stream) {
  KP_DISPATCH(kp, (bcg_small_launch<KP>(phase, st, records, nrecords, nrhs, tol, maxit, (hipStream_t)stream)));
}

void lsb_k_blockcg_start(unsigned kp, unsigned n, const double *b, const double *dinv, double dc, double *w, double *p,
                         double *x, const struct lsb_blockcg_state *st, void *stream) {
  KP_DISPATCH(kp, (k_bcg_start<KP><<<pass_grid(n), WG, 0, (hipStream_t)stream>>>(n, b, dinv, dc, w, p, x, st)));
}

void lsb_k_blockcg_spmm(unsigned kp, unsigned n, const int *offs, const int *cols, const double *vals, unsigned lanes,
                        const double *p, double *q, double *records, unsigned *nrecords,
                        const struct lsb_blockcg_state *st, void *stream) {
  const unsigned L = row_lanes(lanes), g = lsb_k_spmm_grid(n, L);
  *nrecords = g;
  KP_DISPATCH(kp, (bcg_spmm_launch<KP>(L, g, n, offs, cols, vals, p, q, records, st, (hipStream_t)stream)));
}

void lsb_k_blockcg_pass_a(unsigned kp, unsigned n, double *w, const double *q, const double *p, double *x,
                          const double *dinv, double dc, const struct lsb_blockcg_state *st, double *records,
                          unsigned *nrecords, void *stream) {
  const unsigned g = pass_grid(n);
  *nrecords = g;
  KP_DISPATCH(kp, (k_bcg_pass_a<KP><<<g, WG, 0, (hipStream_t)stream>>>(n, w, q, p, x, dinv, dc, st, records)));
}

void lsb_k_blockcg_pass_b(unsigned kp, unsigned n, double *w, double *p, const double *dinv, double dc,
                          const struct lsb_blockcg_state *st, void *stream) {
  KP_DISPATCH(kp, (k_bcg_pass_b<KP><<<pass_grid(n), WG, 0, (hipStream_t)stream>>>(n, w, p, dinv, dc, st)));
}

} // extern "C"
