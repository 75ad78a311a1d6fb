// AMG as the solver on blocks of right-hand sides (lsb_hip_solver_amg_solve_multi[_dev]; driver: hip_rich_m_drv.c):
// hip_rich.hip's stationary V-cycle iteration per column of an interleaved block of KP = 2, 4 or 8 columns (layout:
// hip_mrhs.hip's, element (i, c) at i KP + c, 16-byte aligned).
//
//   X = 0 ; R = B ; b_c . b_c                        k_richm_init, k_richm_init_state
//   cycle k:  Z = M^-1 R                             one V-cycle on the block (amg_cycle at width KP, fp64 or fp32)
//             Q = S Z                                lsb_k_spmm_csr
//             X += Z ; R -= Q ; records of r_c . r_c k_richm_update
//             per column: rr, iters, the stop test   k_richm_step (one workgroup; clears `running` with the last one)
//
// The state is struct lsb_mrhs_state: c[c] is column c's lsb_pcg_state, used as hip_rich.hip uses the shard's; nspmm
// counts the cycles that did work.  Every launch of a cycle returns at once when `running` is 0, and the state is
// written by k_richm_step alone, a launch of one workgroup between the update and the next cycle's first launch.
//
// A column that has stopped is frozen: its x and r are no longer stored (store_pairs, hip_mrhs_k.h), its iters and rr
// no longer written.  The cycle and the SpMM compute it along with the rest and nobody reads the result.
//
// Summation order: the sweeps deal the element pairs (2 i, 2 i + 1) of a COLUMN to threads and workgroups exactly as
// hip_rich.hip's do -- grid lsb_k_blas1_grid(n) whatever the width, pair i to thread i mod (grid WG), the odd last
// element to the last thread, the chain acc = fma(v_hi, v_hi, fma(v_lo, v_lo, acc)) -- and the records, KP doubles per
// workgroup, are summed again per component in wg_sum_partials' order.  So a column's b.b and r.r are the bits of
// k_rich_init's and k_rich_update's on that column alone: they do not depend on the neighbours or on the width.
#include "hip_kcommon.h"
#include "hip_mrhs_k.h"

#define RICHM_HIDDEN __attribute__((visibility("hidden")))

#define RICHM_IDX                                                   \
  constexpr int H = KP / 2;                                         \
  const size_t gtid = (size_t)blockIdx.x * WG + threadIdx.x;        \
  const size_t gsz = (size_t)gridDim.x * WG;                        \
  const size_t n2 = n / 2;                                          \
  const bool tail = (n & 1) && gtid == gsz - 1 /* the odd last row: the last thread's */

// the workgroup's record: KP sums
template <int KP>
__device__ __forceinline__ void richm_record(double (&acc)[KP], double *sred, double *__restrict__ records) {
  wg_sum<KP>(acc, sred);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < KP; k++)
      records[(size_t)blockIdx.x * KP + k] = acc[k];
  }
}

// X = 0 ; R = B ; records of b_c . b_c
template <int KP>
__global__ __launch_bounds__(WG) void k_richm_init(unsigned n, const double *__restrict__ b, double *__restrict__ x,
                                                   double *__restrict__ r, double *__restrict__ records) {
  __shared__ double sred[4 * KP];
  RICHM_IDX;
  const d2v *b2 = (const d2v *)b;
  d2v *x2 = (d2v *)x, *r2 = (d2v *)r;
  double acc[KP];
#pragma unroll
  for (int k = 0; k < KP; k++)
    acc[k] = 0.0;
  for (size_t i = gtid; i < n2; i += gsz) {
#pragma unroll
    for (int lohi = 0; lohi < 2; lohi++) {
#pragma unroll
      for (int h = 0; h < H; h++) {
        const size_t j = (2 * i + lohi) * H + h;
        const d2v bv = b2[j];
        x2[j] = d2v{0.0, 0.0};
        r2[j] = bv;
        acc[2 * h] = fma(bv.x, bv.x, acc[2 * h]);
        acc[2 * h + 1] = fma(bv.y, bv.y, acc[2 * h + 1]);
      }
    }
  }
  if (tail) {
#pragma unroll
    for (int h = 0; h < H; h++) {
      const size_t j = (size_t)(n - 1) * H + h;
      const d2v bv = b2[j];
      x2[j] = d2v{0.0, 0.0};
      r2[j] = bv;
      acc[2 * h] = fma(bv.x, bv.x, acc[2 * h]);
      acc[2 * h + 1] = fma(bv.y, bv.y, acc[2 * h + 1]);
    }
  }
  richm_record<KP>(acc, sred, records);
}

// one workgroup: b.b starts every column's state (not gated: the state still holds the previous block's)
template <int KP>
__global__ __launch_bounds__(WG) void k_richm_init_state(lsb_mrhs_state *__restrict__ st,
                                                         const double *__restrict__ parts, unsigned nparts, double tol,
                                                         int maxit) {
  __shared__ double sred[4 * KP];
  double v[KP];
  wg_sum_partials<KP>(parts, nparts, v, sred);
  if (threadIdx.x != 0)
    return;
  int run = 0;
#pragma unroll
  for (int k = 0; k < KP; k++) {
    lsb_pcg_state *c = &st->c[k];
    const double bb = v[k];
    c->rz[0] = c->rz[1] = c->pq = c->alpha[0] = c->alpha[1] = 0.0; // (the PCG forms' words: not used)
    c->bb = bb, c->thresh2 = tol * tol * bb, c->rr = bb;
    c->iters = 0, c->maxit = maxit;
    c->pad = c->xpend = 0;
    // b == 0 => x = 0 is the solution; maxit == 0 => nothing to do (as k_rich_init_state)
    c->status = bb == 0.0 ? LSB_STATUS_CONVERGED : (maxit <= 0 ? LSB_STATUS_MAXIT : LSB_STATUS_RUNNING);
    run |= c->status == LSB_STATUS_RUNNING;
    st->true_relres[k] = -1.0, st->start_relres[k] = 0.0;
    st->corrections[k] = 0;
  }
  st->tol = tol;
  st->nspmm = 0;
  st->running = run;
}

// X += Z ; R -= Q ; records of r_c . r_c -- of the running columns; a frozen column is not stored
template <int KP>
__global__ __launch_bounds__(WG) void k_richm_update(unsigned n, const double *__restrict__ z,
                                                     const double *__restrict__ q, double *x, double *r,
                                                     const lsb_mrhs_state *__restrict__ st,
                                                     double *__restrict__ records) {
  __shared__ double sred[4 * KP];
  RICHM_IDX;
  if (!st->running)
    return;
  int act[KP];
#pragma unroll
  for (int k = 0; k < KP; k++)
    act[k] = st->c[k].status == LSB_STATUS_RUNNING;
  const d2v *z2 = (const d2v *)z, *q2 = (const d2v *)q, *x2 = (const d2v *)x, *r2 = (const d2v *)r;
  double acc[KP];
#pragma unroll
  for (int k = 0; k < KP; k++)
    acc[k] = 0.0;
  for (size_t i = gtid; i < n2; i += gsz) {
#pragma unroll
    for (int lohi = 0; lohi < 2; lohi++) {
#pragma unroll
      for (int h = 0; h < H; h++) {
        const int a0 = act[2 * h], a1 = act[2 * h + 1];
        if (a0 | a1) {
          const size_t j = (2 * i + lohi) * H + h;
          const d2v xv = x2[j], zv = z2[j], rv = r2[j], qv = q2[j];
          const d2v xn = {xv.x + zv.x, xv.y + zv.y}, rn = {rv.x - qv.x, rv.y - qv.y};
          store_pairs({x, r}, {xn, rn}, j, a0, a1);
          acc[2 * h] = fma(rn.x, rn.x, acc[2 * h]);
          acc[2 * h + 1] = fma(rn.y, rn.y, acc[2 * h + 1]);
        }
      }
    }
  }
  if (tail) {
#pragma unroll
    for (int h = 0; h < H; h++) {
      const int a0 = act[2 * h], a1 = act[2 * h + 1];
      if (a0 | a1) {
        const size_t j = (size_t)(n - 1) * H + h;
        const d2v xv = x2[j], zv = z2[j], rv = r2[j], qv = q2[j];
        const d2v xn = {xv.x + zv.x, xv.y + zv.y}, rn = {rv.x - qv.x, rv.y - qv.y};
        store_pairs({x, r}, {xn, rn}, j, a0, a1);
        acc[2 * h] = fma(rn.x, rn.x, acc[2 * h]);
        acc[2 * h + 1] = fma(rn.y, rn.y, acc[2 * h + 1]);
      }
    }
  }
  richm_record<KP>(acc, sred, records);
}

// one workgroup: per running column r.r of the cycle that has just run, its number, the stop test (k_rich_step's);
// the cycle is counted, and `running` cleared when the last column stops
template <int KP>
__global__ __launch_bounds__(WG) void k_richm_step(lsb_mrhs_state *__restrict__ st, const double *__restrict__ parts,
                                                   unsigned nparts) {
  __shared__ double sred[4 * KP];
  const int running = st->running;
  double v[KP];
  wg_sum_partials<KP>(parts, nparts, v, sred);
  if (!running || threadIdx.x != 0)
    return;
  int run = 0;
#pragma unroll
  for (int k = 0; k < KP; k++) {
    lsb_pcg_state *c = &st->c[k];
    if (c->status != LSB_STATUS_RUNNING)
      continue;
    const double rr = v[k], thresh2 = c->thresh2;
    const int it = c->iters + 1;
    c->iters = it, c->rr = rr;
    if (thresh2 > 0.0 && rr <= thresh2)
      c->status = LSB_STATUS_CONVERGED;
    else if (!isfinite(rr))
      c->status = LSB_STATUS_BREAKDOWN;
    else if (it >= c->maxit)
      c->status = LSB_STATUS_MAXIT;
    else
      run = 1;
  }
  st->nspmm += 1;
  st->running = run;
}

// the restart of opts.verify, for the columns the iteration called converged (b_c != 0): r = b - S x (ax = S x) ;
// records of r.r.  Not gated: it runs on a state whose `running` is 0.  Every other column is frozen.
template <int KP>
__global__ __launch_bounds__(WG) void k_richm_restart(unsigned n, const double *__restrict__ b,
                                                      const double *__restrict__ ax, double *r,
                                                      const lsb_mrhs_state *__restrict__ st,
                                                      double *__restrict__ records) {
  __shared__ double sred[4 * KP];
  RICHM_IDX;
  int act[KP];
#pragma unroll
  for (int k = 0; k < KP; k++)
    act[k] = st->c[k].status == LSB_STATUS_CONVERGED && st->c[k].bb > 0.0;
  const d2v *b2 = (const d2v *)b, *a2 = (const d2v *)ax;
  double acc[KP];
#pragma unroll
  for (int k = 0; k < KP; k++)
    acc[k] = 0.0;
  for (size_t i = gtid; i < n2; i += gsz) {
#pragma unroll
    for (int lohi = 0; lohi < 2; lohi++) {
#pragma unroll
      for (int h = 0; h < H; h++) {
        const int a0 = act[2 * h], a1 = act[2 * h + 1];
        if (a0 | a1) {
          const size_t j = (2 * i + lohi) * H + h;
          const d2v bv = b2[j], av = a2[j];
          const d2v rn = {bv.x - av.x, bv.y - av.y};
          store_pairs({r}, {rn}, j, a0, a1);
          acc[2 * h] = fma(rn.x, rn.x, acc[2 * h]);
          acc[2 * h + 1] = fma(rn.y, rn.y, acc[2 * h + 1]);
        }
      }
    }
  }
  if (tail) {
#pragma unroll
    for (int h = 0; h < H; h++) {
      const int a0 = act[2 * h], a1 = act[2 * h + 1];
      if (a0 | a1) {
        const size_t j = (size_t)(n - 1) * H + h;
        const d2v bv = b2[j], av = a2[j];
        const d2v rn = {bv.x - av.x, bv.y - av.y};
        store_pairs({r}, {rn}, j, a0, a1);
        acc[2 * h] = fma(rn.x, rn.x, acc[2 * h]);
        acc[2 * h + 1] = fma(rn.y, rn.y, acc[2 * h + 1]);
      }
    }
  }
  richm_record<KP>(acc, sred, records);
}

// one workgroup: per column that was called converged the recomputed ||b - S x||^2 decides (k_rich_restart_state's
// rule) -- converged (verified), or cycle on from it while the column has restarts left (fewer than max_restarts so
// far), or not converged
template <int KP>
__global__ __launch_bounds__(WG) void k_richm_restart_state(lsb_mrhs_state *__restrict__ st,
                                                            const double *__restrict__ parts, unsigned nparts,
                                                            int max_restarts) {
  __shared__ double sred[4 * KP];
  double v[KP];
  wg_sum_partials<KP>(parts, nparts, v, sred);
  if (threadIdx.x != 0)
    return;
  int run = 0;
#pragma unroll
  for (int k = 0; k < KP; k++) {
    lsb_pcg_state *c = &st->c[k];
    if (!(c->status == LSB_STATUS_CONVERGED && c->bb > 0.0))
      continue;
    const double rr = v[k];
    const int more = st->corrections[k] < max_restarts;
    c->rr = rr;
    st->true_relres[k] = sqrt(rr / c->bb);
    c->status = rr <= c->thresh2                   ? LSB_STATUS_CONVERGED
                : !isfinite(rr)                    ? LSB_STATUS_BREAKDOWN
                : (!more || c->iters >= c->maxit)  ? LSB_STATUS_MAXIT
                                                   : LSB_STATUS_RUNNING;
    if (c->status == LSB_STATUS_RUNNING)
      st->corrections[k] += 1, run = 1;
  }
  st->running = run;
}

// --------------------------------------------------------------------------
// Launchers (hidden, declared in hip_solver.h).  kp: 2, 4 or 8; records: kp doubles per workgroup, *nrecords of them
// (lsb_k_blas1_grid(n) <= LSB_STREAM_GRID_CAP).
// --------------------------------------------------------------------------
extern "C" {

RICHM_HIDDEN void lsb_k_richm_init(unsigned kp, unsigned n, const double *b, double *x, double *r, double *records,
                                   unsigned *nrecords, void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  *nrecords = g;
  KP_DISPATCH(kp, (k_richm_init<KP><<<g, WG, 0, (hipStream_t)stream>>>(n, b, x, r, records)));
}

RICHM_HIDDEN void lsb_k_richm_init_state(unsigned kp, struct lsb_mrhs_state *st, const double *records,
                                         unsigned nrecords, double tol, int maxit, void *stream) {
  KP_DISPATCH(kp, (k_richm_init_state<KP><<<1, WG, 0, (hipStream_t)stream>>>(st, records, nrecords, tol, maxit)));
}

RICHM_HIDDEN void lsb_k_richm_update(unsigned kp, unsigned n, const double *z, const double *q, double *x, double *r,
                                     const struct lsb_mrhs_state *st, double *records, unsigned *nrecords,
                                     void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  *nrecords = g;
  KP_DISPATCH(kp, (k_richm_update<KP><<<g, WG, 0, (hipStream_t)stream>>>(n, z, q, x, r, st, records)));
}

RICHM_HIDDEN void lsb_k_richm_step(unsigned kp, struct lsb_mrhs_state *st, const double *records, unsigned nrecords,
                                   void *stream) {
  KP_DISPATCH(kp, (k_richm_step<KP><<<1, WG, 0, (hipStream_t)stream>>>(st, records, nrecords)));
}

RICHM_HIDDEN void lsb_k_richm_restart(unsigned kp, unsigned n, const double *b, const double *ax, double *r,
                                      const struct lsb_mrhs_state *st, double *records, unsigned *nrecords,
                                      void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  *nrecords = g;
  KP_DISPATCH(kp, (k_richm_restart<KP><<<g, WG, 0, (hipStream_t)stream>>>(n, b, ax, r, st, records)));
}

RICHM_HIDDEN void lsb_k_richm_restart_state(unsigned kp, struct lsb_mrhs_state *st, const double *records,
                                            unsigned nrecords, int max_restarts, void *stream) {
  KP_DISPATCH(kp, (k_richm_restart_state<KP><<<1, WG, 0, (hipStream_t)stream>>>(st, records, nrecords, max_restarts)));
}

} // extern "C"
