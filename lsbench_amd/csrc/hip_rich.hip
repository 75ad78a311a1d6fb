// AMG as the solver (LSB_KRYLOV_RICHARDSON, --krylov richardson): stationary V-cycle iterations -- preconditioned
// Richardson with unit step in residual-correction form, the way the AMG backends of the reference run theirs
// (a fixed number of cycles, no tolerance: src/hypre.c:185-186, src/amgx.c:78-85).
//
//   x = 0 ; r = b ; bb = b.b                        k_rich_init, k_rich_init_state
//   cycle k:  z = M^-1 r                            one V-cycle (hip_amg.hip / hip_amg_f32.hip), into the gather vector
//             q = S z                               the shard's SpMV
//             x += z ; r -= q ; partials of r.r     k_rich_update
//             rr ; iters = k ; the stop test        k_rich_step (one workgroup)
//
// x and r are fp64 and live outside the cycle: around the fp32 cycle this is an iterative refinement.  Both
// updates are single IEEE operations, so a caller who replays z = M^-1 r, q = S z, x + z, r - q through the
// public entry points gets the same bits.
//
// The rules of the other sweeps (hip_sweeps.hip, hip_bicgstab.hip):
//   * r.r is one partial per workgroup, summed again in fixed order by the one workgroup of k_rich_step: no
//     atomics, the same bits run after run;
//   * every launch of a cycle returns at once when the status has left RUNNING, and the status is written by
//     k_rich_step alone -- a launch of one workgroup, between the update that forms r.r and the next cycle's
//     first launch: nothing is set and tested by different workgroups of one launch.  So x is updated only
//     while the state is RUNNING; after CONVERGED at cycle k it holds x_k;
//   * 16-byte loads and stores where every operand is 16-byte aligned.  The caller's x and b may be only
//     8-byte aligned: the other instantiation walks the same pairs in the same order through plain doubles
//     (no 16-byte type is ever laid over an 8-byte aligned address), so its r.r has the same bits too.
#include "hip_kcommon.h"

#define RICH_HIDDEN __attribute__((visibility("hidden")))

typedef double r2v __attribute__((ext_vector_type(2)));

// the pair (2 i, 2 i + 1) of a vector; NT: nobody reads it again before it is overwritten (hip_sweeps.hip, ld2)
template <bool V2, bool NT>
__device__ __forceinline__ r2v ldp(const double *__restrict__ p, size_t i) {
  if (V2)
    return NT ? __builtin_nontemporal_load((const r2v *)p + i) : ((const r2v *)p)[i];
  if (NT)
    return r2v{__builtin_nontemporal_load(p + 2 * i), __builtin_nontemporal_load(p + 2 * i + 1)};
  return r2v{p[2 * i], p[2 * i + 1]};
}
template <bool V2, bool NT>
__device__ __forceinline__ void stp(double *__restrict__ p, size_t i, r2v v) {
  if (V2) {
    if (NT)
      __builtin_nontemporal_store(v, (r2v *)p + i);
    else
      ((r2v *)p)[i] = v;
  } else if (NT) {
    __builtin_nontemporal_store(v.x, p + 2 * i);
    __builtin_nontemporal_store(v.y, p + 2 * i + 1);
  } else
    p[2 * i] = v.x, p[2 * i + 1] = v.y;
}

#define RICH_IDX                                                    \
  const size_t gtid = (size_t)blockIdx.x * WG + threadIdx.x;        \
  const size_t gsz = (size_t)gridDim.x * WG;                        \
  const size_t n2 = n / 2;                                          \
  const bool tail = (n & 1) && gtid == gsz - 1 /* the odd last element: the last thread's */

// x = 0 ; r = b ; partials of b.b
template <bool V2>
__global__ __launch_bounds__(WG) void k_rich_init(unsigned n, const double *__restrict__ b, double *__restrict__ x,
                                                  double *__restrict__ r, double *__restrict__ partials) {
  __shared__ double sred[4];
  RICH_IDX;
  double acc[1] = {0.0};
  for (size_t i = gtid; i < n2; i += gsz) {
    const r2v bv = ldp<V2, true>(b, i);
    stp<V2, false>(x, i, r2v{0.0, 0.0});
    stp<V2, false>(r, i, bv);
    acc[0] = fma(bv.y, bv.y, fma(bv.x, bv.x, acc[0]));
  }
  if (tail) {
    const double bv = b[n - 1];
    x[n - 1] = 0.0, r[n - 1] = bv;
    acc[0] = fma(bv, bv, acc[0]);
  }
  wg_sum<1>(acc, sred);
  if (threadIdx.x == 0)
    partials[blockIdx.x] = acc[0];
}

// one workgroup: b.b starts the state (not gated: the state still holds the previous solve's status)
__global__ __launch_bounds__(WG) void k_rich_init_state(lsb_pcg_state *__restrict__ st,
                                                        const double *__restrict__ parts, unsigned nparts, double tol,
                                                        int maxit) {
  __shared__ double sred[4];
  double v[1];
  wg_sum_partials<1>(parts, nparts, v, sred);
  if (threadIdx.x != 0)
    return;
  const double bb = v[0];
  st->rz[0] = st->rz[1] = st->pq = st->alpha[0] = st->alpha[1] = 0.0; // (the PCG forms' words: not used)
  st->bb = bb, st->thresh2 = tol * tol * bb, st->rr = bb;
  st->iters = 0, st->maxit = maxit;
  st->pad = st->xpend = 0;
  // b == 0 => x = 0 is the solution; maxit == 0 => nothing to do (as k_pcg_init_state)
  st->status = bb == 0.0 ? LSB_STATUS_CONVERGED : (maxit <= 0 ? LSB_STATUS_MAXIT : LSB_STATUS_RUNNING);
}

// x += z ; r -= q ; partials of r.r
template <bool V2>
__global__ __launch_bounds__(WG) void k_rich_update(unsigned n, const double *__restrict__ z,
                                                    const double *__restrict__ q, double *__restrict__ x,
                                                    double *__restrict__ r, const lsb_pcg_state *__restrict__ st,
                                                    double *__restrict__ partials) {
  __shared__ double sred[4];
  RICH_IDX;
  if (st->status)
    return;
  double acc[1] = {0.0};
  for (size_t i = gtid; i < n2; i += gsz) {
    const r2v xv = ldp<V2, true>(x, i), zv = ldp<V2, true>(z, i);
    const r2v rv = ldp<V2, false>(r, i), qv = ldp<V2, true>(q, i);
    const r2v xn = {xv.x + zv.x, xv.y + zv.y}, rn = {rv.x - qv.x, rv.y - qv.y};
    stp<V2, true>(x, i, xn); // nobody reads x before the next cycle's update
    stp<V2, false>(r, i, rn); // the cycle's first launch reads it next: the plain way
    acc[0] = fma(rn.y, rn.y, fma(rn.x, rn.x, acc[0]));
  }
  if (tail) {
    const size_t i = n - 1;
    const double rn = r[i] - q[i];
    x[i] = x[i] + z[i], r[i] = rn;
    acc[0] = fma(rn, rn, acc[0]);
  }
  wg_sum<1>(acc, sred);
  if (threadIdx.x == 0)
    partials[blockIdx.x] = acc[0];
}

// one workgroup: r.r of the cycle that has just run, its number, the stop test.  tol = 0 (thresh2 = 0) never
// converges: the run is then exactly maxit cycles.
__global__ __launch_bounds__(WG) void k_rich_step(lsb_pcg_state *__restrict__ st, const double *__restrict__ parts,
                                                  unsigned nparts) {
  __shared__ double sred[4];
  const int stopped = st->status;
  double v[1];
  wg_sum_partials<1>(parts, nparts, v, sred);
  if (stopped || threadIdx.x != 0)
    return;
  const double rr = v[0], thresh2 = st->thresh2;
  const int it = st->iters + 1;
  st->iters = it, st->rr = rr;
  if (thresh2 > 0.0 && rr <= thresh2)
    st->status = LSB_STATUS_CONVERGED;
  else if (!isfinite(rr))
    st->status = LSB_STATUS_BREAKDOWN;
  else if (it >= st->maxit)
    st->status = LSB_STATUS_MAXIT;
}

// the restart of opts.verify: r = b - S x (ax = S x) ; partials of r.r.  Not gated: it runs on a state that says
// CONVERGED.
template <bool V2>
__global__ __launch_bounds__(WG) void k_rich_restart(unsigned n, const double *__restrict__ b,
                                                     const double *__restrict__ ax, double *__restrict__ r,
                                                     double *__restrict__ partials) {
  __shared__ double sred[4];
  RICH_IDX;
  double acc[1] = {0.0};
  for (size_t i = gtid; i < n2; i += gsz) {
    const r2v bv = ldp<V2, true>(b, i), av = ldp<V2, true>(ax, i);
    const r2v rn = {bv.x - av.x, bv.y - av.y};
    stp<V2, false>(r, i, rn);
    acc[0] = fma(rn.y, rn.y, fma(rn.x, rn.x, acc[0]));
  }
  if (tail) {
    const double rn = b[n - 1] - ax[n - 1];
    r[n - 1] = rn;
    acc[0] = fma(rn, rn, acc[0]);
  }
  wg_sum<1>(acc, sred);
  if (threadIdx.x == 0)
    partials[blockIdx.x] = acc[0];
}

// one workgroup: the recomputed ||b - S x||^2 decides -- converged (verified), or cycle on from it (more != 0:
// another restart is allowed), or not converged
__global__ __launch_bounds__(WG) void k_rich_restart_state(lsb_pcg_state *__restrict__ st,
                                                           const double *__restrict__ parts, unsigned nparts,
                                                           int more) {
  __shared__ double sred[4];
  double v[1];
  wg_sum_partials<1>(parts, nparts, v, sred);
  if (threadIdx.x != 0)
    return;
  const double rr = v[0];
  st->rr = rr;
  st->status = rr <= st->thresh2                   ? LSB_STATUS_CONVERGED
               : !isfinite(rr)                     ? LSB_STATUS_BREAKDOWN
               : (!more || st->iters >= st->maxit) ? LSB_STATUS_MAXIT
                                                   : LSB_STATUS_RUNNING;
}

extern "C" {

RICH_HIDDEN void lsb_k_rich_init(unsigned n, const double *b, double *x, double *r, double *partials,
                                 unsigned *npartials, void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  *npartials = g;
  const auto kern = aligned16(b) && aligned16(x) && aligned16(r) ? k_rich_init<true> : k_rich_init<false>;
  kern<<<g, WG, 0, (hipStream_t)stream>>>(n, b, x, r, partials);
}

RICH_HIDDEN void lsb_k_rich_init_state(struct lsb_pcg_state *st, const double *parts, unsigned nparts, double tol,
                                       int maxit, void *stream) {
  k_rich_init_state<<<1, WG, 0, (hipStream_t)stream>>>(st, parts, nparts, tol, maxit);
}

RICH_HIDDEN void lsb_k_rich_update(unsigned n, const double *z, const double *q, double *x, double *r,
                                   const struct lsb_pcg_state *st, double *partials, unsigned *npartials,
                                   void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  *npartials = g;
  const bool v2 = aligned16(z) && aligned16(q) && aligned16(x) && aligned16(r);
  const auto kern = v2 ? k_rich_update<true> : k_rich_update<false>;
  kern<<<g, WG, 0, (hipStream_t)stream>>>(n, z, q, x, r, st, partials);
}

RICH_HIDDEN void lsb_k_rich_step(struct lsb_pcg_state *st, const double *parts, unsigned nparts, void *stream) {
  k_rich_step<<<1, WG, 0, (hipStream_t)stream>>>(st, parts, nparts);
}

RICH_HIDDEN void lsb_k_rich_restart(unsigned n, const double *b, const double *ax, double *r, double *partials,
                                    unsigned *npartials, void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  *npartials = g;
  const auto kern = aligned16(b) && aligned16(ax) && aligned16(r) ? k_rich_restart<true> : k_rich_restart<false>;
  kern<<<g, WG, 0, (hipStream_t)stream>>>(n, b, ax, r, partials);
}

RICH_HIDDEN void lsb_k_rich_restart_state(struct lsb_pcg_state *st, const double *parts, unsigned nparts, int more,
                                          void *stream) {
  k_rich_restart_state<<<1, WG, 0, (hipStream_t)stream>>>(st, parts, nparts, more);
}

} // extern "C"
