// The direct solver (LSB_KRYLOV_DIRECT, --krylov direct): x = P^T W^T W P b with the explicit inverse factor W = L^-1
// of P S P^T = L L^T as a skyline (lsb_direct.c): row k of W is the dense run of columns first[k] .. k at
// vals[woff[k] ..], 8 B per entry, no column indices and no transposed copy.
//
// The factor may be cut into tiers (one tier: the single skyline); the products are hip_direct_t.hip's.  This file
// holds what every round shares, whatever the number of tiers:
//
//   state                                          k_dir_init_state (one thread)
//   round k:  x (+)= P^T L^-T L^-1 P r             the products: hip_direct_t.hip (r = b and x stored in round 1)
//             r = b - S x ; records of r.r, b.b    k_dir_resid   (tol = 0: not in the last round)
//             iters = k ; the stop test            k_dir_step    (one workgroup)
//
// Rules, as for the other iterations (hip_rich.hip):
//   * both products sum in a fixed order, no atomics: the same bits run after run, from graphs or plain launches;
//   * every launch of a round returns at once when the status has left RUNNING, and the status is written by
//     k_dir_step alone, a launch of one workgroup between the residual and the next round's first launch;
//   * which round it is comes from the state too (iters), so a captured graph of rounds is the same graph whichever
//     round it starts at.
#include "hip_kcommon.h"

#define DIR_HIDDEN __attribute__((visibility("hidden")))

// not gated: the state still holds the previous solve's status.  alpha[0] keeps tol for k_dir_step (b.b is known
// only after the first residual)
__global__ void k_dir_init_state(lsb_pcg_state *__restrict__ st, double tol, int maxit) {
  if (threadIdx.x != 0 || blockIdx.x != 0)
    return;
  st->rz[0] = st->rz[1] = st->pq = st->alpha[1] = 0.0; // (the PCG forms' words: not used)
  st->alpha[0] = tol;
  st->bb = st->thresh2 = st->rr = 0.0;
  st->iters = 0, st->maxit = maxit;
  st->pad = st->xpend = 0;
  st->status = maxit <= 0 ? LSB_STATUS_MAXIT : LSB_STATUS_RUNNING;
}

// r = b - S x off the plain CSR, L lanes per row by the row kernels' rule; one record (r.r, b.b) per workgroup.
// tol = 0 (alpha[0]): the last round has nobody to read it and returns
template <int L>
__global__ __launch_bounds__(WG) void k_dir_resid(unsigned n, const int *__restrict__ offs,
                                                  const int *__restrict__ cols, const double *__restrict__ vals,
                                                  const double *__restrict__ b, const double *__restrict__ x,
                                                  double *__restrict__ r, double *__restrict__ records,
                                                  const lsb_pcg_state *__restrict__ st) {
  __shared__ double sred[8];
  if (st->status || (st->alpha[0] == 0.0 && st->iters + 1 >= st->maxit))
    return;
  constexpr unsigned RPW = WG / L;
  const unsigned sub = threadIdx.x / L, l = threadIdx.x % L;
  double acc[2] = {0.0, 0.0};
  for (unsigned base = blockIdx.x * RPW; base < n; base += gridDim.x * RPW) {
    const unsigned row = base + sub;
    double s = 0.0;
    if (row < n)
      for (int e = offs[row] + (int)l; e < offs[row + 1]; e += L)
        s = fma(vals[e], x[cols[e]], s);
#pragma unroll
    for (int m = L / 2; m >= 1; m >>= 1)
      s += __shfl_xor(s, m, 64);
    if (row < n && l == 0) {
      const double bv = b[row], rv = bv - s;
      r[row] = rv;
      acc[0] = fma(rv, rv, acc[0]), acc[1] = fma(bv, bv, acc[1]);
    }
  }
  wg_sum<2>(acc, sred);
  if (threadIdx.x == 0)
    records[2 * blockIdx.x] = acc[0], records[2 * blockIdx.x + 1] = acc[1];
}

// one workgroup: the round that has just run is counted, and -- tol > 0 -- the recomputed r.r decides.  tol = 0: the
// run is exactly maxit rounds and the records are not read (the last round leaves none)
__global__ __launch_bounds__(WG) void k_dir_step(lsb_pcg_state *__restrict__ st, const double *__restrict__ records,
                                                 unsigned nrecords) {
  __shared__ double sred[8];
  const int stopped = st->status;
  const double tol = st->alpha[0];
  double v[2];
  wg_sum_partials<2>(records, tol > 0.0 ? nrecords : 0u, v, sred);
  if (stopped || threadIdx.x != 0)
    return;
  const int it = st->iters + 1;
  st->iters = it;
  if (!(tol > 0.0)) {
    if (it >= st->maxit)
      st->status = LSB_STATUS_MAXIT;
    return;
  }
  const double rr = v[0], bb = v[1], thresh2 = tol * tol * bb;
  st->rr = rr, st->bb = bb, st->thresh2 = thresh2;
  if (rr <= thresh2) // (b = 0: x = 0 is the solution)
    st->status = LSB_STATUS_CONVERGED;
  else if (!isfinite(rr))
    st->status = LSB_STATUS_BREAKDOWN;
  else if (it >= st->maxit)
    st->status = LSB_STATUS_MAXIT;
}

extern "C" {

DIR_HIDDEN void lsb_k_dir_init_state(struct lsb_pcg_state *st, double tol, int maxit, void *stream) {
  k_dir_init_state<<<1, 64, 0, (hipStream_t)stream>>>(st, tol, maxit);
}

DIR_HIDDEN void lsb_k_dir_resid(unsigned n, const int *offs, const int *cols, const double *vals, unsigned lanes,
                                const double *b, const double *x, double *r, double *records, unsigned *nrecords,
                                const struct lsb_pcg_state *st, void *stream) {
  const unsigned Lr = row_lanes(lanes);
  unsigned g = div_up(n, WG / Lr);
  if (g > LSB_MAX_PARTIALS)
    g = LSB_MAX_PARTIALS;
  *nrecords = g;
  LANES_DISPATCH(lanes, (k_dir_resid<L><<<g, WG, 0, (hipStream_t)stream>>>(n, offs, cols, vals, b, x, r, records, st)));
}

DIR_HIDDEN void lsb_k_dir_step(struct lsb_pcg_state *st, const double *records, unsigned nrecords, void *stream) {
  k_dir_step<<<1, WG, 0, (hipStream_t)stream>>>(st, records, nrecords);
}

} // extern "C"
