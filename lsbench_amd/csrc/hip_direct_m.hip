// The direct solver on blocks of right-hand sides (lsb_hip_solver_solve_direct_multi[_dev] and its companions; the
// host side: hip_direct_m_drv.c): the rounds of hip_direct.hip on KP = 2, 4 or 8 columns at once.  This file holds what
// every round of a block shares, whatever the number of tiers; the products are hip_direct_tm.hip's.
//
//   state                                           k_dir_init_state_m (one thread)
//   round k:  X (+)= P^T L^-T L^-1 P V               the products: hip_direct_tm.hip (V = B, X stored in round 1)
//             R = B - S X ; records of r.r, b.b      k_dir_resid_m<L, KP>   (tol = 0: not in the last round)
//             iters = k ; the stop test per column   k_dir_step_m<KP>       (one workgroup)
//
// The rule of every block here: a column of a block has the bits of the same column solved alone.  So each kernel
// keeps the summation order of the single-column kernel per column -- the same lanes per row, the same fma chain, the
// same butterfly, the same order of the partial sums -- and only shares what has no rounding: the loads of the
// factor, of first / woff, of the CSR.  That rules out MFMA (v_mfma_f64_* sums in an order of its own); at <= 8
// columns the products are nowhere near the fp64 vector rate anyway.
//
// Block vectors are interleaved as in hip_mrhs.hip: element (i, c) at i KP + c, read and written as 16-byte pairs, in
// the caller's numbering (perm is applied inside the kernels, as by the single-column ones).  The state is a
// lsb_mrhs_state whose c[c] is used as the direct solver uses lsb_pcg_state (alpha[0] = tol, iters, status, rr, bb,
// thresh2); `running` is the gate of every launch of a round, cleared by k_dir_step_m when the last column stops.  A
// column whose status has left RUNNING is frozen: its x and r are no longer written, its iters and rr stay.  All
// running columns have run the same number of rounds, so which round it is comes from any of them (dirm_round), and
// a captured graph of rounds is the same graph wherever it starts.  st == NULL (one application on its own): not
// gated, V = B, X stored, every column written.
#include "hip_mrhs_k.h"

#define DIR_HIDDEN __attribute__((visibility("hidden")))

// not gated: the state still holds the previous block's.  Columns >= kp are no columns: never running
__global__ void k_dir_init_state_m(lsb_mrhs_state *__restrict__ st, unsigned kp, double tol, int maxit) {
  if (threadIdx.x != 0 || blockIdx.x != 0)
    return;
  for (unsigned c = 0; c < LSB_MRHS_MAX; c++) {
    lsb_pcg_state *s = &st->c[c];
    s->rz[0] = s->rz[1] = s->pq = s->alpha[1] = 0.0; // (the PCG forms' words: not used)
    s->alpha[0] = tol;
    s->bb = s->thresh2 = s->rr = 0.0;
    s->iters = 0, s->maxit = maxit;
    s->pad = s->xpend = 0;
    s->status = c >= kp || maxit <= 0 ? LSB_STATUS_MAXIT : LSB_STATUS_RUNNING;
    st->true_relres[c] = -1.0, st->start_relres[c] = 0.0;
    st->corrections[c] = 0;
  }
  st->tol = tol;
  st->running = maxit > 0;
  st->nspmm = 0; // rounds that did work: what the host's hint is taken from
}

// R = B - S X off the plain CSR by k_dir_resid's rule: L lanes per row (the row rule of the blocks is that kernel's:
// entries l, l + L, ... with fma in storage order, the xor butterfly L / 2 .. 1), the same grid and the same strided
// row assignment, one record per workgroup: (r.r, b.b) of column c at 2 c, 2 c + 1, each with the bits of the single
// solve's.  r of a frozen column is not written.  tol = 0: the last round has nobody to read it and returns
template <int L, int KP>
__global__ __launch_bounds__(WG) void k_dir_resid_m(unsigned n, const int *__restrict__ offs,
                                                    const int *__restrict__ cols, const double *__restrict__ vals,
                                                    const double *__restrict__ b, const double *__restrict__ x,
                                                    double *__restrict__ r, double *__restrict__ records,
                                                    const lsb_mrhs_state *__restrict__ st) {
  constexpr int H = KP / 2;
  __shared__ double sred[4 * 2 * KP];
  if (!st->running || (st->tol == 0.0 && dirm_round<KP>(st) + 1 >= st->c[0].maxit))
    return;
  constexpr unsigned RPW = WG / L;
  const unsigned sub = threadIdx.x / L, l = threadIdx.x % L;
  double acc[2 * KP];
#pragma unroll
  for (int c = 0; c < 2 * KP; c++)
    acc[c] = 0.0;
  for (unsigned base = blockIdx.x * RPW; base < n; base += gridDim.x * RPW) {
    const unsigned row = base + sub;
    double s[KP];
    block_row_product<L, KP>(offs, cols, vals, x, row, row < n, l, s);
    if (row < n && l == 0) {
#pragma unroll
      for (int h = 0; h < H; h++) {
        const d2v bv = ((const d2v *)b)[(size_t)row * H + h];
        const d2v rv = d2v{bv.x - s[2 * h], bv.y - s[2 * h + 1]};
        const int a0 = st->c[2 * h].status == LSB_STATUS_RUNNING, a1 = st->c[2 * h + 1].status == LSB_STATUS_RUNNING;
        if (a0 | a1) {
          double *const rs[1] = {r};
          const d2v val[1] = {rv};
          store_pairs<1>(rs, val, (size_t)row * H + h, a0, a1);
        }
        acc[4 * h] = fma(rv.x, rv.x, acc[4 * h]), acc[4 * h + 1] = fma(bv.x, bv.x, acc[4 * h + 1]);
        acc[4 * h + 2] = fma(rv.y, rv.y, acc[4 * h + 2]), acc[4 * h + 3] = fma(bv.y, bv.y, acc[4 * h + 3]);
      }
    }
  }
  wg_sum<2 * KP>(acc, sred);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int h = 0; h < KP; h++)
      ((d2v *)records)[(size_t)blockIdx.x * KP + h] = d2v{acc[2 * h], acc[2 * h + 1]};
  }
}

// one workgroup: k_dir_step's decisions for every running column -- the round that has just run is counted, and,
// tol > 0, the recomputed r.r decides (tol = 0: exactly maxit rounds, the records are not read) -- and `running`
// cleared when the last column has stopped
template <int KP>
__global__ __launch_bounds__(WG) void k_dir_step_m(lsb_mrhs_state *__restrict__ st,
                                                   const double *__restrict__ records, unsigned nrecords) {
  __shared__ double sred[4 * 2 * KP];
  const int running = st->running;
  const double tol = st->tol;
  double v[2 * KP];
  wg_sum_partials<2 * KP>(records, tol > 0.0 ? nrecords : 0u, v, sred);
  if (!running || threadIdx.x != 0)
    return;
  int any = 0;
#pragma unroll
  for (int c = 0; c < KP; c++) {
    lsb_pcg_state *s = &st->c[c];
    if (s->status != LSB_STATUS_RUNNING)
      continue;
    const int it = s->iters + 1;
    int status = LSB_STATUS_RUNNING;
    s->iters = it;
    if (!(tol > 0.0)) {
      if (it >= s->maxit)
        status = LSB_STATUS_MAXIT;
    } else {
      const double rr = v[2 * c], bb = v[2 * c + 1], thresh2 = tol * tol * bb;
      s->rr = rr, s->bb = bb, s->thresh2 = thresh2;
      if (rr <= thresh2) // (b = 0: x = 0 is the solution)
        status = LSB_STATUS_CONVERGED;
      else if (!isfinite(rr))
        status = LSB_STATUS_BREAKDOWN;
      else if (it >= s->maxit)
        status = LSB_STATUS_MAXIT;
    }
    s->status = status;
    any |= status == LSB_STATUS_RUNNING;
  }
  st->nspmm += 1;
  st->running = any;
}

template <int KP>
static void resid_m_launch(unsigned g, unsigned n, const int *offs, const int *cols, const double *vals, unsigned lanes,
                           const double *b, const double *x, double *r, double *records,
                           const struct lsb_mrhs_state *st, hipStream_t s) {
  LANES_DISPATCH(lanes, (k_dir_resid_m<L, KP><<<g, WG, 0, s>>>(n, offs, cols, vals, b, x, r, records, st)));
}

extern "C" {

DIR_HIDDEN void lsb_k_dir_init_state_m(struct lsb_mrhs_state *st, unsigned kp, double tol, int maxit, void *stream) {
  k_dir_init_state_m<<<1, 64, 0, (hipStream_t)stream>>>(st, kp, tol, maxit);
}

DIR_HIDDEN void lsb_k_dir_resid_m(unsigned kp, unsigned n, const int *offs, const int *cols, const double *vals,
                                  unsigned lanes, const double *b, const double *x, double *r, double *records,
                                  unsigned *nrecords, const struct lsb_mrhs_state *st, void *stream) {
  const unsigned Lr = row_lanes(lanes);
  unsigned g = div_up(n, WG / Lr);
  if (g > LSB_MAX_PARTIALS)
    g = LSB_MAX_PARTIALS;
  *nrecords = g;
  KP_DISPATCH(kp, (resid_m_launch<KP>(g, n, offs, cols, vals, lanes, b, x, r, records, st, (hipStream_t)stream)));
}

DIR_HIDDEN void lsb_k_dir_step_m(unsigned kp, struct lsb_mrhs_state *st, const double *records, unsigned nrecords,
                                 void *stream) {
  KP_DISPATCH(kp, (k_dir_step_m<KP><<<1, WG, 0, (hipStream_t)stream>>>(st, records, nrecords)));
}

} // extern "C"
