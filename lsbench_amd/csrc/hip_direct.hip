// The direct solver (LSB_KRYLOV_DIRECT, --krylov direct): x = P^T W^T W P b with the explicit inverse factor W = L^-1
// of P S P^T = L L^T as a skyline (lsb_direct.c): row k of W is the dense run of columns first[k] .. k at
// vals[woff[k] ..], 8 B per entry, no column indices and no transposed copy.
//
//   state                                          k_dir_init_state (one thread)
//   round k:  t = W (P r)      r = b in round 1    k_dir_rows
//             x (+)= P^T W^T t  stored in round 1   k_dir_cols
//             r = b - S x ; records of r.r, b.b    k_dir_resid   (tol = 0: not in the last round)
//             iters = k ; the stop test            k_dir_step    (one workgroup)
//
// Rules, as for the other iterations (hip_rich.hip):
//   * both products sum in a fixed order, no atomics: the same bits run after run, from graphs or plain launches;
//   * every launch of a round returns at once when the status has left RUNNING, and the status is written by
//     k_dir_step alone, a launch of one workgroup between the residual and the next round's first launch;
//   * which round it is comes from the state too (iters), so a captured graph of rounds is the same graph whichever
//     round it starts at.
//
// k_dir_rows.  The host deals the rows into groups -- consecutive rows that take the same number of lanes L, 64 / L
// of them: one wavefront's work -- and the groups into workgroups of about equal entry count.  The column runs of
// consecutive rows nest or abut (postorder), so a workgroup reads one contiguous window of P r; it stages the window
// in LDS once where it fits the launch's LDS (cap doubles), else it gathers from global memory -- the same numbers
// either way.  Lane rule, a function of the row's length alone, so the bits do not depend on the dealing: L lanes per
// row, lane l takes entries l, l + L, ... with fma in ascending order, the lanes are folded by the xor butterfly.
//
// k_dir_cols.  A workgroup owns 64 consecutive columns [j0, j1], one lane per column in each of its sixteen wavefronts,
// and visits the rows that reach them: first the rows j0 .. j1, then the ancestors of j1 beyond it, run by run from
// run_end / parent (every ancestor of a window column above j1 is an ancestor of j1).  Lane j takes part in row k
// where first[k] <= j <= k; a row is one coalesced run of the window's width.  The visited rows are dealt round-robin
// to the sixteen wavefronts in visiting order; each adds its own in ascending k and the sixteen sums are added in
// ascending order.  Nobody walks parent[] vertex by vertex: the largest subtree is numbered last (lsb_direct.c), so a
// walk to the root is a handful of runs.
#include "hip_kcommon.h"

#define DIR_HIDDEN __attribute__((visibility("hidden")))
#define DIR_COLS 64 // columns per workgroup of k_dir_cols: one wavefront's width
#define DIR_FLIGHT 8
#define DIR_CWG 1024 // ... and its threads: sixteen wavefronts share the rows that reach the window

typedef unsigned long long dir_u64;

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

// src: 0 = by the state (b in round 1, r afterwards), 1 = b whatever the state says (one application on its own)
__global__ __launch_bounds__(WG) void k_dir_rows(const double *__restrict__ vals, const dir_u64 *__restrict__ woff,
                                                 const unsigned *__restrict__ first,
                                                 const unsigned *__restrict__ perm, const unsigned *__restrict__ grp,
                                                 const unsigned *__restrict__ blk, const unsigned *__restrict__ bwin,
                                                 unsigned cap, const double *__restrict__ b,
                                                 const double *__restrict__ r, double *__restrict__ t,
                                                 const lsb_pcg_state *__restrict__ st, int src) {
  extern __shared__ double win[];
  if (st->status)
    return;
  const double *__restrict__ v = src || st->iters == 0 ? b : r;
  const unsigned g0 = blk[blockIdx.x], g1 = blk[blockIdx.x + 1];
  const unsigned wlo = bwin[2 * blockIdx.x], ww = bwin[2 * blockIdx.x + 1];
  const bool staged = ww <= cap;
  if (staged) {
    for (unsigned i = threadIdx.x; i < ww; i += WG)
      win[i] = v[perm[wlo + i]];
    __syncthreads();
  }
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (unsigned g = g0 + wave; g < g1; g += WG / 64) {
    const unsigned row0 = grp[2 * g], meta = grp[2 * g + 1];
    const unsigned L = meta & 0xffu, nr = meta >> 8; // L: a power of two, 1 .. 64; nr <= 64 / L rows
    const unsigned sub = lane / L, l = lane & (L - 1);
    const bool mine = sub < nr;
    double acc = 0.0;
    if (mine) {
      const unsigned k = row0 + sub, f = first[k], len = k - f + 1;
      const double *__restrict__ w = vals + woff[k];
      if (staged) {
        const double *__restrict__ a = win + (f - wlo);
#pragma unroll 4
        for (unsigned e = l; e < len; e += L)
          acc = fma(w[e], a[e], acc);
      } else {
        for (unsigned e = l; e < len; e += L)
          acc = fma(w[e], v[perm[f + e]], acc);
      }
    }
    for (unsigned m = 32; m >= 1; m >>= 1)
      if (m < L) // (the same L in the whole wavefront)
        acc += __shfl_xor(acc, m, 64);
    if (mine && l == 0)
      t[row0 + sub] = acc;
  }
}

// mode: 0 = by the state (round 1 stores x, the others add to it), 1 = store whatever the state says
__global__ __launch_bounds__(DIR_CWG) void k_dir_cols(unsigned n, const double *__restrict__ vals,
                                                      const dir_u64 *__restrict__ woff,
                                                      const unsigned *__restrict__ first,
                                                      const unsigned *__restrict__ perm,
                                                      const unsigned *__restrict__ parent,
                                                      const unsigned *__restrict__ run_end,
                                                      const double *__restrict__ t, double *__restrict__ x,
                                                      const lsb_pcg_state *__restrict__ st, int mode) {
  constexpr unsigned NW = DIR_CWG / 64;
  __shared__ double part[NW][DIR_COLS];
  if (st->status)
    return;
  const bool add = !mode && st->iters > 0;
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned j0 = blockIdx.x * DIR_COLS, j1 = (j0 + DIR_COLS < n ? j0 + DIR_COLS : n) - 1;
  const unsigned j = j0 + lane;
  const bool active = j <= j1;
  double acc = 0.0;
  // this wavefront's rows k0, k0 + NW, ... <= kend, 64 at a time: lane m fetches what row m of the batch needs (its
  // first column, its offset, t_k), then every lane walks the batch with those broadcast -- the loads of W are
  // independent of one another and go out several at a time
  auto visit = [&](unsigned k0, unsigned kend) {
    for (unsigned kb = k0; kb <= kend; kb += 64 * NW) {
      const unsigned km = kb + lane * NW;
      unsigned fm = 0;
      dir_u64 om = 0;
      double tm = 0.0;
      if (km <= kend)
        fm = first[km], om = woff[km], tm = t[km];
      const unsigned left = (kend - kb) / NW + 1, cnt = left < 64 ? left : 64;
      for (unsigned m0 = 0; m0 < cnt; m0 += DIR_FLIGHT) { // DIR_FLIGHT rows' loads in flight together
        double w[DIR_FLIGHT], tk[DIR_FLIGHT];
#pragma unroll
        for (unsigned u = 0; u < DIR_FLIGHT; u++) {
          const unsigned m = m0 + u < cnt ? m0 + u : cnt - 1; // (past the batch: its last row again, not added)
          const unsigned f = __shfl(fm, m, 64), k = kb + m * NW;
          const dir_u64 o = __shfl(om, m, 64);
          tk[u] = __shfl(tm, m, 64);
          const bool in = active && j >= f && j <= k && m0 + u < cnt;
          w[u] = in ? vals[o + (j - f)] : 0.0;
          tk[u] = in ? tk[u] : 0.0;
        }
#pragma unroll
        for (unsigned u = 0; u < DIR_FLIGHT; u++)
          acc = fma(tk[u], w[u], acc);
      }
    }
  };
  visit(j0 + wave, j1); // the window's own rows
  unsigned pos = j1 - j0 + 1; // rows visited so far
  for (unsigned p = parent[j1]; p < n;) { // the ancestors of j1, run by run
    const unsigned re = run_end[p];
    visit(p + ((wave + NW - (pos & (NW - 1))) & (NW - 1)), re);
    pos += re - p + 1;
    p = parent[re];
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && active) {
    double z = part[0][lane];
#pragma unroll
    for (unsigned w = 1; w < NW; w++)
      z += part[w][lane];
    const unsigned i = perm[j];
    x[i] = add ? x[i] + z : z;
  }
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

DIR_HIDDEN void lsb_k_dir_rows(const struct lsb_dir_dev *d, const double *b, const double *r, double *t,
                               const struct lsb_pcg_state *st, int src, void *stream) {
  if (!d->nblk)
    return;
  k_dir_rows<<<d->nblk, WG, (size_t)d->lds_doubles * sizeof(double), (hipStream_t)stream>>>(
      d->vals, d->woff, d->first, d->perm, d->grp, d->blk, d->bwin, d->lds_doubles, b, r, t, st, src);
}

DIR_HIDDEN void lsb_k_dir_cols(const struct lsb_dir_dev *d, const double *t, double *x, const struct lsb_pcg_state *st,
                               int mode, void *stream) {
  if (!d->n)
    return;
  k_dir_cols<<<div_up(d->n, DIR_COLS), DIR_CWG, 0, (hipStream_t)stream>>>(d->n, d->vals, d->woff, d->first, d->perm,
                                                                    d->parent, d->run_end, t, x, st, mode);
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
