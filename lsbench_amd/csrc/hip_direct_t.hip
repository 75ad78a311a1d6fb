// The direct solver's products x (+)= P^T L^-T L^-1 P r on the inverse factor in m tiers (the factor: lsb_direct.c,
// struct lsb_tierinv; the driver: hip_direct_drv.c).  The rows are numbered tier by tier, L is block lower triangular,
// and only the diagonal blocks are inverted: W_tt = (L_tt)^-1 are skylines -- row k is the dense run of columns
// first[k] .. k at vals[woff[k] ..], 8 B per entry, no column indices and no transposed copy --, the blocks below the
// diagonal are the sparse rows of L, by rows (C) and by columns (C^T).  One tier (lsb_hip_solver_create, tiers = 1) is
// the single skyline W = L^-1: no coupling, x = P^T W^T (W (P r)), k_dirt_rows<true> and k_dirt_cols and nothing else,
// z == NULL and not stored.  Two work vectors in the tier-major numbering otherwise: y (the forward result, then the
// backward operand u, in place) and z.
//
//   round k:  y_0 = W_00 (P r)_0                      k_dirt_rows<true>   r = b in round 1, read through perm
//             t = 1 .. m - 1:
//               z_t = (P r)_t - C_t y_<t              k_dirt_fwd
//               y_t = W_tt z_t                        k_dirt_rows<false>  operand in the tier numbering already
//             z_(m-1) = W^T y_(m-1) ; x[perm] (+)= z  k_dirt_cols
//             t = m - 1 .. 1:
//               y_j -= sum_i C_t[i, j] z_i, j < lo_t  k_dirt_bwd          rows of C^T: one owner per y_j
//               z_(t-1) = W^T y_(t-1) ; x[perm] (+)=  k_dirt_cols
//   then k_dir_resid and k_dir_step of hip_direct.hip: 4 m - 2 launches in front of them, two at one tier.
//
// The rules are hip_direct.hip's: every launch is gated on the status, the round is read from the state (iters), all
// sums run in a fixed order without atomics, and no workgroup waits on another -- the launches are the only ordering.
//
// k_dirt_rows, on one tier's row range.  The host deals the rows into groups -- consecutive rows that take the same
// number of lanes L, 64 / L of them: one wavefront's work -- and the groups into workgroups of about equal entry
// count; no group, workgroup or window straddles a tier.  The column runs of consecutive rows nest or abut
// (postorder), so a workgroup reads one contiguous window of its operand; it stages the window in LDS once where it
// fits the launch's LDS (cap doubles), else it gathers from global memory -- the same numbers either way.  Lane rule,
// a function of the row's length alone, so the bits do not depend on the dealing: L lanes per row (about four entries
// per lane, 1 .. 64), lane l takes entries l, l + L, ... with fma in ascending order, the lanes are folded by the xor
// butterfly.
//
// k_dirt_cols, on one tier's columns.  A workgroup owns 64 consecutive columns [j0, j1] from the tier's first row on,
// one lane per column in each of its sixteen wavefronts, and visits the rows that reach them: first the rows
// j0 .. j1, then the ancestors of j1 beyond it, run by run from run_end / parent (every ancestor of a window column
// above j1 is an ancestor of j1), up to the root of the tier's tree (parent = n).  Lane j takes part in row k where
// first[k] <= j <= k; a row is one coalesced run of the window's width.  The visited rows are dealt round-robin to
// the sixteen wavefronts in visiting order; each adds its own in ascending k and the sixteen sums are added in
// ascending order.  Nobody walks parent[] vertex by vertex: the largest subtree is numbered last (lsb_direct.c), so a
// walk to the root is a handful of runs.
//
// The coupling kernels take a wavefront per group of consecutive rows with the same lane count L, by the lane rule
// above; a row of thousands of entries is one wavefront's.
#include "hip_kcommon.h"

#define DIRT_HIDDEN __attribute__((visibility("hidden")))
#define DIRT_COLS 64 // columns per workgroup of k_dirt_cols: one wavefront's width
#define DIRT_FLIGHT 8
#define DIRT_CWG 1024 // ... and its threads: sixteen wavefronts share the rows that reach the window

typedef unsigned long long dirt_u64;

// PERM: the operand is b or r in the caller's numbering, read through perm (src: 0 = by the state, 1 = b whatever
// the state says); else it is v in the tier-major numbering
template <bool PERM>
__global__ __launch_bounds__(WG) void k_dirt_rows(const double *__restrict__ vals, const dirt_u64 *__restrict__ woff,
                                                  const unsigned *__restrict__ first,
                                                  const unsigned *__restrict__ perm, const unsigned *__restrict__ grp,
                                                  const unsigned *__restrict__ blk, const unsigned *__restrict__ bwin,
                                                  unsigned cap, const double *__restrict__ b,
                                                  const double *__restrict__ r, double *__restrict__ t,
                                                  const lsb_pcg_state *__restrict__ st, int src) {
  extern __shared__ double win[];
  if (st->status)
    return;
  const double *__restrict__ v = !PERM || src || st->iters == 0 ? b : r;
  const unsigned g0 = blk[blockIdx.x], g1 = blk[blockIdx.x + 1];
  const unsigned wlo = bwin[2 * blockIdx.x], ww = bwin[2 * blockIdx.x + 1];
  const bool staged = ww <= cap;
  if (staged) {
    for (unsigned i = threadIdx.x; i < ww; i += WG)
      win[i] = PERM ? v[perm[wlo + i]] : v[wlo + i];
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
      } else if (PERM) { // (no unroll hint: two dependent loads per entry; measured slower with one on one tier)
        for (unsigned e = l; e < len; e += L)
          acc = fma(w[e], v[perm[f + e]], acc);
      } else {
#pragma unroll 4
        for (unsigned e = l; e < len; e += L)
          acc = fma(w[e], v[f + e], acc);
      }
    }
    for (unsigned m = 32; m >= 1; m >>= 1)
      if (m < L) // (the same L in the whole wavefront)
        acc += __shfl_xor(acc, m, 64);
    if (mine && l == 0)
      t[row0 + sub] = acc;
  }
}

// the columns lo .. hi - 1 of one tier: z_j = (W_tt^T t)_j, stored where z != NULL, and x[perm[j]] = or += z_j (mode:
// 0 = by the state -- round 1 stores x, the others add to it --, 1 = store whatever the state says)
__global__ __launch_bounds__(DIRT_CWG) void k_dirt_cols(unsigned n, unsigned lo, unsigned hi,
                                                        const double *__restrict__ vals,
                                                        const dirt_u64 *__restrict__ woff,
                                                        const unsigned *__restrict__ first,
                                                        const unsigned *__restrict__ perm,
                                                        const unsigned *__restrict__ parent,
                                                        const unsigned *__restrict__ run_end,
                                                        const double *__restrict__ t, double *__restrict__ z,
                                                        double *__restrict__ x, const lsb_pcg_state *__restrict__ st,
                                                        int mode) {
  constexpr unsigned NW = DIRT_CWG / 64;
  __shared__ double part[NW][DIRT_COLS];
  if (st->status)
    return;
  const bool add = !mode && st->iters > 0;
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned j0 = lo + blockIdx.x * DIRT_COLS, j1 = (j0 + DIRT_COLS < hi ? j0 + DIRT_COLS : hi) - 1;
  const unsigned j = j0 + lane;
  const bool active = j <= j1;
  double acc = 0.0;
  // this wavefront's rows k0, k0 + NW, ... <= kend, 64 at a time: lane m fetches what row m of the batch needs (its
  // first column, its offset, t_k), then every lane walks the batch with those broadcast -- the loads of W are
  // independent of one another, DIRT_FLIGHT rows' go out together
  auto visit = [&](unsigned k0, unsigned kend) {
    for (unsigned kb = k0; kb <= kend; kb += 64 * NW) {
      const unsigned km = kb + lane * NW;
      unsigned fm = 0;
      dirt_u64 om = 0;
      double tm = 0.0;
      if (km <= kend)
        fm = first[km], om = woff[km], tm = t[km];
      const unsigned left = (kend - kb) / NW + 1, cnt = left < 64 ? left : 64;
      for (unsigned m0 = 0; m0 < cnt; m0 += DIRT_FLIGHT) {
        double w[DIRT_FLIGHT], tk[DIRT_FLIGHT];
#pragma unroll
        for (unsigned u = 0; u < DIRT_FLIGHT; u++) {
          const unsigned m = m0 + u < cnt ? m0 + u : cnt - 1; // (past the batch: its last row again, not added)
          const unsigned f = __shfl(fm, m, 64), k = kb + m * NW;
          const dirt_u64 o = __shfl(om, m, 64);
          tk[u] = __shfl(tm, m, 64);
          const bool in = active && j >= f && j <= k && m0 + u < cnt;
          w[u] = in ? vals[o + (j - f)] : 0.0;
          tk[u] = in ? tk[u] : 0.0;
        }
#pragma unroll
        for (unsigned u = 0; u < DIRT_FLIGHT; u++)
          acc = fma(tk[u], w[u], acc);
      }
    }
  };
  visit(j0 + wave, j1); // the window's own rows
  unsigned pos = j1 - j0 + 1; // rows visited so far
  for (unsigned p = parent[j1]; p < n;) { // the ancestors of j1 inside the tier, run by run
    const unsigned re = run_end[p];
    visit(p + ((wave + NW - (pos & (NW - 1))) & (NW - 1)), re);
    pos += re - p + 1;
    p = parent[re];
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && active) {
    const unsigned i = perm[j]; // (asked for ahead of the sums and of the branch on z: its latency hides behind them)
    double s = part[0][lane];
#pragma unroll
    for (unsigned w = 1; w < NW; w++)
      s += part[w][lane];
    if (z) // (uniform over the launch: NULL at one tier, where nobody reads z)
      z[j] = s;
    x[i] = add ? x[i] + s : s;
  }
}

// one wavefront per group g0 + (its index in the launch) < g1 of rows of a CSR (offs indexed by row - row_base): the
// row's sum over its entries of vals * v[cols], by the lane rule; returns it in the row's lane 0
__device__ __forceinline__ double dirt_row_sum(const unsigned *__restrict__ offs, const unsigned *__restrict__ cols,
                                               const double *__restrict__ vals, const double *__restrict__ v,
                                               unsigned slot, unsigned L, unsigned l, bool mine, unsigned *len) {
  double acc = 0.0;
  *len = 0;
  if (mine) {
    const unsigned e0 = offs[slot], e1 = offs[slot + 1];
    *len = e1 - e0;
#pragma unroll 4
    for (unsigned e = e0 + l; e < e1; e += L)
      acc = fma(vals[e], v[cols[e]], acc);
  }
  for (unsigned m = 32; m >= 1; m >>= 1)
    if (m < L)
      acc += __shfl_xor(acc, m, 64);
  return acc;
}

// z_i = (P r)_i - sum_j C[i, j] y_j for the rows i of one tier (groups g0 .. g1 - 1 of cgrp)
__global__ __launch_bounds__(WG) void k_dirt_fwd(const unsigned *__restrict__ grp, unsigned g0, unsigned g1,
                                                 unsigned lo1, const unsigned *__restrict__ coffs,
                                                 const unsigned *__restrict__ ccols, const double *__restrict__ cvals,
                                                 const unsigned *__restrict__ perm, const double *__restrict__ b,
                                                 const double *__restrict__ r, const double *__restrict__ y,
                                                 double *__restrict__ z, const lsb_pcg_state *__restrict__ st,
                                                 int src) {
  if (st->status)
    return;
  const double *__restrict__ v = src || st->iters == 0 ? b : r;
  const unsigned g = g0 + blockIdx.x * (WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= g1)
    return;
  const unsigned row0 = grp[2 * g], meta = grp[2 * g + 1];
  const unsigned L = meta & 0xffu, nr = meta >> 8, sub = lane / L, l = lane & (L - 1);
  const bool mine = sub < nr;
  const unsigned i = row0 + sub;
  unsigned len;
  const double acc = dirt_row_sum(coffs, ccols, cvals, y, mine ? i - lo1 : 0u, L, l, mine, &len);
  if (mine && l == 0)
    z[i] = v[perm[i]] - acc;
}

// y_j -= sum_i C[i, j] z_i over the rows i of one tier, for the columns j below it: the rows of that tier's C^T
// (toffs: the tier's own offsets, indexed by j).  A column the tier does not reach is left as it is
__global__ __launch_bounds__(WG) void k_dirt_bwd(const unsigned *__restrict__ grp, unsigned g0, unsigned g1,
                                                 const unsigned *__restrict__ toffs,
                                                 const unsigned *__restrict__ tcols, const double *__restrict__ tvals,
                                                 const double *__restrict__ z, double *__restrict__ y,
                                                 const lsb_pcg_state *__restrict__ st) {
  if (st->status)
    return;
  const unsigned g = g0 + blockIdx.x * (WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= g1)
    return;
  const unsigned row0 = grp[2 * g], meta = grp[2 * g + 1];
  const unsigned L = meta & 0xffu, nr = meta >> 8, sub = lane / L, l = lane & (L - 1);
  const bool mine = sub < nr;
  const unsigned j = row0 + sub;
  unsigned len;
  const double acc = dirt_row_sum(toffs, tcols, tvals, z, mine ? j : 0u, L, l, mine, &len);
  if (mine && l == 0 && len)
    y[j] -= acc;
}

extern "C" {

DIRT_HIDDEN void lsb_k_dirt_rows(const struct lsb_dirt_dev *d, unsigned t, const double *b, const double *r,
                                 const double *v, double *y, const struct lsb_pcg_state *st, int src, void *stream) {
  const struct lsb_dirt_tier *q = &d->t[t];
  if (!q->nblk)
    return;
  const size_t lds = (size_t)q->lds_doubles * sizeof(double);
  if (t == 0)
    k_dirt_rows<true><<<q->nblk, WG, lds, (hipStream_t)stream>>>(d->vals, d->woff, d->first, d->perm, d->grp,
                                                                d->blk + q->blk0, d->bwin + 2 * q->blk0,
                                                                q->lds_doubles, b, r, y, st, src);
  else
    k_dirt_rows<false><<<q->nblk, WG, lds, (hipStream_t)stream>>>(d->vals, d->woff, d->first, d->perm, d->grp,
                                                                 d->blk + q->blk0, d->bwin + 2 * q->blk0,
                                                                 q->lds_doubles, v, v, y, st, src);
}

DIRT_HIDDEN void lsb_k_dirt_cols(const struct lsb_dirt_dev *d, unsigned t, const double *y, double *z, double *x,
                                 const struct lsb_pcg_state *st, int mode, void *stream) {
  const struct lsb_dirt_tier *q = &d->t[t];
  if (q->hi == q->lo)
    return;
  k_dirt_cols<<<div_up(q->hi - q->lo, DIRT_COLS), DIRT_CWG, 0, (hipStream_t)stream>>>(
      d->n, q->lo, q->hi, d->vals, d->woff, d->first, d->perm, d->parent, d->run_end, y, z, x, st, mode);
}

DIRT_HIDDEN void lsb_k_dirt_fwd(const struct lsb_dirt_dev *d, unsigned t, const double *b, const double *r,
                                const double *y, double *z, const struct lsb_pcg_state *st, int src, void *stream) {
  const struct lsb_dirt_tier *q = &d->t[t];
  if (q->cg1 == q->cg0)
    return;
  k_dirt_fwd<<<div_up(q->cg1 - q->cg0, WG / 64), WG, 0, (hipStream_t)stream>>>(
      d->cgrp, q->cg0, q->cg1, d->t[1].lo, d->coffs, d->ccols, d->cvals, d->perm, b, r, y, z, st, src);
}

DIRT_HIDDEN void lsb_k_dirt_bwd(const struct lsb_dirt_dev *d, unsigned t, const double *z, double *y,
                                const struct lsb_pcg_state *st, void *stream) {
  const struct lsb_dirt_tier *q = &d->t[t];
  if (q->tg1 == q->tg0)
    return;
  k_dirt_bwd<<<div_up(q->tg1 - q->tg0, WG / 64), WG, 0, (hipStream_t)stream>>>(
      d->tgrp, q->tg0, q->tg1, d->toffs + q->tbase, d->tcols, d->tvals, z, y, st);
}

} // extern "C"
